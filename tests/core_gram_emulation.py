"""NumPy emulation of the per-core Gram call (plfem_core_grams: k_core_owner, the compaction, k_core_grams) for the tests.

The owner of a quadrature point is the highest-index closed disc that holds it, with the arithmetic of
``GramEmulation.core_mask`` (the assembly's core test); the features are ``GramEmulation.features``; the outputs and
``points`` are those of the C entry.
"""
from __future__ import annotations

import numpy as np

from gram_emulation import GramEmulation

NAMES = {2: ("Mx", "My", "K"), 1: ("M",)}


class CoreGramEmulation(GramEmulation):
    def core_owner(self, geometry):
        """(ne, 6) int: the highest index of a closed core disc holding the quadrature point, -1 in the cladding."""
        qx, qy = self.basis.qx
        owner = np.full(qx.shape, -1, dtype=np.int64)
        pos = np.atleast_2d(np.asarray(geometry.positions, dtype=np.float64))
        rad = np.asarray(geometry.core_radii, dtype=np.float64).reshape(-1)
        for c, ((cx, cy), r) in enumerate(zip(pos, rad)):
            owner[(qx - cx) ** 2 + (qy - cy) ** 2 <= r * r] = c
        return owner

    def flat_features(self, vals, indexed):
        """``GramEmulation.features`` as contiguous (k, 6 ne) arrays, element-major like the device's point index: they
        do not depend on the core table, so one evaluation serves many tables."""
        k = vals.shape[1]
        return [[np.ascontiguousarray(f).reshape(k, -1) for f in comp] for comp in self.features(vals, indexed)]

    def core_grams(self, vals, indexed, geometry, features=None):
        """dict name -> (ncore, k, k) and "points" (ncore,) int64: the outputs of plfem_core_grams (``features``: what
        ``flat_features(vals, indexed)`` returned, to share it between core tables)."""
        k = vals.shape[1]
        owner = self.core_owner(geometry)
        ncore = np.atleast_2d(np.asarray(geometry.positions)).shape[0]
        w = np.ascontiguousarray(self.basis.dx).reshape(-1)           # (6 ne,), element-major
        F = self.flat_features(vals, indexed) if features is None else features

        def g(X, Y, pts):                                              # the sum over the points pts of the rule
            return (X[:, pts] * w[pts][None]) @ Y[:, pts].T

        out = {nm: np.zeros((ncore, k, k)) for nm in NAMES[vals.shape[0]]}
        out["points"] = np.array([(owner == c).sum() for c in range(ncore)], dtype=np.int64)
        for c in range(ncore):
            pts = np.flatnonzero(owner.reshape(-1) == c)
            if vals.shape[0] == 1:
                (u, _, _), = F
                out["M"][c] = g(u, u, pts)
                continue
            (hx, hxx, hxy), (hy, hyx, hyy) = F                         # hxy = d hx / dy, hyx = d hy / dx
            out["Mx"][c] = g(hx, hx, pts)
            out["My"][c] = g(hy, hy, pts)
            out["K"][c] = g(hxy, hxy, pts) + g(hyx, hyx, pts) - g(hxx, hyy, pts) - g(hyy, hxx, pts)
        return out
