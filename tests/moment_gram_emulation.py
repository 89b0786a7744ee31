"""NumPy emulation of the coordinate-weighted Gram call (plfem_moment_grams: k_moment_grams + k_overlap_reduce) for the tests.

The region of a quadrature point is ``GramEmulation.core_mask`` (the assembly's core test), the features are
``CoreGramEmulation.flat_features``, the coordinates are the rule's physical points minus the origin, and the outputs
are those of the C entry.  ``moment_grams16`` evaluates the value-only outputs on the 16-point degree-8 rule of
``quartic_emulation`` instead: a measure of the six-point rule's error on them.
"""
from __future__ import annotations

import numpy as np

from core_gram_emulation import CoreGramEmulation
from quartic_emulation import QuarticEmulation

NAMES = {2: ("M_core_X", "M_core_Y", "M_clad_X", "M_clad_Y", "K_core_X", "K_core_Y", "K_clad_X", "K_clad_Y", "M_XX", "M_XY",
             "M_YY"),
         1: ("M_core_X", "M_core_Y", "M_clad_X", "M_clad_Y", "M_XX", "M_XY", "M_YY")}


class MomentGramEmulation(CoreGramEmulation):
    def moment_grams(self, vals, indexed, geometry, origin=(0.0, 0.0), features=None):
        """dict name -> (k, k): the outputs of plfem_moment_grams (``features``: what ``flat_features(vals, indexed)``
        returned, to share it between core tables and origins)."""
        core = self.core_mask(geometry).reshape(-1)
        w = np.ascontiguousarray(self.basis.dx).reshape(-1)            # (6 ne,), element-major
        X = np.ascontiguousarray(self.basis.qx[0]).reshape(-1) - float(origin[0])
        Y = np.ascontiguousarray(self.basis.qx[1]).reshape(-1) - float(origin[1])
        F = self.flat_features(vals, indexed) if features is None else features

        def g(P, Q, wt):
            return (P * wt[None]) @ Q.T

        def m(wt):
            return sum(g(f[0], f[0], wt) for f in F)                   # u u', or hx hx' + hy hy'

        out = {}
        for nm, reg in (("core", core), ("clad", ~core)):
            for ax, C in (("X", X), ("Y", Y)):
                wt = w * reg * C
                out[f"M_{nm}_{ax}"] = m(wt)
                if len(F) == 2:
                    (hx, hxx, hxy), (hy, hyx, hyy) = F                 # hxy = d hx / dy, hyx = d hy / dx
                    out[f"K_{nm}_{ax}"] = g(hxy, hxy, wt) + g(hyx, hyx, wt) - g(hxx, hyy, wt) - g(hyy, hxx, wt)
        out["M_XX"], out["M_XY"], out["M_YY"] = m(w * X * X), m(w * X * Y), m(w * Y * Y)
        return {nm: out[nm] for nm in NAMES[len(F)]}

    def moment_grams16(self, vals, indexed, origin=(0.0, 0.0)):
        """M, M_X, M_Y, M_XX, M_XY, M_YY over both regions on the 16-point degree-8 rule: dict name -> (k, k)."""
        from pl_fem_vectoriel_amd.nonlinear import QUAD16_X
        q = QuarticEmulation.__new__(QuarticEmulation)
        q.__dict__.update(self.__dict__)
        U = q.values16(vals, indexed)                                  # (ncomp, k, ne, 16)
        k = vals.shape[1]
        w = q.weights16().reshape(-1)
        p0 = self.mesh.p[:, self.mesh.t[0]]
        J = self.basis.J
        qx = p0[:, :, None] + J[:, 0][:, :, None] * QUAD16_X[0][None, None] + J[:, 1][:, :, None] * QUAD16_X[1][None, None]
        X, Y = qx[0].reshape(-1) - float(origin[0]), qx[1].reshape(-1) - float(origin[1])
        u = U.reshape(U.shape[0], k, -1)

        def m(wt):
            return sum((u[c] * wt[None]) @ u[c].T for c in range(u.shape[0]))

        return {"M": m(w), "M_X": m(w * X), "M_Y": m(w * Y), "M_XX": m(w * X * X), "M_XY": m(w * X * Y), "M_YY": m(w * Y * Y)}
