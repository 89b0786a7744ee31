"""NumPy emulation of the pixel-density call (plfem_index_map_gradients: k_map_point_keys + sort + k_point_densities +
k_map_gather) for the tests, in point order.

Built on ``ProfileGramEmulation``: the same features at the six-point rule and the same material weight ``w`` (1 / eps for
vectorial records, eps for scalar ones).  A quadrature point contributes when it lies in the closed extent of the
profile's map and no layer holds it (``IndexProfile._placement``: the membership and the cell of ``IndexProfile.epsilon``);
it adds ``c = |det J| w_q dw`` -- ``dw = -(w w)`` or 1 -- times the density of the field times a corner weight to the four
nodes of its cell, point after point (``np.add.at``), which is what the sorted lists of the kernel add up to.
"""
from __future__ import annotations

import numpy as np

from profile_gram_emulation import ProfileGramEmulation

NAMES = {2: ("M_px", "K_px"), 1: ("M_px",)}


class MapGradientEmulation(ProfileGramEmulation):
    def contributions(self, profile, ncomp):
        """``(live, i0, j0, a, b, c)``: the flat indices (element-major, 6 per element) of the contributing points, their
        cell and weights, and ``c = |det J| w_q dw``."""
        qx, qy = self.basis.qx
        top, _, inside, cell = profile._placement(qx, qy)
        i0 = np.zeros(qx.shape, dtype=np.int64)
        j0 = np.zeros(qx.shape, dtype=np.int64)
        a, b = np.zeros(qx.shape), np.zeros(qx.shape)
        i0[inside], j0[inside], a[inside], b[inside] = cell
        live = inside & (top < 0)
        w = self.profile_weight(profile, ncomp)
        dw = -(w * w) if ncomp == 2 else np.ones_like(w)
        c = self.basis.dx * dw
        f = np.nonzero(live.reshape(-1))[0]
        return f, i0.reshape(-1)[f], j0.reshape(-1)[f], a.reshape(-1)[f], b.reshape(-1)[f], c.reshape(-1)[f]

    def point_densities(self, vals, indexed):
        """(nout, k, ne * 6): m (and kk) of every field at every point."""
        k = vals.shape[1]
        F = self.features(vals, indexed)
        if vals.shape[0] == 1:
            (u, _, _), = F
            return (u * u).reshape(1, k, -1)
        (hx, hxx, hxy), (hy, hyx, hyy) = F                             # hxy = d hx / dy, hyx = d hy / dx
        return np.stack([hx * hx + hy * hy, hxy * hxy + hyx * hyx - 2.0 * (hxx * hyy)]).reshape(2, k, -1)

    def map_gradients(self, vals, indexed, profile):
        """``(out (k, nout, ny, nx), support (ny, nx) int32)``: out_host and support_host of plfem_index_map_gradients."""
        ncomp, k = vals.shape[0], vals.shape[1]
        ny, nx = profile.index_map[0].shape
        f, i0, j0, a, b, c = self.contributions(profile, ncomp)
        dens = self.point_densities(vals, indexed)[:, :, f]            # (nout, k, nlive)
        nout = dens.shape[0]
        out = np.zeros((k, nout, ny, nx))
        support = np.zeros((ny, nx), dtype=np.int32)
        a1, b1 = 1.0 - a, 1.0 - b
        for dj, di, beta in ((0, 0, a1 * b1), (0, 1, a * b1), (1, 0, a1 * b), (1, 1, a * b)):
            np.add.at(support, (j0 + dj, i0 + di), 1)
            for r in range(k):
                for o in range(nout):
                    np.add.at(out[r, o], (j0 + dj, i0 + di), (c * beta) * dens[o, r])
        return out, support

    def named(self, out, support):
        """``out`` and ``support`` under the names of ModeFields.index_map_densities."""
        res = {nm: out[:, i] for i, nm in enumerate(NAMES[out.shape[1]])}
        res["support"] = support
        return res
