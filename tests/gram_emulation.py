"""NumPy emulation of the same-mesh Gram kernel (k_mode_grams) for the tests.

Independent of the library: values and physical gradients of the P2 basis at the six-point rule come from
``oracle.p2.P2Basis``, the DOF numbering and the interior map from ``fields_emulation.Emulation``, and the region of a
quadrature point is the closed-disc core test of the assembly.
"""
from __future__ import annotations

import numpy as np

from fields_emulation import Emulation
from oracle.p2 import PHI_Q

NAMES = {2: ("M_core", "M_clad", "K_core", "K_clad", "D"), 1: ("M_core", "M_clad", "S")}


class GramEmulation(Emulation):
    def core_mask(self, geometry):
        """(ne, 6) True where the quadrature point lies in a closed core disc."""
        qx, qy = self.basis.qx
        inside = np.zeros(qx.shape, dtype=bool)
        pos = np.atleast_2d(np.asarray(geometry.positions, dtype=np.float64))
        rad = np.asarray(geometry.core_radii, dtype=np.float64).reshape(-1)
        for (cx, cy), r in zip(pos, rad):
            inside |= (qx - cx) ** 2 + (qy - cy) ** 2 <= r * r
        return inside

    def features(self, vals, indexed):
        """Per component c: (value, d/dx, d/dy), each (k, ne, 6), of the modes vals (ncomp, k, nrows)."""
        rows = self._rows(indexed)
        valid = rows >= 0
        r = np.where(valid, rows, 0)
        gx, gy = self.basis.grad[:, 0], self.basis.grad[:, 1]          # (6, ne, 6)
        out = []
        for c in range(vals.shape[0]):
            g = vals[c][:, r] * valid[None]                            # (k, 6, ne)
            out.append((np.einsum("aq,kae->keq", PHI_Q, g), np.einsum("aeq,kae->keq", gx, g),
                        np.einsum("aeq,kae->keq", gy, g)))
        return out

    def grams(self, vals, indexed, geometry):
        """dict name -> (k, k), the outputs of plfem_mode_grams."""
        k = vals.shape[1]
        core = self.core_mask(geometry)
        w = self.basis.dx                                              # (ne, 6)
        wc, wl = (w * core).reshape(-1), (w * ~core).reshape(-1)

        def g(X, Y, wt):
            return (X.reshape(k, -1) * wt[None]) @ Y.reshape(k, -1).T

        F = self.features(vals, indexed)
        if vals.shape[0] == 1:
            (u, ux, uy), = F
            wa = w.reshape(-1)
            return {"M_core": g(u, u, wc), "M_clad": g(u, u, wl), "S": g(ux, ux, wa) + g(uy, uy, wa)}
        (hx, hxx, hxy), (hy, hyx, hyy) = F                             # hxy = d hx / dy, hyx = d hy / dx
        out = {}
        for nm, wt in (("core", wc), ("clad", wl)):
            out["M_" + nm] = g(hx, hx, wt) + g(hy, hy, wt)
            out["K_" + nm] = g(hxy, hxy, wt) + g(hyx, hyx, wt) - g(hxx, hyy, wt) - g(hyy, hxx, wt)
        wa = w.reshape(-1)
        out["D"] = g(hxx, hxx, wa) + g(hyy, hyy, wa) + g(hxy, hyx, wa) + g(hyx, hxy, wa)
        return out
