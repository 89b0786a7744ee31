"""NumPy emulation of the profile Gram call (plfem_profile_grams: k_profile_grams + k_overlap_reduce) for the tests.

Built on ``GramEmulation``: the same features at the six-point rule; in place of the region of a quadrature point, the
permittivity of the index profile there (``IndexProfile.epsilon`` at ``P2Basis.qx``, the point as the assembly forms it)
gives the point's weight: 1 / eps for vectorial records, eps for scalar ones.
"""
from __future__ import annotations

import numpy as np

from gram_emulation import GramEmulation

NAMES = {2: ("M", "M_w", "K_w", "D"), 1: ("M", "M_w", "S")}


class ProfileGramEmulation(GramEmulation):
    def profile_weight(self, profile, ncomp):
        """(ne, 6): the material weight of every quadrature point."""
        qx, qy = self.basis.qx
        eps = profile.epsilon(qx, qy)
        return 1.0 / eps if ncomp == 2 else eps

    def profile_grams(self, vals, indexed, profile):
        """dict name -> (k, k), the outputs of plfem_profile_grams."""
        k = vals.shape[1]
        w = self.basis.dx                                              # (ne, 6)
        wa, ww = w.reshape(-1), (w * self.profile_weight(profile, vals.shape[0])).reshape(-1)

        def g(X, Y, wt):
            return (X.reshape(k, -1) * wt[None]) @ Y.reshape(k, -1).T

        F = self.features(vals, indexed)
        if vals.shape[0] == 1:
            (u, ux, uy), = F
            return {"M": g(u, u, wa), "M_w": g(u, u, ww), "S": g(ux, ux, wa) + g(uy, uy, wa)}
        (hx, hxx, hxy), (hy, hyx, hyy) = F                             # hxy = d hx / dy, hyx = d hy / dx
        return {"M": g(hx, hx, wa) + g(hy, hy, wa), "M_w": g(hx, hx, ww) + g(hy, hy, ww),
                "K_w": g(hxy, hxy, ww) + g(hyx, hyx, ww) - g(hxx, hyy, ww) - g(hyy, hxx, ww),
                "D": g(hxx, hxx, wa) + g(hyy, hyy, wa) + g(hxy, hyx, wa) + g(hyx, hxy, wa)}
