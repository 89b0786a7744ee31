"""NumPy emulation of the velocity Gram call (plfem_velocity_grams: k_velocity_flag, k_velocity_count + k_velocity_fill,
k_velocity_grams + k_overlap_reduce + k_velocity_symmetrise) for the tests.

Built on ``ProfileGramEmulation``: the same features at the six-point rule, the element geometry of ``oracle.p2.P2Basis`` and the
material of ``geometry.epsilon`` at ``P2Basis.qx`` (its real part: what the eigenmode path reads).  Per velocity V (nv, 2)
and element: ``G[a, b] = dV_a / dx_b`` from the three vertex velocities and adj(J) / det J, ``tr = G_xx + G_yy``, and with ``gt(f) = -G^T
grad f + (tr / 2) grad f`` every gradient form changes by ``P + P^T``, P the form with gt on the row mode; a mass form by
``sum tr |det J| w_q c u_m . u_n``.  ``count``: the elements with any entry of G non-zero.
"""
from __future__ import annotations

import numpy as np

from profile_gram_emulation import ProfileGramEmulation

NAMES = {2: ("dK_w", "dD", "dM", "dM_w"), 1: ("dS", "dM", "dM_w")}


class VelocityGramEmulation(ProfileGramEmulation):
    def velocity_gradient(self, V):
        """(ne, 2, 2): G[e, a, b] = dV_a / dx_b of the P1 field V (nv, 2)."""
        t, J, det = self.mesh.t, self.basis.J, self.basis.detJ         # J[r, c, e] = d x_r / d xi_c
        d1, d2 = V[t[1]] - V[t[0]], V[t[2]] - V[t[0]]                  # (ne, 2)
        G = np.empty((t.shape[1], 2, 2))
        for a in range(2):                                             # [d1, d2] adj(J) / det J: V = x gives the identity exactly
            G[:, a, 0] = (d1[:, a] * J[1, 1] - d2[:, a] * J[1, 0]) / det
            G[:, a, 1] = (d2[:, a] * J[0, 0] - d1[:, a] * J[0, 1]) / det
        return G

    def material_weight(self, geometry, ncomp):
        """(ne, 6): 1 / eps (vectorial) or eps (scalar) of every quadrature point."""
        qx, qy = self.basis.qx
        eps = np.real(geometry.epsilon(qx, qy))
        return 1.0 / eps if ncomp == 2 else eps

    def velocity_grams(self, vals, indexed, geometry, velocities):
        """(out (nvel, nout, k, k), count (nvel,)): out_host and count_host of plfem_velocity_grams."""
        ncomp, k = vals.shape[0], vals.shape[1]
        F = self.features(vals, indexed)
        wq = self.basis.dx                                             # (ne, 6)
        wm = wq * self.material_weight(geometry, ncomp)
        outs, counts = [], []
        for V in np.asarray(velocities, dtype=np.float64):
            G = self.velocity_gradient(V)
            counts.append(int(np.count_nonzero((G != 0).any(axis=(1, 2)))))
            tr = G[:, 0, 0] + G[:, 1, 1]

            def gt(fx, fy):
                """the transformed gradient of fields (k, ne, 6)"""
                h = 0.5 * tr[None, :, None]
                g = lambda a, b: G[None, :, a, b, None]
                return h * fx - (g(0, 0) * fx + g(1, 0) * fy), h * fy - (g(0, 1) * fx + g(1, 1) * fy)

            def form(X, Y, w):
                return (X.reshape(k, -1) * w.reshape(-1)[None]) @ Y.reshape(k, -1).T

            def sym(P):
                return P + P.T

            wt, wtm = tr[:, None] * wq, tr[:, None] * wm
            if ncomp == 1:
                (u, ux, uy), = F
                tx, ty = gt(ux, uy)
                outs.append(np.stack([sym(form(tx, ux, wq) + form(ty, uy, wq)), form(u, u, wt), form(u, u, wtm)]))
                continue
            (hx, hxx, hxy), (hy, hyx, hyy) = F                         # hxy = d hx / dy, hyx = d hy / dx
            txx, txy = gt(hxx, hxy)                                    # transformed gradient of hx
            tyx, tyy = gt(hyx, hyy)                                    # ... of hy
            PK = form(txy, hxy, wm) + form(tyx, hyx, wm) - form(txx, hyy, wm) - form(tyy, hxx, wm)
            PD = form(txx, hxx, wq) + form(tyy, hyy, wq) + form(txy, hyx, wq) + form(tyx, hxy, wq)
            outs.append(np.stack([sym(PK), sym(PD), form(hx, hx, wt) + form(hy, hy, wt),
                                  form(hx, hx, wtm) + form(hy, hy, wtm)]))
        return np.stack(outs), np.array(counts, dtype=np.int64)

    def named(self, out):
        """``out`` (nvel, nout, k, k) under the names of ModeFields.velocity_grams."""
        return {nm: out[:, i] for i, nm in enumerate(NAMES[2 if out.shape[1] == 4 else 1])}
