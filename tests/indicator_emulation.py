"""NumPy restatement of the a-posteriori error indicators (plfem_mode_indicators: k_mode_indicators) for the tests.

Independent of the library: the P2 numbering, the affine maps, the six-point rule and the basis come from ``oracle.p2``,
the interior map from ``fields_emulation.Emulation``.  For mode m with pencil eigenvalue lambda, element T and its edges e

    eta2[m][T] = |det J_T| sum_q |det J_T| w_q |r(x_q)|^2 + sum_e c_e |e| int_e |[F . n]|^2 ds

with the edge integral on the two-point Gauss rule s = 1/2 -+ 1/(2 sqrt 3), c_e = 1/2 inside, on the outer boundary 1
(scalar) or 0 (vectorial); edges run from the lower to the higher vertex id and the edge point is ``x_lo + s * (x_hi -
x_lo)``, every operation rounded on its own, so both neighbours -- and the device -- see the same permittivity there.

    scalar     F = grad u,  r = -lap u - (k0^2 eps + lambda) u
    vectorial  w = 1 / eps,
               F_x = (-w dy hy + alpha dx hx,  w dy hx + alpha dx hy),  F_y = (w dx hy + alpha dy hx, -w dx hx + alpha dy hy),
               r_c = -div F_c - (k0^2 + lambda w) h_c, div F with w frozen at the point

``signed_residual`` sums the same pieces with their signs against the basis functions: the assembled ``(A - lambda B) h``.
"""
from __future__ import annotations

import numpy as np

from fields_emulation import Emulation
from oracle.p2 import LOCAL_EDGES, PHI_Q, p2_basis

GAUSS = (0.5 - 0.5 / np.sqrt(3), 0.5 + 0.5 / np.sqrt(3))
# reference Hessians of the six basis functions: xi xi, eta eta, xi eta
H00 = np.array([4.0, 4.0, 0.0, -8.0, 0.0, 0.0])
H11 = np.array([4.0, 0.0, 4.0, 0.0, 0.0, -8.0])
H01 = np.array([4.0, 0.0, 0.0, -4.0, 4.0, -4.0])


def eps_of(geometry):
    """``eps(x, y)`` (real) of a geometry: its index profile if it carries one, otherwise n_core^2 in the closed core
    discs (the reference's ``(x - cx)**2 + (y - cy)**2 <= r**2``) and n_clad^2 outside."""
    prof = getattr(geometry, "index_profile", None)
    if prof is not None:
        return prof.epsilon
    pos = np.atleast_2d(np.asarray(geometry.positions, dtype=np.float64)).reshape(-1, 2)
    rad = np.asarray(geometry.core_radii, dtype=np.float64).reshape(-1)

    def eps(x, y):
        inside = np.zeros(np.shape(x), dtype=bool)
        for (cx, cy), r in zip(pos, rad):
            inside |= (x - cx) ** 2 + (y - cy) ** 2 <= r * r
        return np.where(inside, float(geometry.n_core) ** 2, float(geometry.n_clad) ** 2)
    return eps


def edge_ref_point(l, s):
    """Reference coordinates of the point at parameter s (lower -> higher vertex) of local edge l."""
    return ((s, 0.0), (1.0 - s, s), (0.0, s))[l]


class IndicatorEmulation(Emulation):
    def __init__(self, p, t):
        super().__init__(p, t)
        mesh, ne = self.mesh, self.mesh.t.shape[1]
        t2f, nf = mesh.t2f, mesh.facets.shape[1]
        f2t = -np.ones((nf, 2), dtype=np.int64)
        f2l = -np.ones((nf, 2), dtype=np.int64)
        for l in range(3):
            for e in range(ne):
                f = t2f[l, e]
                s = 0 if f2t[f, 0] < 0 else 1
                f2t[f, s], f2l[f, s] = e, l
        e_ids = np.arange(ne)
        self.nbr = np.empty((3, ne), dtype=np.int64)           # the element across local edge l, -1 = outer boundary
        self.nbr_l = np.empty((3, ne), dtype=np.int64)         # ... and the neighbour's local index of that edge
        for l in range(3):
            first = f2t[t2f[l], 0] == e_ids
            self.nbr[l] = np.where(first, f2t[t2f[l], 1], f2t[t2f[l], 0])
            self.nbr_l[l] = np.where(first, f2l[t2f[l], 1], f2l[t2f[l], 0])
        p_, t_ = mesh.p, mesh.t
        self.lo = np.stack([p_[:, t_[a]] for a, _ in LOCAL_EDGES])          # (3, 2, ne)
        self.tv = np.stack([p_[:, t_[b]] - p_[:, t_[a]] for a, b in LOCAL_EDGES])
        # outward sign of (t_y, -t_x): away from the opposite vertex
        cent = p_[:, t_].mean(axis=1)
        mid = self.lo + 0.5 * self.tv
        self.out_sign = np.sign((mid[:, 0] - cent[0]) * self.tv[:, 1] - (mid[:, 1] - cent[1]) * self.tv[:, 0])   # (3, ne)

    # -- points ----------------------------------------------------------------------------------------------
    def edge_points(self):
        """x, y (3, ne, 2): x_lo + s (x_hi - x_lo), the product and the sum rounded on their own."""
        s = np.array(GAUSS)
        return (self.lo[:, 0, :, None] + s[None, None, :] * self.tv[:, 0, :, None],
                self.lo[:, 1, :, None] + s[None, None, :] * self.tv[:, 1, :, None])

    def _local(self, vals, indexed):
        """(ncomp, k, 6, ne): the element coefficients, 0 for a boundary DOF of an indexed record."""
        rows = self._rows(indexed)
        valid = rows >= 0
        return vals[:, :, np.where(valid, rows, 0)] * valid[None, None]

    def _hess(self, U):
        """uxx, uxy, uyy (ncomp, k, ne) of the element coefficients U (ncomp, k, 6, ne)."""
        inv = self.basis.invJ                                    # d/dx_r = sum_c inv[c, r] d_c

        def d2(r, s):
            b = (np.outer(H00, inv[0, r] * inv[0, s]) + np.outer(H11, inv[1, r] * inv[1, s])
                 + np.outer(H01, inv[0, r] * inv[1, s] + inv[1, r] * inv[0, s]))          # (6, ne)
            return np.einsum("ae,ckae->cke", b, U)
        return d2(0, 0), d2(0, 1), d2(1, 1)

    def _edge_grad(self, U, elem, loc, g):
        """ux, uy (ncomp, k, n) at Gauss point g of local edge loc[i] of element elem[i], U (ncomp, k, 6, ne)."""
        xi = np.array([edge_ref_point(l, GAUSS[g])[0] for l in range(3)])[loc]
        et = np.array([edge_ref_point(l, GAUSS[g])[1] for l in range(3)])[loc]
        _, dph = p2_basis(xi, et)                                # (6, 2, n)
        gr = np.einsum("crn,acn->arn", self.basis.invJ[:, :, elem], dph)
        Ue = U[:, :, :, elem]
        return np.einsum("an,ckan->ckn", gr[:, 0], Ue), np.einsum("an,ckan->ckn", gr[:, 1], Ue)

    # -- the pieces ------------------------------------------------------------------------------------------
    def pieces(self, vals, indexed, lam, k0, alpha, eps_fn):
        """``r`` (ncomp, k, ne, 6): the strong residual at the quadrature points; ``flux`` (2 sides, ncomp, k, 3, ne, 2): F .
        (t_y, -t_x) at the edge points from this element (side 0) and from its neighbour (side 1; 0 on the boundary)."""
        vals = np.asarray(vals, dtype=np.float64)
        lam = np.asarray(lam, dtype=np.float64)
        ncomp, k, _ = vals.shape
        ne = self.mesh.t.shape[1]
        U = self._local(vals, indexed)
        uxx, uxy, uyy = self._hess(U)
        uq = np.einsum("aq,ckae->ckeq", PHI_Q, U)
        qx, qy = self.basis.qx
        eps = np.asarray(eps_fn(qx, qy), dtype=np.float64)       # (ne, 6)
        L = lam[:, None, None]
        if ncomp == 1:
            r = (-(uxx + uyy)[..., None] - (k0 ** 2 * eps[None] + L)[None] * uq)
        else:
            w = (1.0 / eps)[None]                                # (1, ne, 6)
            hx, hy = 0, 1
            dfx = (-w * uxy[hy][..., None] + alpha * uxx[hx][..., None] + w * uyy[hx][..., None] + alpha * uxy[hy][..., None])
            dfy = (w * uxx[hy][..., None] + alpha * uxy[hx][..., None] - w * uxy[hx][..., None] + alpha * uyy[hy][..., None])
            r = np.stack([-dfx - (k0 ** 2 + L * w) * uq[hx], -dfy - (k0 ** 2 + L * w) * uq[hy]])
        ex, ey = self.edge_points()
        eeps = np.asarray(eps_fn(ex, ey), dtype=np.float64)      # (3, ne, 2)
        flux = np.zeros((2, ncomp, k, 3, ne, 2))
        e_ids = np.arange(ne)
        for l in range(3):
            tx, ty = self.tv[l, 0], self.tv[l, 1]
            has = self.nbr[l] >= 0
            for g in range(2):
                for side in range(2):
                    elem = e_ids if side == 0 else np.where(has, self.nbr[l], 0)
                    loc = np.full(ne, l) if side == 0 else np.where(has, self.nbr_l[l], 0)
                    ux, uy = self._edge_grad(U, elem, loc, g)
                    if ncomp == 1:
                        f = (ux * ty - uy * tx)
                    else:
                        w = 1.0 / eeps[l, :, g]
                        fxx, fxy = -w * uy[1] + alpha * ux[0], w * uy[0] + alpha * ux[1]
                        fyx, fyy = w * ux[1] + alpha * uy[0], -w * ux[0] + alpha * uy[1]
                        f = np.stack([fxx * ty - fxy * tx, fyx * ty - fyy * tx])
                    flux[side, :, :, l, :, g] = f if side == 0 else f * has
        return {"r": r, "flux": flux}

    def eta2_parts(self, vals, indexed, lam, k0, alpha, eps_fn):
        """(residual part, jump part), each (k, ne)."""
        P = self.pieces(vals, indexed, lam, k0, alpha, eps_fn)
        ncomp = np.shape(vals)[0]
        res = self.basis.absdet[None] * np.einsum("eq,ckeq->ke", self.basis.dx, P["r"] ** 2)
        flux = P["flux"]
        boundary = self.nbr < 0                                  # (3, ne)
        jump = np.where(boundary[None, None, :, :, None], flux[0], flux[0] - flux[1])
        c_e = np.where(boundary, 1.0 if ncomp == 1 else 0.0, 0.5)
        # c_e |e| int (F . n)^2 ds = c_e |e| (|e| / 2) sum_g (F . (t_y, -t_x) / |e|)^2
        tl = np.hypot(self.tv[:, 0], self.tv[:, 1])              # (3, ne)
        integral = 0.5 * tl[None, None, :, :] * np.sum((jump / tl[None, None, :, :, None]) ** 2, axis=-1)
        jmp = np.einsum("le,ckle->ke", c_e * tl, integral)
        return res, jmp

    def eta2(self, vals, indexed, lam, k0, alpha, eps_fn):
        res, jmp = self.eta2_parts(vals, indexed, lam, k0, alpha, eps_fn)
        return res + jmp

    def signed_residual(self, vals, lam, k0, alpha, eps_fn):
        """(ncomp, k, N): sum over the elements of int r phi_i plus the outward flux int F . n phi_i over all three edges of
        every element, boundary edges included -- (A - lambda B) h of the unrestricted matrices (vals on all N DOFs)."""
        P = self.pieces(vals, False, lam, k0, alpha, eps_fn)
        ncomp, k, _ = np.shape(vals)
        ed = self.basis.element_dofs
        out = np.zeros((ncomp, k, self.N))
        vol = np.einsum("eq,ckeq,aq->ckae", self.basis.dx, P["r"], PHI_Q)
        for a in range(6):
            for c in range(ncomp):
                for m in range(k):
                    np.add.at(out[c, m], ed[a], vol[c, m, a])
        for l in range(3):
            for g in range(2):
                xi, et = edge_ref_point(l, GAUSS[g])
                ph, _ = p2_basis(np.array(xi), np.array(et))     # (6,)
                # int_e F . n phi ds = (|e| / 2) sum_g F . n phi = (1 / 2) sum_g F . (t_y, -t_x) sign phi
                f = 0.5 * P["flux"][0][:, :, l, :, g] * self.out_sign[l][None, None]
                for a in range(6):
                    if ph[a] == 0.0:
                        continue
                    for c in range(ncomp):
                        for m in range(k):
                            np.add.at(out[c, m], ed[a], f[c, m] * ph[a])
        return out
