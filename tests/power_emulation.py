"""NumPy emulation of the electric-field kernels (plfem_flux_grams: k_flux_grams + k_overlap_reduce; plfem_sample_efields:
k_sample_efields) for the tests.

Built on ``GramEmulation`` / ``Emulation``: the same DOF numbering, interior map, features at the six-point rule, core
test and brute-force point location.  What is added: the physical Hessians of the six basis functions (constant per
element: the J^-1 products applied to the reference Hessians), the permittivity of a geometry at a point
(``indicator_emulation.eps_of``: its index profile if it carries one, else its discs at n_core on n_clad), and

    gx = -(hx,xx + hy,xy)      gy = -(hx,xy + hy,yy)
    Ex = w (beta hy + gy / beta) / k0,  Ey = -w (beta hx + gx / beta) / k0,  Ez_im = -w (dx hy - dy hx) / k0,
    Sz = (Ex hy - Ey hx) / 2,          w = 1 / eps
    M_w[m][n] = int w (hx_m hx_n + hy_m hy_n),   G_w[m][n] = int w (gx_m hx_n + gy_m hy_n),

the Grams split by the closed core discs of the geometry (none: everything is "rest").
"""
from __future__ import annotations

import numpy as np

from gram_emulation import GramEmulation
from indicator_emulation import H00, H01, H11, eps_of
from oracle.p2 import p2_basis

NAMES = ("M_w_core", "M_w_rest", "G_w_core", "G_w_rest")
E_NAMES = ("Ex", "Ey", "Ez_im", "Sz")


class PowerEmulation(GramEmulation):
    def basis_hess(self, e=None):
        """(3, 6, n): xx, xy, yy of the six basis functions on the elements ``e`` (default: all)."""
        inv = self.basis.invJ if e is None else self.basis.invJ[:, :, e]      # inv[r, c] = d xi_r / d x_c
        i00, i01, i10, i11 = inv[0, 0], inv[0, 1], inv[1, 0], inv[1, 1]
        h00, h01, h11 = H00[:, None], H01[:, None], H11[:, None]
        return np.stack([i00 * i00 * h00 + 2.0 * (i00 * i10) * h01 + i10 * i10 * h11,
                         i00 * i01 * h00 + (i00 * i11 + i10 * i01) * h01 + i10 * i11 * h11,
                         i01 * i01 * h00 + 2.0 * (i01 * i11) * h01 + i11 * i11 * h11])

    def region_mask(self, geometry):
        """(ne, 6) True where the quadrature point lies in a closed core disc of the geometry; all False without discs."""
        if not all(hasattr(geometry, a) for a in ("positions", "core_radii")) or np.size(geometry.core_radii) == 0:
            return np.zeros(self.basis.dx.shape, dtype=bool)
        return self.core_mask(geometry)

    def _coeffs(self, vals, indexed, e=None):
        """(2, k, 6, n): the element coefficients on the elements ``e``, 0 for a boundary DOF of an indexed record."""
        rows = self._rows(indexed) if e is None else self._rows(indexed)[:, e]
        valid = rows >= 0
        r = np.where(valid, rows, 0)
        return np.stack([vals[c][:, r] * valid[None] for c in range(2)])

    def flux_grams(self, vals, indexed, geometry):
        """dict name -> (k, k), the outputs of plfem_flux_grams, for vals (2, k, nrows)."""
        k = vals.shape[1]
        (hx, _, _), (hy, _, _) = self.features(vals, indexed)                  # (k, ne, 6)
        H = self.basis_hess()                                                  # (3, 6, ne)
        c = self._coeffs(vals, indexed)                                        # (2, k, 6, ne)
        gx = -(np.einsum("ae,kae->ke", H[0], c[0]) + np.einsum("ae,kae->ke", H[1], c[1]))
        gy = -(np.einsum("ae,kae->ke", H[1], c[0]) + np.einsum("ae,kae->ke", H[2], c[1]))
        gx = np.broadcast_to(gx[:, :, None], hx.shape)
        gy = np.broadcast_to(gy[:, :, None], hx.shape)
        qx, qy = self.basis.qx
        w = self.basis.dx / np.real(eps_of(geometry)(qx, qy))                  # (ne, 6): |det J| w_q / eps
        core = self.region_mask(geometry)

        def g(X, Y, wt):
            return (X.reshape(k, -1) * wt.reshape(-1)[None]) @ Y.reshape(k, -1).T

        out = {}
        for nm, wt in (("core", w * core), ("rest", w * ~core)):
            out["M_w_" + nm] = g(hx, hx, wt) + g(hy, hy, wt)
            out["G_w_" + nm] = g(gx, hx, wt) + g(gy, hy, wt)
        return out

    def sample_e(self, vals, pts, indexed, beta, k0, geometry, located=None):
        """vals (2, k, nrows) -> out (4, k, npts) = Ex, Ey, Ez_im, Sz, eps (npts,), element (npts,)."""
        elem, xi, eta, near = self.locate(pts) if located is None else located
        k, npts = vals.shape[1], elem.size
        out = np.zeros((4, k, npts))
        eps = np.zeros(npts)
        ok = np.nonzero(elem >= 0)[0]
        if ok.size == 0:
            return out, eps, elem
        e = elem[ok]
        x, y = np.asarray(pts[0], dtype=np.float64)[ok], np.asarray(pts[1], dtype=np.float64)[ok]
        eps[ok] = np.real(eps_of(geometry)(x, y))
        w = 1.0 / eps[ok]
        phi, dphi = p2_basis(xi[ok], eta[ok])                                  # (6, n), (6, 2, n)
        inv = self.basis.invJ[:, :, e]
        gx = dphi[:, 0] * inv[0, 0] + dphi[:, 1] * inv[1, 0]
        gy = dphi[:, 0] * inv[0, 1] + dphi[:, 1] * inv[1, 1]
        H = self.basis_hess(e)                                                 # (3, 6, n)
        c = self._coeffs(vals, indexed, e)                                     # (2, k, 6, n)
        hx, hy = np.einsum("an,kan->kn", phi, c[0]), np.einsum("an,kan->kn", phi, c[1])
        dxhy, dyhx = np.einsum("an,kan->kn", gx, c[1]), np.einsum("an,kan->kn", gy, c[0])
        ggx = -(np.einsum("an,kan->kn", H[0], c[0]) + np.einsum("an,kan->kn", H[1], c[1]))
        ggy = -(np.einsum("an,kan->kn", H[1], c[0]) + np.einsum("an,kan->kn", H[2], c[1]))
        b = np.asarray(beta, dtype=np.float64)[:, None]
        ex = w * (b * hy + ggy / b) / k0
        ey = -w * (b * hx + ggx / b) / k0
        out[0][:, ok], out[1][:, ok] = ex, ey
        out[2][:, ok] = -w * (dxhy - dyhx) / k0
        out[3][:, ok] = (ex * hy - ey * hx) / 2
        return out, eps, elem
