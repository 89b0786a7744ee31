"""NumPy emulation of the mode-field kernels (k_sample_fields, k_field_overlap) for the tests.

Independent of the library: the P2 numbering, the affine maps and the quadrature come from ``oracle.p2`` (``P2Basis``,
``p2_basis``), and point location is brute force -- every element is tested against every point of its x-slab, with the
kernel's containment rule (every barycentric coordinate >= -(TOL + its rounding bound)) and tie rule (the smallest element id wins).
"""
from __future__ import annotations

import numpy as np

from oracle.p2 import P2Basis, MeshTriLite, PHI_Q, p2_basis

TOL = 1e-10          # PLFEM_LOC_TOL
EPS4 = 4 * np.finfo(np.float64).eps   # PLFEM_LOC_EPS4: the rounding bound of a coordinate (see dev_locate)
LOOSE = 1e-8         # a point within LOOSE of two elements may go to either under rounding differences


class Emulation:
    def __init__(self, p, t):
        self.mesh = MeshTriLite(p, t)
        self.basis = P2Basis(self.mesh)
        self.N = self.basis.N
        bnd = self.basis.get_dofs().all()
        mask = np.zeros(self.N, dtype=bool)
        mask[bnd] = True
        self.interior = np.nonzero(~mask)[0]
        self.int_index = np.full(self.N, -1, dtype=np.int64)
        self.int_index[self.interior] = np.arange(self.interior.size)

    def locate(self, pts):
        """(element, xi, eta, near): near = number of elements within LOOSE of the point."""
        p, t = self.mesh.p, self.mesh.t
        x, y = np.asarray(pts[0], dtype=np.float64), np.asarray(pts[1], dtype=np.float64)
        n = x.size
        order = np.argsort(x, kind="stable")
        xs = x[order]
        elem = np.full(n, -1, dtype=np.int64)
        xi = np.zeros(n)
        eta = np.zeros(n)
        near = np.zeros(n, dtype=np.int64)
        px, py = p[0], p[1]
        for e in range(t.shape[1]):
            v0, v1, v2 = t[0, e], t[1, e], t[2, e]
            vx, vy = px[[v0, v1, v2]], py[[v0, v1, v2]]
            mx = 1e-6 * (vx.max() - vx.min() + vy.max() - vy.min()) + 1e-300
            lo = np.searchsorted(xs, vx.min() - mx, "left")
            hi = np.searchsorted(xs, vx.max() + mx, "right")
            if lo == hi:
                continue
            idx = order[lo:hi]
            idx = idx[(y[idx] >= vy.min() - mx) & (y[idx] <= vy.max() + mx)]
            if idx.size == 0:
                continue
            ax, ay = px[v0], py[v0]
            j00, j10, j01, j11 = px[v1] - ax, py[v1] - ay, px[v2] - ax, py[v2] - ay
            det = j00 * j11 - j01 * j10
            dx, dy = x[idx] - ax, y[idx] - ay
            a = (j11 * dx - j01 * dy) / det
            b = (j00 * dy - j10 * dx) / det
            mx, my = np.abs(x[idx]) + abs(ax), np.abs(y[idx]) + abs(ay)
            sa = EPS4 * (abs(j11) * mx + abs(j01) * my) / abs(det)
            sb = EPS4 * (abs(j00) * my + abs(j10) * mx) / abs(det)
            c = 1.0 - a - b
            inside = (a >= -(TOL + sa)) & (b >= -(TOL + sb)) & (c >= -(TOL + sa + sb))
            mn = np.minimum(np.minimum(a, b), c)
            near[idx[(mn >= -LOOSE) | inside]] += 1
            hit = inside & (elem[idx] < 0)
            # coordinates within their rounding bound of an edge are put on it (the kernel's rule)
            za, zb = np.abs(a) <= sa, np.abs(b) <= sb
            a = np.where(za, 0.0, a)
            b = np.where(zb, 0.0, b)
            zc = np.abs(c) <= sa + sb
            a_new = np.where(zb, 1.0, np.where(za, a, np.where(sa >= sb, 1.0 - b, a)))
            b_new = np.where(zb, b, np.where(za, 1.0, np.where(sa >= sb, b, 1.0 - a)))
            a = np.where(zc, a_new, a)
            b = np.where(zc, b_new, b)
            elem[idx[hit]] = e
            xi[idx[hit]] = a[hit]
            eta[idx[hit]] = b[hit]
        return elem, xi, eta, near

    def _rows(self, indexed):
        dofs = self.basis.element_dofs                       # (6, ne)
        return self.int_index[dofs] if indexed else dofs

    def sample(self, vals, pts, indexed, beta=None, located=None):
        """vals (ncomp, k, nrows) -> out (nout, k, npts), element."""
        elem, xi, eta, near = self.locate(pts) if located is None else located
        ncomp, k, _ = vals.shape
        npts = elem.size
        nout = ncomp + (1 if (ncomp == 2 and beta is not None) else 0)
        out = np.zeros((nout, k, npts))
        ok = np.nonzero(elem >= 0)[0]
        if ok.size == 0:
            return out, elem
        e = elem[ok]
        phi, dphi = p2_basis(xi[ok], eta[ok])                # (6, n), (6, 2, n)
        rows = self._rows(indexed)[:, e]                     # (6, n)
        valid = rows >= 0
        r = np.where(valid, rows, 0)
        for c in range(ncomp):
            g = vals[c][:, r] * valid[None]                  # (k, 6, n)
            out[c][:, ok] = np.einsum("an,kan->kn", phi, g)
        if nout == 3:
            inv = self.basis.invJ[:, :, e]                   # (2, 2, n): inv[r, c] = d xi_r / d x_c
            gx = dphi[:, 0] * inv[0, 0] + dphi[:, 1] * inv[1, 0]
            gy = dphi[:, 0] * inv[0, 1] + dphi[:, 1] * inv[1, 1]
            g0 = vals[0][:, r] * valid[None]
            g1 = vals[1][:, r] * valid[None]
            div = np.einsum("an,kan->kn", gx, g0) + np.einsum("an,kan->kn", gy, g1)
            out[2][:, ok] = -div / np.asarray(beta)[:, None]
        return out, elem

    def quadrature(self, weight=None):
        """Quadrature points (2, 6 ne), weights (6 ne) of this mesh (element-major), wt = 1 or 1/eps(x)."""
        qx = self.basis.qx.reshape(2, -1)
        w = self.basis.dx.reshape(-1).copy()
        if weight is not None:
            pos = np.atleast_2d(np.asarray(weight.positions, dtype=np.float64))
            rad = np.asarray(weight.core_radii, dtype=np.float64).reshape(-1)
            inside = np.zeros(qx.shape[1], dtype=bool)
            for (cx, cy), r in zip(pos, rad):
                inside |= (qx[0] - cx) ** 2 + (qx[1] - cy) ** 2 <= r * r
            w *= np.where(inside, 1.0 / weight.n_core ** 2, 1.0 / weight.n_clad ** 2)
        return qx, w

    def own_values(self, vals, indexed):
        """Values of this mesh's modes at its own quadrature points, (ncomp, k, 6 ne)."""
        rows = self._rows(indexed)                           # (6, ne)
        valid = rows >= 0
        r = np.where(valid, rows, 0)
        out = []
        for c in range(vals.shape[0]):
            g = vals[c][:, r] * valid[None]                  # (k, 6, ne)
            out.append(np.einsum("aq,kae->keq", PHI_Q, g).reshape(vals.shape[1], -1))
        return np.stack(out)


def overlap(em_a, vals_a, em_b, vals_b, indexed, weight=None, located=None):
    """O[i, j] over mesh B's quadrature, A located brute force (the emulation of k_field_overlap); ``located``: the
    result of em_a.locate on B's quadrature points, when the caller reuses it."""
    qx, w = em_b.quadrature(weight)
    ua, _ = em_a.sample(vals_a, qx, indexed, located=located)
    ub = em_b.own_values(vals_b, indexed)
    return sum(ua[c] @ (ub[c] * w[None]).T for c in range(vals_a.shape[0]))
