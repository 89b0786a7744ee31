"""NumPy emulation of the quartic overlap kernel (k_mode_quartic) for the tests, and an independent exact integration.

The emulation reuses the DOF numbering and interior map of ``fields_emulation.Emulation`` and the closed-disc core test of
``gram_emulation``, and evaluates the P2 basis at the 16-point degree-8 rule (the Python copy in
``pl_fem_vectoriel_amd.nonlinear``).  ``exact_quartic`` integrates without any quadrature: a P2 field is a homogeneous
quadratic in the barycentric coordinates, so a product of four is a homogeneous octic, and
``int_T l1^a l2^b l3^c = 2 |T| a! b! c! / (a + b + c + 2)!``.
"""
from __future__ import annotations

from math import factorial

import numpy as np

from gram_emulation import GramEmulation
from oracle.p2 import p2_basis
from pl_fem_vectoriel_amd.nonlinear import QUAD16_W, QUAD16_X

PHI16 = p2_basis(QUAD16_X[0], QUAD16_X[1])[0]                       # (6, 16)

# barycentric monomials of degree 2 (l1 = 1 - xi - eta, l2 = xi, l3 = eta) and the P2 basis in them:
# vertex a: l_a (2 l_a - 1) = l_a^2 - l_a l_b - l_a l_c; edge (a, b): 4 l_a l_b; edges (0,1), (1,2), (0,2)
MONO2 = ((2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 0), (0, 1, 1), (1, 0, 1))
BASIS2 = np.array([[1, 0, 0, -1, 0, -1],         # rows: the six P2 basis functions, columns: MONO2
                   [0, 1, 0, -1, -1, 0],
                   [0, 0, 1, 0, -1, -1],
                   [0, 0, 0, 4, 0, 0],
                   [0, 0, 0, 0, 4, 0],
                   [0, 0, 0, 0, 0, 4]], dtype=np.float64)


def _product_table(ea, eb):
    """Exponents of the products of two monomial lists: (list of distinct exponents, index (len(ea), len(eb)))."""
    out, idx = [], np.zeros((len(ea), len(eb)), dtype=np.int64)
    for i, a in enumerate(ea):
        for j, b in enumerate(eb):
            e = tuple(x + y for x, y in zip(a, b))
            if e not in out:
                out.append(e)
            idx[i, j] = out.index(e)
    return out, idx


MONO4, _IDX22 = _product_table(MONO2, MONO2)                       # 15 quartic monomials
_M8, _IDX44 = _product_table(MONO4, MONO4)
# C[m, n] = int over the reference-scaled triangle of MONO4[m] MONO4[n], per unit 2 |T|
C44 = np.array([[factorial(e[0]) * factorial(e[1]) * factorial(e[2]) / factorial(sum(e) + 2)
                 for e in (_M8[_IDX44[m, n]] for n in range(len(MONO4)))] for m in range(len(MONO4))])


class QuarticEmulation(GramEmulation):
    def values16(self, vals, indexed):
        """(ncomp, k, ne, 16): the modes at the 16-point rule of every element."""
        rows = self._rows(indexed)
        valid = rows >= 0
        r = np.where(valid, rows, 0)
        return np.stack([np.einsum("aq,kae->keq", PHI16, vals[c][:, r] * valid[None]) for c in range(vals.shape[0])])

    def weights16(self, geometry=None, weights=(1.0, 1.0)):
        """(ne, 16): |det J| w_q, times weights[0] / weights[1] in / out of the closed core discs when a geometry is given."""
        w = self.basis.absdet[:, None] * QUAD16_W[None, :]
        if geometry is None:
            return w
        p0 = self.mesh.p[:, self.mesh.t[0]]
        J = self.basis.J                                             # (2, 2, ne)
        qx = p0[:, :, None] + J[:, 0][:, :, None] * QUAD16_X[0][None, None] + J[:, 1][:, :, None] * QUAD16_X[1][None, None]
        inside = np.zeros(w.shape, dtype=bool)
        pos = np.atleast_2d(np.asarray(geometry.positions, dtype=np.float64))
        rad = np.asarray(geometry.core_radii, dtype=np.float64).reshape(-1)
        for (cx, cy), rr in zip(pos, rad):
            inside |= (qx[0] - cx) ** 2 + (qx[1] - cy) ** 2 <= rr * rr
        return w * np.where(inside, weights[0], weights[1])

    def quartic(self, vals, indexed, geometry=None, weights=(1.0, 1.0), chunk=4096):
        """The packed np x np output of plfem_mode_quartic, accumulated over chunks of elements."""
        k = vals.shape[1]
        I, J = np.triu_indices(k)                                    # row-major: the order p(i, j)
        U = self.values16(vals, indexed)
        W = self.weights16(geometry, weights)
        Q = np.zeros((I.size, I.size))
        for s in range(0, W.shape[0], chunk):
            u = U[:, :, s:s + chunk].reshape(U.shape[0], k, -1)     # (ncomp, k, npts)
            R = sum(u[c][I] * u[c][J] for c in range(u.shape[0])).T  # (npts, np)
            Q += R.T @ (R * W[s:s + chunk].reshape(-1)[:, None])
        return Q


def exact_quartic(em, vals, indexed, entries=None, chunk=512):
    """Exact integral of (u_i . u_j)(u_l . u_m) over the mesh (no quadrature), packed np x np, or the given
    ``entries`` (n, 2) of it."""
    k = vals.shape[1]
    I, J = np.triu_indices(k)
    rows = em._rows(indexed)
    valid = rows >= 0
    r = np.where(valid, rows, 0)
    det = em.basis.absdet                                            # 2 |T|
    coef = [np.einsum("am,kae->kem", BASIS2, vals[c][:, r] * valid[None]) for c in range(vals.shape[0])]   # (k, ne, 6)
    npair = I.size
    Q = np.zeros((npair, npair)) if entries is None else np.zeros(len(entries))
    ne = det.size
    for s in range(0, ne, chunk):
        R = np.zeros((npair, min(chunk, ne - s), len(MONO4)))
        for c in range(len(coef)):
            a, b = coef[c][I, s:s + chunk], coef[c][J, s:s + chunk]  # (np, ne_c, 6)
            for m in range(6):
                for n in range(6):
                    R[:, :, _IDX22[m, n]] += a[:, :, m] * b[:, :, n]
        Y = np.einsum("mn,Pen->Pem", C44, R) * det[None, s:s + chunk, None]
        if entries is None:
            Q += R.reshape(npair, -1) @ Y.reshape(npair, -1).T
        else:
            e = np.asarray(entries)
            for t in range(0, len(e), 1024):
                ee = e[t:t + 1024]
                Q[t:t + 1024] += np.einsum("nem,nem->n", R[ee[:, 0]], Y[ee[:, 1]])
    return Q


def square_mesh(n=16, jitter=0.2, seed=0):
    """A jittered n x n two-triangle-per-cell mesh of [-1, 1]^2: (p (2, nv), t (3, ne))."""
    rng = np.random.default_rng(seed)
    x = np.linspace(-1.0, 1.0, n + 1)
    X, Y = np.meshgrid(x, x, indexing="ij")
    h = 2.0 / n
    inner = (np.abs(X) < 1) & (np.abs(Y) < 1)
    X = X + inner * rng.uniform(-jitter, jitter, X.shape) * h
    Y = Y + inner * rng.uniform(-jitter, jitter, Y.shape) * h
    p = np.vstack([X.ravel(), Y.ravel()])
    v = np.arange((n + 1) ** 2).reshape(n + 1, n + 1)
    a, b, c, d = v[:-1, :-1].ravel(), v[1:, :-1].ravel(), v[:-1, 1:].ravel(), v[1:, 1:].ravel()
    t = np.hstack([np.vstack([a, b, d]), np.vstack([a, d, c])])
    return p, t
