"""NumPy emulation of the posed flux overlap (plfem_flux_overlap_posed: k_flux_overlap_posed + k_overlap_reduce) for the
tests, built on ``power_emulation.PowerEmulation`` and the pose helpers of ``pose_overlap_emulation`` (imported, not edited).

Mesh B's quadrature points are taken into mesh A's frame with the kernel's arithmetic, located there by brute force; A's
values and its ``g = -(hx,xx + hy,xy), -(hx,xy + hy,yy)`` come from the located element's basis values and physical
Hessians and are turned by the pose's rotation; B's own values and g come from its own elements; the two permittivities are
evaluated on the host by ``indicator_emulation.eps_of`` (``IndexProfile.epsilon`` or the closed-disc test), A's at the point
in A's frame and B's at B's point:

    MA[i, j] = sum wA (hA'_i . hB_j)      GA[i, j] = sum wA (gA'_i . hB_j)
    MB[i, j] = sum wB (hA'_i . hB_j)      GB[i, j] = sum wB (hA'_i . gB_j)

with |det J| w_q of B, and 0 for a point in no element of A.  Also what the tests share: the materials on the two small
meshes of ``pose_overlap_emulation.small_meshes``, a geometry moved by a pose, and the closed forms of the quadratic
fields of ``power_cases``.
"""
from __future__ import annotations

import numpy as np

import power_cases
from indicator_emulation import eps_of
from oracle.p2 import p2_basis
from pl_fem_vectoriel_amd import IndexProfile, ProfiledGeometry
from pose_overlap_emulation import rotate, to_a_frame
from power_emulation import PowerEmulation

NAMES = ("MA", "GA", "MB", "GB")
OUTSIDE = (0.9, 0.3, float(np.cos(0.2)), float(np.sin(0.2)), 0.4)      # the posed A covers part of B only


def _g_of(H, c):
    """g (2, k, n) from the basis Hessians H (3, 6, n) and the element coefficients c (2, k, 6, n)."""
    return np.stack([-(np.einsum("an,kan->kn", H[0], c[0]) + np.einsum("an,kan->kn", H[1], c[1])),
                     -(np.einsum("an,kan->kn", H[1], c[0]) + np.einsum("an,kan->kn", H[2], c[1]))])


def posed_flux(em_a: PowerEmulation, vals_a, geometry_a, em_b: PowerEmulation, vals_b, geometry_b, indexed, pose):
    """({name: (ka, kb)}, element of A per quadrature point of B) under one pose; vals (2, k, nrows)."""
    qx = em_b.basis.qx.reshape(2, -1)
    w = em_b.basis.dx.reshape(-1)
    nq = qx.shape[1]
    xa = to_a_frame(qx, pose)
    elem, xi, eta, _ = em_a.locate(xa)
    ok = np.nonzero(elem >= 0)[0]
    ka = vals_a.shape[1]
    hA, gA = np.zeros((2, ka, nq)), np.zeros((2, ka, nq))
    wA, wB = np.zeros(nq), np.zeros(nq)
    if ok.size:
        e = elem[ok]
        phi, _ = p2_basis(xi[ok], eta[ok])                               # (6, n)
        c = em_a._coeffs(vals_a, indexed, e)                             # (2, ka, 6, n)
        hA[0][:, ok] = np.einsum("an,kan->kn", phi, c[0])
        hA[1][:, ok] = np.einsum("an,kan->kn", phi, c[1])
        gA[:, :, ok] = _g_of(em_a.basis_hess(e), c)
        wA[ok] = w[ok] / np.real(eps_of(geometry_a)(xa[0][ok], xa[1][ok]))
        wB[ok] = w[ok] / np.real(eps_of(geometry_b)(qx[0][ok], qx[1][ok]))
    hA, gA = rotate(hA, pose), rotate(gA, pose)
    hB = em_b.own_values(vals_b, indexed)                                # (2, kb, nq), element-major
    gB = np.repeat(_g_of(em_b.basis_hess(), em_b._coeffs(vals_b, indexed)), 6, axis=2)

    def s(X, Y, wt):
        return sum(X[c] @ (Y[c] * wt[None]).T for c in range(2))

    return {"MA": s(hA, hB, wA), "GA": s(gA, hB, wA), "MB": s(hA, hB, wB), "GB": s(hA, gB, wB)}, elem


# -- materials on the two small meshes (A on [-2, 2]^2, B on [-0.5, 0.5]^2) --------------------------------------------
def rim_disc_geometry(em_b: PowerEmulation, element=7, q=1, n_core=1.535, n_clad=1.0):
    """Three discs inside mesh B, the first with its rim exactly through quadrature point (element, q) of B: centre (X - r0,
    Y) with the radius taken back from the rounded centre, r = X - cx, so that (X - cx)^2 + 0 <= r^2 holds with equality
    in the kernel's arithmetic.  Returns (geometry, index of that point)."""
    qx = em_b.basis.qx
    X, Y = float(qx[0, element, q]), float(qx[1, element, q])
    cx = X - 0.17
    r = X - cx
    g = power_cases.discs([[cx, Y], [0.22, 0.1], [0.0, 0.3]], [r, 0.12, 0.1], n_core=n_core, n_clad=n_clad)
    assert (X - cx) ** 2 + (Y - Y) ** 2 == r * r
    return g, 6 * element + q


def centred_profile() -> IndexProfile:
    """A ring plus a graded layer around the origin over a background of 1.2: both inside mesh B."""
    return IndexProfile(1.2).ring((0.05, -0.1), 0.15, 0.3, 1.40).graded((-0.1, 0.1), 0.2, 1.535, 1.45, 2)


def wide_profile() -> IndexProfile:
    """Layers of mesh A's size: a graded core and a ring."""
    return IndexProfile(1.0).graded((0.1, -0.05), 0.6, 1.535, 1.2, 2).ring((0.0, 0.0), 0.9, 1.4, 1.3)


def profiled(profile, base) -> ProfiledGeometry:
    return ProfiledGeometry(base, profile, n_core=1.535, n_clad=1.2)


def uniform_geometry(eps=power_cases.KA_EPS):
    return power_cases.no_discs(np.sqrt(eps))


def moved_discs(geometry, pose):
    """The discs of ``geometry`` as they stand in B's frame: centres t + m R c, radii m r."""
    tx, ty, c, s, m = pose
    pos = np.atleast_2d(np.asarray(geometry.positions, dtype=np.float64)).reshape(-1, 2)
    moved = np.column_stack([tx + m * (c * pos[:, 0] - s * pos[:, 1]), ty + m * (s * pos[:, 0] + c * pos[:, 1])])
    return power_cases.discs(moved, m * np.asarray(geometry.core_radii, dtype=np.float64), n_core=geometry.n_core,
                             n_clad=geometry.n_clad)


# -- the known answer: the two quadratic fields of power_cases on both sides, uniform eps -------------------------------
def ka_closed_form(pose, eps=power_cases.KA_EPS, box=(-0.5, 0.5, -0.5, 0.5)):
    """{name: (2, 2)} over the box: A's field is evaluated at R^T (x - t) / m and turned, its g (constant) turned; the
    integrands have degree <= 4, so a 6 x 6 Gauss-Legendre rule integrates them exactly, independent of any mesh."""
    t, wt = np.polynomial.legendre.leggauss(6)
    x = 0.5 * (box[0] + box[1]) + 0.5 * (box[1] - box[0]) * t
    y = 0.5 * (box[2] + box[3]) + 0.5 * (box[3] - box[2]) * t
    X, Y = (v.ravel() for v in np.meshgrid(x, y))
    W = np.outer(wt, wt).ravel() * 0.25 * (box[1] - box[0]) * (box[3] - box[2]) / eps
    xa = to_a_frame(np.vstack([X, Y]), pose)
    hx, hy, _, _, gx, gy = power_cases.ka_fields(xa[0], xa[1])
    hA, gA = rotate(np.stack([hx, hy]), pose), rotate(np.stack([gx, gy]), pose)
    hx, hy, _, _, gx, gy = power_cases.ka_fields(X, Y)
    hB, gB = np.stack([hx, hy]), np.stack([gx, gy])

    def s(P, Q):
        return sum(P[c] @ (Q[c] * W[None]).T for c in range(2))

    M = s(hA, hB)
    return {"MA": M, "GA": s(gA, hB), "MB": M, "GB": s(hA, gB)}
