"""What the electric-field and power tests share: small geometries on the unit square, synthetic vectorial records, and the
known-answer quadratic field whose E, Sz and power Grams have closed forms."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from pl_fem_vectoriel_amd import IndexProfile, MCFGeometry, ProfiledGeometry

KA_EPS = 2.25              # uniform permittivity of the known-answer case
KA_BETA = (7.0, 5.5)
KA_K0 = 2.0 * np.pi / 1.55


def discs(positions, radii, n_core=1.535, n_clad=1.45):
    """A geometry of the package with the given core discs (no PML: only the real permittivity is read)."""
    g = MCFGeometry(7, 8.0, 1.5, n_core, n_clad, wavelength_um=1.55, use_complex_pml=False)
    g.positions = g.core_positions = np.asarray(positions, dtype=np.float64).reshape(-1, 2)
    g.core_radii = np.asarray(radii, dtype=np.float64).reshape(-1)
    g.n_cores = len(g.core_radii)
    return g


def rim_discs():
    """One disc at (0.5, 0.5) of radius 0.25 -- (0.75, 0.5) is exactly on its rim: 0.25^2 + 0 <= 0.25^2 with every term
    exact -- and a second one overlapping it."""
    return discs([[0.5, 0.5], [0.62, 0.41]], [0.25, 0.2])


def no_discs(n=1.5):
    """Uniform n, no cores: everything is "rest"."""
    g = discs(np.zeros((0, 2)), np.zeros(0))
    g.n_core = g.n_clad = float(n)         # (the constructor refuses equal indices)
    return g


def ring_profile() -> IndexProfile:
    """A ring plus a graded layer over a background of 1.2."""
    return IndexProfile(1.2).ring((0.5, 0.5), 0.22, 0.37, 1.40).graded((0.4, 0.55), 0.2, 1.535, 1.45, 2)


def map_profile() -> IndexProfile:
    """The same layers over an 8 x 5 sampled map that covers part of the square."""
    x, y = np.linspace(0.05, 0.9, 8), np.linspace(-0.1, 0.8, 5)
    n = 1.25 + 0.2 * np.random.default_rng(11).uniform(size=(5, 8))
    return IndexProfile(1.2).sampled(x, y, n).ring((0.5, 0.5), 0.22, 0.37, 1.40).graded((0.4, 0.55), 0.2, 1.535, 1.45, 2)


def profiled(profile) -> ProfiledGeometry:
    """``profile`` on the discs of :func:`rim_discs`, which stay the region split."""
    return ProfiledGeometry(rim_discs(), profile, n_core=1.535, n_clad=1.2)


def records(rng, nrows, k):
    return [{"Ex_dofs": rng.standard_normal(nrows), "Ey_dofs": rng.standard_normal(nrows), "beta": float(rng.uniform(5, 10))}
            for _ in range(k)]


def vals_of(modes):
    return np.stack([np.array([m["Ex_dofs"] for m in modes]), np.array([m["Ey_dofs"] for m in modes])])


def betas_of(modes):
    return np.array([m["beta"] for m in modes])


# -- the known answer: two quadratic fields, exactly representable in P2 ------------------------------------------------
def ka_fields(x, y):
    """(k = 2) of hx, hy, dx hy, dy hx, gx, gy at the points: mode 0 is hx = x^2 + 2 x y, hy = y^2 - x y + x, so
    g = (-1, -4); mode 1 is hx = y^2 - x, hy = 2 x^2 + x y - y + 1.5 y^2, so g = -(0 + 1, 0 + 3) = (-1, -3)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    one = np.ones_like(x)
    hx = np.stack([x * x + 2 * x * y, y * y - x])
    hy = np.stack([y * y - x * y + x, 2 * x * x + x * y - y + 1.5 * y * y])
    dxhy = np.stack([-y + 1, 4 * x + y])
    dyhx = np.stack([2 * x, 2 * y])
    gx = np.stack([-one, -one])
    gy = np.stack([-4 * one, -3 * one])
    return hx, hy, dxhy, dyhx, gx, gy


def ka_closed_forms(x, y, beta=KA_BETA, k0=KA_K0, eps=KA_EPS):
    """(4, 2, npts): Ex, Ey, Ez_im, Sz of the two fields from the definitions."""
    hx, hy, dxhy, dyhx, gx, gy = ka_fields(x, y)
    b = np.asarray(beta)[:, None]
    w = 1.0 / eps
    ex = w * (b * hy + gy / b) / k0
    ey = -w * (b * hx + gx / b) / k0
    return np.stack([ex, ey, -w * (dxhy - dyhx) / k0, (ex * hy - ey * hx) / 2])


def ka_grams(eps=KA_EPS):
    """M_w, G_w (2, 2) over the unit square: the integrands are polynomials of degree <= 4, so a 4 x 4 Gauss-Legendre
    rule integrates them exactly -- independent of any mesh."""
    t, wt = np.polynomial.legendre.leggauss(4)
    t, wt = 0.5 * (t + 1.0), 0.5 * wt
    X, Y = np.meshgrid(t, t)
    W = (wt[:, None] * wt[None, :]).reshape(-1) / eps
    hx, hy, _, _, gx, gy = ka_fields(X.reshape(-1), Y.reshape(-1))
    return (hx * W) @ hx.T + (hy * W) @ hy.T, (gx * W) @ hx.T + (gy * W) @ hy.T


def ka_all_dof_vectors(doflocs):
    """The two fields as all-DOF P2 vectors (2 components, k = 2, N): nodal interpolation is exact for quadratics."""
    hx, hy, *_ = ka_fields(doflocs[0], doflocs[1])
    return np.stack([hx, hy])


def ka_geometry():
    g = no_discs(np.sqrt(KA_EPS))
    return SimpleNamespace(positions=g.positions, core_radii=g.core_radii, n_core=g.n_core, n_clad=g.n_clad, k0=KA_K0)
