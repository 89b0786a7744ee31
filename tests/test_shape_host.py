"""Shape sensitivities on the host: the NumPy emulation of the velocity Gram kernel against central differences of the
oracle's element matrices on the moved mesh, the convected-material condition those differences rest on, the k x k host
math against central differences of the oracle's eigenvalues, the velocity fields of core_velocities and the disorder
statistics."""
import numpy as np
import pytest
from scipy.sparse.linalg import eigsh

from oracle import hfield, scalar
from oracle.p2 import MeshTriLite, P2Basis
from pl_fem_vectoriel_amd import (PhotonicLanternGeometry, core_velocities, disorder_statistics, generate_mesh,
                                  shape_response_from_grams)
from profile_cases import POS, RAD, own_discs, three_core
from velocity_gram_emulation import VelocityGramEmulation


def moved_geometry(core, kind, t):
    """three_core's geometry with ``core`` displaced by t along x or y, or its radius changed by t."""
    pos, rad = POS.copy(), RAD.copy()
    if kind == "dx":
        pos[core, 0] += t
    elif kind == "dy":
        pos[core, 1] += t
    else:
        assert kind == "dr"
        rad[core] += t
    return PhotonicLanternGeometry(3, "triangular_3", pos, rad, 1.535, 1.0, wavelength=1.55)


class Convected:
    """The material of ``geometry`` at the quadrature points of the unmoved mesh, carried to whatever points are asked
    for (same shape): the moved section of a velocity that no disc geometry can express (an ellipse)."""

    def __init__(self, geometry, basis):
        self.k0 = geometry.k0
        self._eps = np.real(geometry.epsilon(*basis.qx))

    def epsilon(self, x, y):
        assert np.shape(x) == self._eps.shape
        return self._eps


@pytest.fixture(scope="module")
def three():
    g, mesh = three_core()
    em = VelocityGramEmulation(mesh.p, mesh.t)
    V, labels = core_velocities(mesh, g, kinds=("dx", "dy", "dr", "e2c"))
    return g, mesh, em, V, labels


def moved_basis(em, V, t):
    return P2Basis(MeshTriLite(em.mesh.p + t * V.T, em.mesh.t))


def smooth_fields(em, k, seed):
    """(k, N): low-order trigonometric fields at the P2 nodes of the unmoved mesh, under a C^2 envelope that is exactly 0
    from r = 15 on.  The mesh has three sliver elements at the corners of the domain (|det J| 1e-9 of the edge products):
    a field that reaches them projects to forms of size 1e6, and the rounding of those sums, not the derivative, is
    then what a difference of two forms shows."""
    rng = np.random.default_rng(seed)
    x, y = em.basis.doflocs
    a = rng.uniform(0.05, 0.4, (k, 2))
    ph = rng.uniform(0, 2 * np.pi, (k, 2))
    env = np.clip(1.0 - (x * x + y * y) / 15.0 ** 2, 0.0, None) ** 3
    return np.cos(a[:, :1] * x[None] + ph[:, :1]) * np.cos(a[:, 1:] * y[None] + ph[:, 1:]) * env[None]


def project(E, ed, U, W=None):
    """U^T E W of element matrices E (ne, 6, 6) on nodal vectors U, W (k, N)."""
    W = U if W is None else W
    return np.einsum("mie,eij,nje->mn", U[:, ed], E, W[:, ed], optimize=True)


def projected_forms(ncomp, geometry, basis, vals):
    """The forms of ModeFields.velocity_grams' outputs (before the derivative) from the oracle's element matrices."""
    ed = basis.element_dofs
    if ncomp == 1:
        E = scalar.element_matrices(geometry, basis)
        return np.stack([project(E[nm], ed, vals[0]) for nm in ("stiff", "mass", "eps_m")])
    E = hfield.element_matrices(geometry, basis)
    hx, hy = vals
    Kw = (project(E["kxx"], ed, hx) + project(E["kyy"], ed, hy) + project(E["kxy"], ed, hx, hy) + project(E["kyx"], ed, hy, hx))
    D = (project(E["div_xx"], ed, hx) + project(E["div_yy"], ed, hy) + project(E["div_xy"], ed, hx, hy) +
         project(E["div_xy"].transpose(0, 2, 1), ed, hy, hx))
    M = project(E["mass"], ed, hx) + project(E["mass"], ed, hy)
    Mw = project(E["mass_eps_inv"], ed, hx) + project(E["mass_eps_inv"], ed, hy)
    return np.stack([Kw, D, M, Mw])


# ---- (a) the emulation is the derivative of the oracle's element matrices on the moved mesh ---------------------------
@pytest.mark.parametrize("ncomp", [2, 1])
def test_emulation_against_central_differences_of_the_oracles_element_matrices(three, ncomp):
    g, mesh, em, V, labels = three
    t = 1e-4
    vals = np.stack([smooth_fields(em, 4, 5 + c) for c in range(ncomp)])
    for kind in ("dx", "dr", "e2c"):
        v = V[labels.index((0, kind))]
        out, count = em.velocity_grams(vals, False, g, v[None])
        assert 0 < count[0] < mesh.t.shape[1]
        fd = []
        for s in (+t, -t):
            basis = moved_basis(em, v, s)
            geo = Convected(g, em.basis) if kind == "e2c" else moved_geometry(0, kind, s)
            if kind != "e2c":                                            # the moved discs hold the points they held
                assert np.array_equal(np.real(geo.epsilon(*basis.qx)), np.real(g.epsilon(*em.basis.qx)))
            fd.append(projected_forms(ncomp, geo, basis, vals))
        d = (fd[0] - fd[1]) / (2 * t)
        for o in range(d.shape[0]):
            err = np.abs(out[0, o] - d[o]).max() / np.abs(d[o]).max()
            print(f"ncomp {ncomp} {kind} output {o}: |emulation - central difference| max {err:.1e} of max |d|")
            assert err <= 1e-6


# ---- (b) the condition under which a finite difference of re-solved sections is the convected derivative -------------
def test_every_quadrature_point_keeps_its_material_under_the_nine_core_motions(three):
    g, mesh, em, V, labels = three
    eps0 = np.real(g.epsilon(*em.basis.qx))
    for core in range(3):
        for kind in ("dx", "dy", "dr"):
            v = V[labels.index((core, kind))]
            for s in (2.5e-4, -2.5e-4):
                basis = moved_basis(em, v, s)
                assert np.array_equal(np.real(moved_geometry(core, kind, s).epsilon(*basis.qx)), eps0), (core, kind, s)


# ---- (c) the host math against central differences of the oracle's eigenvalues --------------------------------------
def oracle_scalar_eigs(geometry, mesh_lite, k=10):
    K, M, Me, basis = scalar.assemble(geometry, mesh_lite)
    A = (K - geometry.k0 ** 2 * Me).tocsr()
    lam, U = eigsh(A, k=k, M=M, sigma=scalar.shift(geometry), which="LM", tol=1e-13, maxiter=6000)
    order = np.argsort(lam)
    return lam[order], U[:, order].T


def test_shape_response_from_grams_against_central_differences_of_oracle_eigenvalues(three):
    g, mesh, em, V, labels = three
    t, k0 = 2.5e-4, g.k0
    lam, U = oracle_scalar_eigs(g, em.mesh)
    assert np.all(lam < 0)
    beta = np.sqrt(-lam)
    vals = U[None]
    cases = [(c, kd) for c in range(3) for kd in ("dx", "dy", "dr")]
    vel = np.stack([V[labels.index(cs)] for cs in cases])
    out, _ = em.velocity_grams(vals, False, g, vel)
    grams = em.profile_grams(vals, False, own_discs(g).index_profile)
    res = shape_response_from_grams("scalar", grams, em.named(out), beta, k0)
    assert res["dneff_dp"].shape == (10, 9) and res["rayleigh_defect"].max() <= 1e-9
    dlam = -2.0 * beta[:, None] * k0 * res["dneff_dp"]                  # lambda = -beta^2
    for i, (core, kind) in enumerate(cases):
        pm = [oracle_scalar_eigs(moved_geometry(core, kind, s), MeshTriLite(em.mesh.p + s * vel[i].T, em.mesh.t))[0]
              for s in (+t, -t)]
        fd = (pm[0] - pm[1]) / (2 * t)
        err = np.abs(dlam[:, i] - fd).max() / np.abs(fd).max()
        print(f"core {core} {kind}: |d lambda - central difference| max {err:.1e} of max |d lambda| {np.abs(fd).max():.3g}")
        assert err <= 1e-5


# ---- (d) the velocity fields -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("inner", [1.25, 1.5])
def test_core_velocities_are_rigid_or_linear_on_every_element_that_touches_the_disc(inner):
    g, mesh = three_core()
    V, labels = core_velocities(mesh, g, inner=inner)
    assert V.shape == (15, mesh.p.shape[1], 2) and V.flags.c_contiguous
    assert labels == [(c, kd) for c in range(3) for kd in ("dx", "dy", "dr", "e2c", "e2s")]
    x, y = mesh.p
    for c in range(3):
        (cx, cy), r = POS[c], RAD[c]
        X, Y = x - cx, y - cy
        eta = V[labels.index((c, "dx"))][:, 0]
        assert np.array_equal(eta, V[labels.index((c, "dy"))][:, 1]) and eta.min() == 0.0 and eta.max() == 1.0
        touching = (X[mesh.t] ** 2 + Y[mesh.t] ** 2 <= r * r).any(0)
        assert touching.sum() > 50 and np.all(eta[mesh.t[:, touching]] == 1.0)
        inside = np.hypot(X, Y) <= inner * r                            # exactly linear there
        assert np.all(eta[inside] == 1.0)
        for kind, (fx, fy) in {"dr": (X / r, Y / r), "e2c": (X / r, -(Y / r)), "e2s": (Y / r, X / r)}.items():
            v = V[labels.index((c, kind))]
            assert np.array_equal(v[inside, 0], fx[inside]) and np.array_equal(v[inside, 1], fy[inside])
        # nothing moves on another core or on the boundary
        for o in range(3):
            if o != c:
                other = (x - POS[o][0]) ** 2 + (y - POS[o][1]) ** 2 <= RAD[o] ** 2
                assert not V[5 * c:5 * c + 5][:, other].any()
    sub, lab = core_velocities(mesh, g, kinds=("dr",), inner=inner, cores=[2])
    assert lab == [(2, "dr")] and np.array_equal(sub[0], V[labels.index((2, "dr"))])


def test_core_velocities_refuse_what_the_collar_cannot_hold():
    g, mesh = three_core()
    with pytest.raises(ValueError, match="too coarse"):
        core_velocities(mesh, g, inner=1.0 + 1e-9)
    touching = PhotonicLanternGeometry(3, "triangular_3", np.array([[0.0, 0.0], [2.6, 0.0], [-2.5, 4.33]]), RAD, 1.535, 1.0,
                                       wavelength=1.55)
    with pytest.raises(ValueError, match="collar does not fit"):
        core_velocities(generate_mesh(touching, 0.5, 0), touching)
    for bad in (dict(kinds=()), dict(kinds=("dz",)), dict(inner=1.0), dict(inner=np.nan), dict(cores=[3]), dict(cores=[])):
        with pytest.raises(ValueError):
            core_velocities(mesh, g, **bad)


# ---- (e) disorder statistics -----------------------------------------------------------------------------------------
def test_disorder_statistics_against_the_direct_formula():
    rng = np.random.default_rng(8)
    gx, gy, gr = rng.standard_normal((3, 5, 3))
    resp = {"dneff_dx": gx, "dneff_dy": gy, "dneff_dr": gr}
    sp, sr = 0.05, np.array([0.01, 0.0, 0.02])
    st = disorder_statistics(resp, sp, sr)
    var = np.zeros(5)
    dvar = np.zeros((5, 5))
    for c in range(3):
        var += sp ** 2 * (gx[:, c] ** 2 + gy[:, c] ** 2) + sr[c] ** 2 * gr[:, c] ** 2
        for m in range(5):
            for n in range(5):
                dvar[m, n] += (sp ** 2 * ((gx[m, c] - gx[n, c]) ** 2 + (gy[m, c] - gy[n, c]) ** 2) +
                               sr[c] ** 2 * (gr[m, c] - gr[n, c]) ** 2)
    assert np.allclose(st["neff_std"], np.sqrt(var), rtol=1e-14, atol=0)
    assert np.allclose(st["dneff_std"], np.sqrt(dvar), rtol=1e-13, atol=1e-16)
    assert np.array_equal(st["dneff_std"], st["dneff_std"].T) and not np.diag(st["dneff_std"]).any()
    only = disorder_statistics({"dneff_dx": gx, "dneff_dy": gy}, sp)
    assert np.allclose(only["neff_std"], sp * np.sqrt((gx ** 2 + gy ** 2).sum(1)), rtol=1e-14, atol=0)
    for bad in (lambda: disorder_statistics({"dneff_dx": gx}, sp), lambda: disorder_statistics(resp, -1.0),
                lambda: disorder_statistics(resp, [0.1, 0.2]), lambda: disorder_statistics({"dneff_dx": gx, "dneff_dy": gy}, sp, 0.1)):
        with pytest.raises(ValueError):
            bad()
