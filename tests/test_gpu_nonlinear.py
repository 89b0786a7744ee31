"""Quartic overlap tensor on the GPU (k_mode_quartic + k_quartic_reduce): solver output at C1 L = 0 against the NumPy
emulation (tests/quartic_emulation.py), unweighted and core-weighted; random P2 fields at k = 1 .. 64 against exact
barycentric integration (the device copy of the 16-point rule, and pairs on both sides of a 64-pair tile and of a
32-mode chunk); bit-identical repeats, exact symmetry, mode permutation, untouched records; and A_eff / MFD of the LP01
mode of a step-index fibre against the Bessel-function values."""
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import integrate, optimize, special

from quartic_emulation import QuarticEmulation, exact_quartic, square_mesh
from pl_fem_vectoriel_amd import MCFGeometry, ModeFields, generate_mesh, mode_nonlinearity
from pl_fem_vectoriel_amd.nonlinear import pair_index
from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver

pytestmark = pytest.mark.gpu

# the bound of every comparison with the emulation or the exact integral below, as a share of max |Q| (also imported by
# tests/test_gpu_field_instances.py)
QUARTIC_TOL = 1e-12


@pytest.fixture(scope="module")
def c1(c1_geometry, gpu_device, built_library):
    mesh = generate_mesh(c1_geometry, 1.0, 0)
    vsol = TrueVectorialMaxwellSolver(c1_geometry, device=gpu_device, eig_tol=1e-10)
    ssol = ScalarHelmholtzSolver(c1_geometry, device=gpu_device)
    vec = vsol.solve_vectorial_modes(mesh, 20)
    scal = ssol.solve(mesh, 10)
    mf = ModeFields(mesh, device=gpu_device, solver=vsol)
    yield {"mesh": mesh, "vec": vec, "scal": scal, "mf": mf, "em": QuarticEmulation(mesh.p, mesh.t)}
    mf.close()
    vsol.clear_cache()
    ssol.clear_cache()
    import torch
    torch.cuda.empty_cache()


def _vals(modes):
    if "Ex_dofs" in modes[0]:
        return np.stack([np.array([m["Ex_dofs"] for m in modes]), np.array([m["Ey_dofs"] for m in modes])])
    return np.array([m["field_vector"] for m in modes])[None]


def test_kernel_matches_emulation_on_solver_modes(c1, c1_geometry):
    mf, em, g = c1["mf"], c1["em"], c1_geometry
    for modes, indexed in ((c1["vec"], True), (c1["scal"], False)):
        vals = _vals(modes)
        for geom, w in ((None, (1.0, 1.0)), (g, (2.5, 0.25))):
            Q = mf.quartic(modes, geom, w)
            ref = em.quartic(vals, indexed, geom, w)
            err = np.abs(Q - ref).max() / np.abs(ref).max()
            print(f"{'vectorial' if indexed else 'scalar'} k = {len(modes)} weights {geom is not None}: {err:.2e} of max |Q|")
            assert err <= 1e-12
            assert np.array_equal(Q, Q.T)
            assert np.array_equal(Q, mf.quartic(modes, geom, w))            # bit-identical repeat


def test_permuting_modes_permutes_the_tensor_and_records_are_untouched(c1, c1_geometry):
    modes = c1["scal"]
    before = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in m.items()} for m in modes]
    res = mode_nonlinearity(modes, c1["mf"], c1_geometry, n2=(2.6e-20, 0.0))
    for a, b in zip(modes, before):
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(a[k], b[k]) if isinstance(b[k], np.ndarray) else a[k] == b[k]
    perm = np.random.default_rng(3).permutation(len(modes))
    other = mode_nonlinearity([modes[i] for i in perm], c1["mf"], c1_geometry, n2=(2.6e-20, 0.0))
    Q = res["Q"]
    want = Q[np.ix_(perm, perm, perm, perm)]
    assert np.abs(other["Q"] - want).max() <= 1e-13 * np.abs(Q).max()
    assert np.allclose(other["a_eff"], res["a_eff"][perm], rtol=1e-13)
    assert np.all(res["gamma_self"] > 0) and np.all(res["a_eff"] > 0) and np.all(res["mfd_petermann"] > 0)
    vres = mode_nonlinearity(c1["vec"], c1["mf"])
    assert np.all(np.isfinite(vres["a_eff"])) and np.all(vres["a_eff"] > 0)


@pytest.fixture(scope="module")
def square(gpu_device, built_library):
    p, t = square_mesh(16, seed=2)
    mf = ModeFields(SimpleNamespace(p=p, t=t), device=gpu_device)
    yield mf, QuarticEmulation(p, t)
    mf.close()


@pytest.mark.parametrize("k,ncomp", [(1, 1), (22, 2), (33, 1), (40, 2), (64, 1), (64, 2)])
def test_random_fields_against_exact_integration(square, k, ncomp):
    mf, em = square
    rng = np.random.default_rng(k + 100 * ncomp)
    indexed = ncomp == 2
    vals = rng.standard_normal((ncomp, k, em.interior.size if indexed else em.N))
    recs = ([{"Ex_dofs": vals[0, i], "Ey_dofs": vals[1, i]} for i in range(k)] if indexed
            else [{"field_vector": vals[0, i]} for i in range(k)])
    Q = mf.quartic(recs)
    npair = k * (k + 1) // 2
    assert Q.shape == (npair, npair) and np.array_equal(Q, Q.T)
    if k <= 40:
        E = exact_quartic(em, vals, indexed)
        err = np.abs(Q - E).max() / np.abs(E).max()
    else:
        ent = np.concatenate([np.stack([np.arange(npair)] * 2, 1), rng.integers(0, npair, (4096, 2))])
        E = exact_quartic(em, vals, indexed, entries=ent)
        err = np.abs(Q[ent[:, 0], ent[:, 1]] - E).max() / np.abs(E).max()
    print(f"k = {k}, ncomp = {ncomp}: {err:.2e} of max |Q|")
    assert err <= 1e-12
    P = pair_index(k)
    i, j = k - 1, max(0, k - 2)
    assert Q[P[i, j], P[i, j]] > 0                                         # a square of a real product


def _lp01(g):
    """n_eff, A_eff and Petermann II MFD of the LP01 mode of a step-index fibre (J0 / K0 field)."""
    a = float(g.r_core)
    V = g.k0 * a * np.sqrt(g.n_core ** 2 - g.n_clad ** 2)
    U = optimize.brentq(lambda u: u * special.j1(u) / special.j0(u)
                        - np.sqrt(V * V - u * u) * special.k1(np.sqrt(V * V - u * u)) / special.k0(np.sqrt(V * V - u * u)),
                        1e-6, min(V, 2.404825557695773) - 1e-9, xtol=1e-15)
    W = np.sqrt(V * V - U * U)
    c = special.j0(U) / special.k0(W)

    def integral(fin, fout):
        opts = dict(epsabs=0, epsrel=1e-13, limit=200)
        return 2 * np.pi * (integrate.quad(lambda r: fin(r) * r, 0, a, **opts)[0]
                            + integrate.quad(lambda r: fout(r) * r, a, np.inf, **opts)[0])

    N = integral(lambda r: special.j0(U * r / a) ** 2, lambda r: (c * special.k0(W * r / a)) ** 2)
    P4 = integral(lambda r: special.j0(U * r / a) ** 4, lambda r: (c * special.k0(W * r / a)) ** 4)
    G = integral(lambda r: (U / a * special.j1(U * r / a)) ** 2, lambda r: (W / a * c * special.k1(W * r / a)) ** 2)
    n_eff = np.sqrt(g.n_core ** 2 - (U / (g.k0 * a)) ** 2)
    return n_eff, N * N / P4, 2 * np.sqrt(2 * N / G)


def test_step_index_lp01_effective_area_and_mfd(gpu_device, built_library):
    g = MCFGeometry(1, 8.0, 2.5, 1.46, 1.444, wavelength_um=1.55)              # V ~ 2.18, single-mode
    n_eff, a_eff, mfd = _lp01(g)
    mesh = generate_mesh(g, 1.0, 1)
    sol = ScalarHelmholtzSolver(g, device=gpu_device)
    try:
        modes = sol.solve(mesh, 4)
        hit = [m for m in modes if abs(m["n_eff"] - n_eff) <= 2e-5]
        assert len(hit) == 1, ([m["n_eff"] for m in modes], n_eff)
        res = mode_nonlinearity(hit, mesh, g, n2=(2.6e-20, 0.0), device=gpu_device)
    finally:
        sol.clear_cache()
    print(f"LP01: n_eff {hit[0]['n_eff']:.9f} (analytic {n_eff:.9f}); A_eff {res['a_eff'][0]:.6f} um^2 "
          f"(analytic {a_eff:.6f}); MFD {res['mfd_petermann'][0]:.6f} um (analytic {mfd:.6f}); "
          f"gamma {res['gamma_self'][0]:.4f} /W/km")
    assert abs(res["a_eff"][0] / a_eff - 1) <= 2e-3
    assert abs(res["mfd_petermann"][0] / mfd - 1) <= 2e-3
    assert 0 < res["gamma_self"][0] < 1e21 * g.k0 * 2.6e-20 / res["a_eff"][0]     # n2 only in the core
