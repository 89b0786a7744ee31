"""Electric field, Poynting flux and power Grams, host side (no GPU): the NumPy emulation (tests/power_emulation.py) against
a closed-form quadratic field, the k x k host math of pl_fem_vectoriel_amd.power on hand-made Grams, the Python argument
errors that must come before any device call, and the work-buffer sizer of plfem_flux_grams against the documented
layout."""
import ctypes

import numpy as np
import pytest

import power_cases as pc
from power_emulation import PowerEmulation
from pl_fem_vectoriel_amd import ModeFields, Z0_OHM, _native, mode_power, power_quantities_from_grams
from pl_fem_vectoriel_amd.mesh import unit_square_mesh


@pytest.fixture(scope="module")
def known():
    mesh = unit_square_mesh(3)
    em = PowerEmulation(mesh.p, mesh.t)
    return em, pc.ka_all_dof_vectors(em.basis.doflocs), pc.ka_geometry()


def test_emulated_fields_equal_the_closed_forms(known):
    em, vals, g = known
    rng = np.random.default_rng(5)
    P = rng.uniform(0.02, 0.98, (2, 200))
    out, eps, elem = em.sample_e(vals, P, False, pc.KA_BETA, pc.KA_K0, g)
    assert np.all(elem >= 0) and np.all(eps == pc.KA_EPS)
    ref = pc.ka_closed_forms(P[0], P[1])
    for c, nm in enumerate(("Ex", "Ey", "Ez_im", "Sz")):
        err = np.max(np.abs(out[c] - ref[c])) / np.max(np.abs(ref[c]))
        assert err < 1e-12, (nm, err)


def test_emulated_grams_equal_the_analytic_integrals(known):
    em, vals, g = known
    G = em.flux_grams(vals, False, g)
    Mw, Gw = pc.ka_grams()
    assert np.all(G["M_w_core"] == 0) and np.all(G["G_w_core"] == 0)           # no discs: everything is "rest"
    assert np.max(np.abs(G["M_w_rest"] - Mw)) < 1e-12 * np.max(np.abs(Mw))
    assert np.max(np.abs(G["G_w_rest"] - Gw)) < 1e-12 * np.max(np.abs(Gw))
    # mode 0 by hand: int hx^2 = 1/5 + 1/2 + 4/9, int hy^2 = 1/5 + 1/9 + 1/3 - 1/4 + 1/3 - 1/3, int hx = 5/6, int hy = 7/12
    m00 = (1 / 5 + 1 / 2 + 4 / 9 + 1 / 5 + 1 / 9 + 1 / 3 - 1 / 4) / pc.KA_EPS
    g00 = (-1 * 5 / 6 - 4 * 7 / 12) / pc.KA_EPS
    assert abs(G["M_w_rest"][0, 0] - m00) < 1e-12 * m00 and abs(G["G_w_rest"][0, 0] - g00) < 1e-12 * abs(g00)
    assert not np.allclose(G["G_w_rest"], G["G_w_rest"].T)                    # G_w is not symmetric


def test_emulated_power_is_the_integral_of_sz(known):
    """P = (beta M_w + G_w / beta) / (2 k0) against the six-point sum of the emulated Sz (degree 4: exact)."""
    em, vals, g = known
    q = power_quantities_from_grams(em.flux_grams(vals, False, g), pc.KA_BETA, pc.KA_K0)
    qx, w = em.quadrature()
    out, _, _ = em.sample_e(vals, qx, False, pc.KA_BETA, pc.KA_K0, g)
    assert np.max(np.abs(out[3] @ w - q["power"]) / np.abs(q["power"])) < 1e-12


def test_power_quantities_on_hand_made_grams():
    Mc = np.array([[2.0, 0.5], [0.5, 1.0]])
    Mr = np.array([[1.0, 0.25], [0.25, 3.0]])
    Gc = np.array([[-0.5, 0.2], [0.1, -0.25]])
    Gr = np.array([[-0.25, 0.0], [0.3, -0.75]])
    beta, k0 = np.array([2.0, 4.0]), 0.5
    q = power_quantities_from_grams({"M_w_core": Mc, "M_w_rest": Mr, "G_w_core": Gc, "G_w_rest": Gr}, beta, k0)
    # P[m][n] = (beta_m M[m][n] + G[m][n] / beta_m) / (2 k0), 2 k0 = 1
    cross = np.array([[2 * 3.0 - 0.75 / 2, 2 * 0.75 + 0.2 / 2], [4 * 0.75 + 0.4 / 4, 4 * 4.0 - 1.0 / 4]])
    core = np.array([[2 * 2.0 - 0.5 / 2, 2 * 0.5 + 0.2 / 2], [4 * 0.5 + 0.1 / 4, 4 * 1.0 - 0.25 / 4]])
    assert np.allclose(q["cross"], cross, rtol=0, atol=1e-15) and np.allclose(q["cross_core"], core, rtol=0, atol=1e-15)
    assert np.array_equal(q["power"], np.diag(q["cross"]))
    assert np.allclose(q["core_fraction"], np.diag(core) / np.diag(cross), rtol=1e-15)
    sym = 0.5 * (cross + cross.T)
    assert np.allclose(q["cross_sym"], sym, rtol=1e-15)
    orth = abs(sym[0, 1]) / np.sqrt(cross[0, 0] * cross[1, 1])
    assert np.allclose(q["orthogonality"], [[0.0, orth], [orth, 0.0]], rtol=1e-15)
    assert np.allclose(q["scale"], 1.0 / np.sqrt(np.diag(cross)), rtol=1e-15)
    assert Z0_OHM == 376.730313668
    # scaled to unit power, the diagonal of the cross power is 1
    s = q["scale"]
    assert np.allclose(np.diag(s[:, None] * q["cross"] * s[None, :]), 1.0, rtol=1e-15)


def test_power_quantities_zero_power_guard_and_shapes():
    Z = np.zeros((2, 2))
    M = np.array([[0.0, 0.0], [0.0, 1.0]])
    q = power_quantities_from_grams({"M_w_core": Z, "M_w_rest": M, "G_w_core": Z, "G_w_rest": Z}, [1.0, 2.0], 1.0)
    assert q["power"][0] == 0 and q["core_fraction"][0] == 0 and q["scale"][0] == 0
    assert np.all(np.isfinite(q["orthogonality"])) and np.all(q["orthogonality"] == 0)
    assert q["scale"][1] == 1.0 and q["core_fraction"][1] == 0.0
    E = np.zeros((0, 0))
    q = power_quantities_from_grams({"M_w_core": E, "M_w_rest": E, "G_w_core": E, "G_w_rest": E}, [], 1.0)
    assert {nm: v.shape for nm, v in q.items()} == {"cross": (0, 0), "cross_core": (0, 0), "power": (0,), "core_fraction": (0,),
                                                    "cross_sym": (0, 0), "orthogonality": (0, 0), "scale": (0,)}
    G = {"M_w_core": Z, "M_w_rest": Z, "G_w_core": Z, "G_w_rest": Z}
    for bad in ((G, [1.0, 0.0], 1.0), (G, [1.0, np.nan], 1.0), (G, [1.0, 2.0], 0.0), (G, [1.0, 2.0], np.inf), (G, [1.0], 1.0),
                ({"M_w_core": Z}, [1.0, 2.0], 1.0)):
        with pytest.raises(ValueError):
            power_quantities_from_grams(*bad)


def test_python_argument_errors_come_before_any_device_call():
    mesh = unit_square_mesh(3)
    mf = ModeFields(mesh)
    rng = np.random.default_rng(6)
    good = pc.records(rng, mf.nsolve, 2)
    g = pc.rim_discs()
    P = np.zeros((2, 3))
    scalar = [{"field_vector": rng.standard_normal(mf.N)}]
    for call in (lambda: mf.flux_grams(scalar, g), lambda: mf.sample_e(scalar, P, g), lambda: mf.sample_grid_e(scalar, 3, 3, g),
                 lambda: mode_power(scalar, mesh, g, fields=mf)):
        with pytest.raises(ValueError, match="the electric field needs vectorial records"):
            call()
    for b in (0.0, np.nan, np.inf):
        bad = [dict(good[0]), dict(good[1], beta=b)]
        for call in (lambda: mf.flux_grams(bad, g), lambda: mf.sample_e(bad, P, g), lambda: mode_power(bad, mesh, g, fields=mf)):
            with pytest.raises(ValueError, match="beta"):
                call()
    no_beta = [{"Ex_dofs": good[0]["Ex_dofs"], "Ey_dofs": good[0]["Ey_dofs"]}]
    with pytest.raises(ValueError, match="beta"):
        mf.flux_grams(no_beta, g)
    for pts in (np.zeros(3), np.zeros((3, 2)), np.zeros((2, 3, 1))):
        with pytest.raises(ValueError, match="points"):
            mf.sample_e(good, pts, g)
    with pytest.raises(ValueError, match="nx and ny"):
        mf.sample_grid_e(good, 0, 3, g)

    class Bare:                      # neither a profile nor cores / n_core
        k0 = 4.0

    class NoIndex:                   # discs without n_core / n_clad
        k0 = 4.0
        positions, core_radii = np.zeros((1, 2)), np.ones(1)

    for geom in (Bare(), NoIndex()):
        for call in (lambda: mf.flux_grams(good, geom), lambda: mf.sample_e(good, P, geom),
                     lambda: mode_power(good, mesh, geom, fields=mf)):
            with pytest.raises(ValueError, match="geometry"):
                call()
    with pytest.raises(ValueError, match="wrong length|one entry per interior"):
        mf.flux_grams([dict(good[0], Ex_dofs=np.zeros(3), Ey_dofs=np.zeros(3))], g)
    # k = 0: empty results, the device untouched
    assert {nm: v.shape for nm, v in mf.flux_grams([], g).items()} == {nm: (0, 0) for nm in
                                                                         ("M_w_core", "M_w_rest", "G_w_core", "G_w_rest")}
    r = mf.sample_e([], P, g)
    assert all(r[nm].shape == (0, 3) for nm in ("Ex", "Ey", "Ez_im", "Sz")) and r["eps"].shape == (3,) and r["element"].shape == (3,)
    assert mode_power([], mesh, g, fields=mf)["power"].shape == (0,)
    assert mf._loc is None                                                       # nothing created a locator


def test_flux_gram_sizer_is_the_documented_layout(built_library):
    """plfem.h: nout k^2 doubles, rounded up to 256 bytes, plus nout ceil(k / 32)^2 x 768 partial blocks of 8 KiB, nout = 4."""
    fn = built_library.plfem_flux_gram_work_bytes
    for k in (1, 31, 32, 33, 64, 65, 96):
        need = ctypes.c_int64(-7)
        assert fn(k, ctypes.byref(need)) == _native.PLFEM_OK, k
        nc = (k + 31) // 32
        assert need.value == (4 * k * k * 8 + 255) // 256 * 256 + 4 * nc * nc * 768 * 8192, k
        # the layout of plfem_profile_grams (nout = 4 for ncomp = 2): one gram_layout
        other = ctypes.c_int64(0)
        assert built_library.plfem_profile_gram_work_bytes(2, k, ctypes.byref(other)) == _native.PLFEM_OK
        assert other.value == need.value, k
        assert fn(k, None) == _native.PLFEM_EINVAL
    for k in (0, -1):
        need = ctypes.c_int64(-7)
        assert fn(k, ctypes.byref(need)) == _native.PLFEM_EINVAL and need.value == -7, k
