"""Tangents of index profiles on the host: ProfileTangent.epsilon is the exact first-order change of IndexProfile.epsilon
(layers, graded cores, maps, points on closed rims), the NumPy emulation of the tangent Gram kernel against differences of
the oracle's pencils between two profiled geometries, the k x k host math of profile_response against hand-built
pencils, the guards of every new Python entry with the device never touched, and the argument checks of the C ABI that
need no device."""
import ctypes

import numpy as np
import pytest

from oracle import hfield, scalar
from pl_fem_vectoriel_amd import (IndexProfile, ModeFields, ProfiledGeometry, ProfileTangent, _native, profile_bend_from_grams,
                                  profile_bend_response, profile_dispersion, profile_dispersion_from_grams,
                                  profile_sensitivity, profile_sensitivity_from_grams)
from pl_fem_vectoriel_amd.bend import bend_propagate
from map_cases import m3l_profile
from profile_cases import p5, p5_profile, three_core, tie_square
from tangent_gram_emulation import TangentGramEmulation, moved_profile, random_tangent


@pytest.fixture(scope="module")
def three(built_library):
    g, mesh = three_core()
    return g, mesh, TangentGramEmulation(mesh.p, mesh.t)


@pytest.fixture(scope="module")
def square():
    ties, g, pgt, mesh = tie_square()
    return ties, g, pgt, mesh, TangentGramEmulation(mesh.p, mesh.t)


def step_p5() -> IndexProfile:
    """P5 with its graded core made a step: constant layers only."""
    return (IndexProfile(1.0).disc((0.8, 1.4), 9.0, 1.45).ring((5.0, 0.0), 1.3, 2.2, 1.40).disc((0.0, 0.0), 1.5, 1.535)
            .disc((5.0, 0.0), 1.3, 1.530).disc((-2.5, 4.33), 1.1, 1.540))


# ---- tangents ------------------------------------------------------------------------------------------------------
def test_tangent_is_the_exact_change_of_epsilon(three, square):
    _, _, em = three
    ties, _, pgt, _, ems = square
    cases = (("p5", p5_profile(), em), ("tie square", pgt.index_profile, ems), ("m3l", m3l_profile(), em))
    for name, prof, e in cases:
        qx, qy = e.basis.qx
        tan = random_tangent(prof, seed=11)
        assert (tan.d_map is not None) == (prof.index_map is not None)
        moved = moved_profile(prof, tan, 1.0)
        eps = prof.epsilon(qx, qy)
        err = np.abs((moved.epsilon(qx, qy) - eps) - tan.epsilon(qx, qy)).max() / eps.max()
        print(f"{name}: |eps' - eps - d eps| max {err:.1e} of max eps")
        assert err <= 1e-12
    # the tie points on the closed rims of the square: the tangent puts them in the layer the profile puts them in
    prof = pgt.index_profile
    qx, qy = ems.basis.qx
    unit = prof.unit_tangents()
    assert len(unit) == len(prof) + 1
    for kind in ("on", "ulp_out"):
        i = ties.kinds.index(kind)
        e, q = ties.targets[i]
        owner = [l for l in range(len(unit)) if unit[l].epsilon(qx[e, q], qy[e, q]) != 0.0]
        ring = len(prof) - 2 + ("on", "ulp_out").index(kind)           # the two rings painted last
        assert owner == [ring + 1] and float(unit[ring + 1].epsilon(qx[e, q], qy[e, q])) == 2.0 * np.sqrt(prof.table()[ring, 4])


def test_unit_tangents_partition_the_index_change(three):
    _, _, em = three
    qx, qy = em.basis.qx
    for prof in (p5_profile(), m3l_profile()):
        unit = prof.unit_tangents()
        assert len(unit) == len(prof) + 1 and all(isinstance(t, ProfileTangent) for t in unit)
        assert (unit[0].d_map is not None) == (prof.index_map is not None) and all(t.d_map is None for t in unit[1:])
        for l, t in enumerate(unit[1:]):
            row = t.row()
            assert row.shape == (1 + 2 * len(prof),) and row.dtype == np.float64 and np.count_nonzero(row) == 2
            assert np.array_equal(row[1 + 2 * l:3 + 2 * l], 2.0 * np.sqrt(prof.table()[l, 4:6]))
    # constant layers, no map: dn = 1 on everything is d eps = 2 n at every point, each point counted by exactly one tangent
    prof = step_p5()
    total = sum(t.epsilon(qx, qy) for t in prof.unit_tangents())
    assert np.abs(total - 2.0 * np.sqrt(prof.epsilon(qx, qy))).max() <= 1e-15
    # tangent_index: centre and edge of a graded layer separately, the map by 2 sqrt(E) dn
    prof = m3l_profile()
    t = prof.tangent_index(0.5, [0.25, 0.125], 2.0)
    assert t.d_eps_background == 1.0 and np.array_equal(t.d_map, 4.0 * np.sqrt(prof.index_map[0]))
    assert np.array_equal(t.d_layers, 2.0 * np.sqrt(prof.table()[:, 4:6]) * np.array([[0.25], [0.125]]))
    g = p5_profile().tangent_index(dn_layers=[[0, 0], [0, 0], [1.0, 2.0], [0, 0], [0, 0]])
    assert g.d_layers[2].tolist() == [2 * 1.535, 4 * 1.50]
    assert np.array_equal(g.scaled(-0.5).d_layers, -0.5 * g.d_layers)


def test_tangent_validation():
    prof, mprof = p5_profile(), m3l_profile()
    ny, nx = mprof.index_map[0].shape
    bad = [lambda: prof.tangent_eps(np.nan), lambda: prof.tangent_eps("x"), lambda: prof.tangent_eps(0.0, [1.0, 2.0]),
           lambda: prof.tangent_eps(0.0, np.zeros((5, 3))), lambda: prof.tangent_eps(0.0, [0, 0, np.inf, 0, 0]),
           lambda: prof.tangent_eps(0.0, 0.0, np.zeros((3, 3))),                      # no map on this profile
           lambda: prof.tangent_index(0.0, 0.0, 1.0), lambda: prof.tangent_index(np.inf),
           lambda: prof.tangent_eps(0.0, [[1.0, 2.0]] + [[0.0, 0.0]] * 4),            # a constant layer has one value
           lambda: mprof.tangent_eps(0.0, 0.0, np.zeros((nx, ny))), lambda: mprof.tangent_eps(0.0, 0.0, np.full((ny, nx), np.nan)),
           lambda: mprof.tangent_index(0.0, 0.0, np.zeros(3)), lambda: ProfileTangent("no profile")]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    t = prof.tangent_eps(0.1, [[0, 0], [0, 0], [0.1, 0.2], [0, 0], [0, 0]])
    assert t.check(prof) is t and t.check(p5_profile()) is t           # the same object, or the same table
    for other in (mprof, IndexProfile(1.0).disc((0, 0), 1.0, 1.5), p5_profile().disc((0, 0), 0.2, 1.6)):
        with pytest.raises(ValueError, match="another index profile"):
            t.check(other)
    grown = p5_profile()
    tg = grown.tangent_eps(0.1)
    grown.disc((0, 0), 0.2, 1.6)                                         # the profile moved on: the tangent is stale
    with pytest.raises(ValueError, match="another index profile"):
        tg.epsilon(0.0, 0.0)
    tm = mprof.tangent_eps(0.0, 0.0, np.ones((ny, nx)))
    with pytest.raises(ValueError, match="another index profile"):
        tm.check(m3l_profile().sampled(np.linspace(-7.0, 9.0, 41), np.linspace(-5.0, 9.0, 33), np.full((33, 41), 1.2)))


# ---- the emulation against the oracle ------------------------------------------------------------------------------
def test_emulated_scalar_tangent_grams_are_the_difference_of_the_oracles_pencils(three, square):
    g, mesh, em = three
    _, gs, pgt, mesh_s, ems = square
    rng = np.random.default_rng(43)
    for name, base, prof, e in (("p5", g, p5_profile(), em), ("tie square", gs, pgt.index_profile, ems), ("m3l", g, m3l_profile(), em)):
        tan = random_tangent(prof, seed=12)
        pg, pg2 = ProfiledGeometry(base, prof), ProfiledGeometry(base, moved_profile(prof, tan, 1.0))
        k0 = base.k0
        u = rng.standard_normal((1, 4, e.N))
        Md = e.tangent_grams(u, False, prof, [tan])[0, 0]
        U = u[0].T
        S1, _, Me1, _ = scalar.assemble(pg, e.mesh)
        S2, _, Me2, _ = scalar.assemble(pg2, e.mesh)
        A1, A2 = U.T @ ((S1 - k0 ** 2 * Me1) @ U), U.T @ ((S2 - k0 ** 2 * Me2) @ U)
        err = np.abs(-k0 ** 2 * Md - (A2 - A1)).max() / np.abs(A1).max()
        print(f"{name}: |-k0^2 M_d - (A' - A)| max {err:.1e} of max |A|")
        assert err <= 1e-12


def test_emulated_vectorial_tangent_grams_are_the_difference_of_the_oracles_pencils(three):
    g, mesh, em = three
    prof = step_p5()
    tan = random_tangent(prof, seed=13)
    # every value moved so that 1 / eps' = 1 / eps + dw exactly: the pencil is linear in 1 / eps
    moved = moved_profile(prof, tan, eps_of=lambda eps, d: 1.0 / (1.0 / eps - d / eps ** 2))
    pg, pg2 = ProfiledGeometry(g, prof), ProfiledGeometry(g, moved)
    rng = np.random.default_rng(44)
    vals = rng.standard_normal((2, 4, em.interior.size))
    T = em.tangent_grams(vals, True, prof, [tan])[0]
    V = np.hstack([vals[0], vals[1]]).T
    P = []
    for geo in (pg, pg2):
        A, B, basis, *_ = hfield.assemble_hfield_system_fused(geo, em.mesh)
        A, B, _ = hfield.restrict_interior(A, B, basis)
        P.append((V.T @ (A @ V), V.T @ (B @ V)))
    scale = np.abs(P[0][0]).max()
    ea, eb = np.abs(T[1] - (P[1][0] - P[0][0])).max() / scale, np.abs(T[0] - (P[1][1] - P[0][1])).max() / scale
    print(f"|K_d - V^T (A' - A) V| max {ea:.1e}, |M_d - V^T (B' - B) V| max {eb:.1e} of max |A|")
    assert ea <= 1e-12 and eb <= 1e-12
    assert np.abs(T[1]).max() > 1e-4 * scale                             # (the change is no rounding of A)


def test_emulated_point_weights_of_graded_layers_and_maps(three):
    _, _, em = three
    qx, qy = em.basis.qx
    for prof in (p5_profile(), m3l_profile()):
        tans = [random_tangent(prof, seed=14), random_tangent(prof, seed=15, with_map=False)] + prof.unit_tangents()
        eps = prof.epsilon(qx, qy)
        W2 = em.column_weights(prof, tans, 2, moments=True, origin=(0.3, -0.2))
        W1 = em.column_weights(prof, tans, 1, moments=True, origin=(0.3, -0.2))
        assert W2.shape == W1.shape == (len(tans) + 2,) + qx.shape
        for i, t in enumerate(tans):
            want = -t.epsilon(qx, qy) / eps ** 2
            assert np.abs(W2[i] - want).max() <= 4 * 2.0 ** -52 * np.abs(want).max()
            assert np.array_equal(W1[i], t.epsilon(qx, qy))
        assert np.array_equal(W2[-2], (1.0 / eps) * (qx - 0.3)) and np.array_equal(W1[-1], eps * (qy + 0.2))
        if prof.index_map is not None:                                   # a tangent without a map: flat inside the extent too
            top, _, inside, _ = prof._placement(qx, qy)
            bare = inside & (top < 0)
            assert bare.sum() > 1000 and np.all(tans[1].epsilon(qx, qy)[bare] == tans[1].d_eps_background)
            assert np.unique(tans[0].epsilon(qx, qy)[bare]).size > 1000


# ---- k x k host math -----------------------------------------------------------------------------------------------
def _scalar_case():
    """Three scalar records, the first two degenerate: M = I, A = diag(-beta^2)."""
    rng = np.random.default_rng(3)
    k0, beta = 4.0, np.array([6.0, 6.0, 5.0])
    R = rng.standard_normal((3, 3))
    Mw = R @ R.T + 3.0 * np.eye(3)
    grams = {"M": np.eye(3), "M_w": Mw, "S": np.diag(-beta ** 2) + k0 ** 2 * Mw}
    T = rng.standard_normal((2, 3, 3))
    return k0, beta, grams, T + T.transpose(0, 2, 1)


def test_scalar_from_grams_against_a_hand_built_pencil_with_a_degenerate_pair():
    k0, beta, grams, T = _scalar_case()
    res = profile_sensitivity_from_grams("scalar", grams, {"M_d": T}, beta, k0, direction=[1.0, -2.0])
    assert res["cluster"].tolist() == [0, 0, -1] and res["rayleigh_defect"].max() <= 1e-14
    assert res["dneff_dp"].shape == (3, 2) and res["sensitivity"].shape == (2, 3, 3)
    assert np.allclose(res["sensitivity"], -k0 ** 2 * T, rtol=1e-14, atol=0)
    for p in range(2):
        # lambda = -beta^2: d n_eff = -d lambda / (2 beta k0); the pair takes the eigenvalues of the cluster block, ascending
        pair = np.linalg.eigvalsh(-k0 ** 2 * T[p][:2, :2])
        want = -np.array([pair[0], pair[1], -k0 ** 2 * T[p][2, 2]]) / (2 * beta * k0)
        assert np.allclose(res["dneff_dp"][:, p], want, rtol=1e-13, atol=1e-12)
    Td = T[0] - 2.0 * T[1]
    pair = np.linalg.eigvalsh(-k0 ** 2 * Td[:2, :2])
    assert np.allclose(res["dneff_direction"], -np.array([pair[0], pair[1], -k0 ** 2 * Td[2, 2]]) / (2 * beta * k0), rtol=1e-13)
    # dispersion: A' = -2 k0 M_w - k0^2 M_d, n_g = -d lambda / (2 beta)
    for tg in (None, {"M_d": T[:1]}, {"M_d": T[0]}):
        disp = profile_dispersion_from_grams("scalar", grams, tg, beta, k0)
        Ad = -2 * k0 * grams["M_w"] - (0.0 if tg is None else k0 ** 2 * T[0])
        pair = np.linalg.eigvalsh(Ad[:2, :2])
        assert np.allclose(disp["n_g"], -np.array([pair[0], pair[1], Ad[2, 2]]) / (2 * beta), rtol=1e-13, atol=1e-12)
        assert disp["cluster"].tolist() == [0, 0, -1] and len(disp["cluster_rotation"]) == 1
        assert set(disp) >= {"n_g", "group_delay_ps_per_m", "dmgd_ps_per_m", "coupling", "rayleigh_defect"}
    # bend: A1 = -2 k0^2 M_wX/Y; the pencil feeds bend_propagate
    mg = {"M_clad_X": np.diag([0.5, -0.25, 1.0]), "M_clad_Y": np.diag([0.0, 0.125, -1.0]), "M_XX": 2.0 * np.eye(3),
          "M_XY": np.zeros((3, 3)), "M_YY": 3.0 * np.eye(3)}
    bend = profile_bend_from_grams("scalar", grams, {"M_wX": T[0], "M_wY": T[1]}, mg, beta, k0, curvature=[1e-4], angle=0.0)
    assert np.array_equal(bend["centroid"], np.array([[0.5, 0.0], [-0.25, 0.125], [1.0, -1.0]]))
    assert np.allclose(bend["pencil"]["A1"], -2 * k0 ** 2 * T, rtol=1e-14, atol=0) and not bend["pencil"]["B1"].any()
    pair = np.linalg.eigvalsh(-2 * k0 ** 2 * T[0][:2, :2])
    assert np.allclose(bend["dneff_dkappa"], -np.array([pair[0], pair[1], -2 * k0 ** 2 * T[0][2, 2]]) / (2 * beta * k0), rtol=1e-13)
    assert bend["n_eff_ritz"].shape == (1, 3)
    out = bend_propagate(bend, [[100.0, 1e-4, 0.0]])
    assert np.allclose(out["transfer"].conj().T @ out["transfer"], np.eye(3), atol=1e-12)


def test_vectorial_from_grams_against_a_hand_built_2x2_pencil():
    k0, beta, b = 4.0, np.array([6.0, 5.5]), np.array([2.0, 0.5])
    mu = beta ** 2
    grams = {"M": np.eye(2), "M_w": np.diag(b), "D": np.zeros((2, 2)), "K_w": np.diag(mu * b) + k0 ** 2 * np.eye(2)}
    Md = np.array([[[0.3, 0.1], [0.1, -0.2]]])
    Kd = np.array([[[1.0, 0.5], [0.5, 2.0]]])
    res = profile_sensitivity_from_grams("vectorial", grams, {"M_d": Md, "K_d": Kd}, beta, k0)
    assert res["cluster"].tolist() == [-1, -1] and res["rayleigh_defect"].max() <= 1e-14
    dmu = (np.diag(Kd[0]) - mu * np.diag(Md[0])) / b                    # Hellmann-Feynman on h = e_i / sqrt(b_i)
    assert np.allclose(res["dneff_dp"][:, 0], dmu / (2 * beta * k0), rtol=1e-14, atol=0)
    assert np.isclose(res["sensitivity"][0, 0, 1], (Kd[0, 0, 1] - mu[1] * Md[0, 0, 1]) / np.sqrt(b[0] * b[1]), rtol=1e-14)
    disp = profile_dispersion_from_grams("vectorial", grams, {"M_d": Md, "K_d": Kd}, beta, k0)
    dmu = (np.diag(-2 * k0 * np.eye(2) + Kd[0]) - mu * np.diag(Md[0])) / b
    assert np.allclose(disp["n_g"], dmu / (2 * beta), rtol=1e-14, atol=0)
    assert np.allclose(np.diag(disp["coupling"]), -0.5 * np.diag(Md[0]) / b, rtol=1e-14, atol=0)
    mg = {"M_clad_X": np.eye(2), "M_clad_Y": np.zeros((2, 2)), "M_XX": 2.0 * np.eye(2), "M_XY": np.zeros((2, 2)), "M_YY": 2.0 * np.eye(2)}
    bend = profile_bend_from_grams("vectorial", grams, {"M_wX": Md[0], "M_wY": 2 * Md[0], "K_wX": Kd[0], "K_wY": 2 * Kd[0]}, mg, beta, k0,
                                   angle=np.pi / 2)
    dmu = -4.0 * (np.diag(Kd[0]) - mu * np.diag(Md[0])) / b             # along y: A1 = -2 K_wY, B1 = -2 M_wY
    assert np.allclose(bend["dneff_dkappa"], dmu / (2 * beta * k0), rtol=1e-13, atol=1e-12)
    with pytest.raises(ValueError):
        bend_propagate(bend, [[1.0, 0.0, 0.0]])                          # vectorial: B moves with the bend
    for call in (lambda: profile_sensitivity_from_grams("vectorial", grams, {"M_d": Md}, beta, k0),
                 lambda: profile_sensitivity_from_grams("tensor", grams, {"M_d": Md, "K_d": Kd}, beta, k0),
                 lambda: profile_sensitivity_from_grams("vectorial", grams, {"M_d": Md, "K_d": Kd}, beta, k0, direction=[1, 2]),
                 lambda: profile_sensitivity_from_grams("vectorial", grams, {"M_d": Md[0], "K_d": Kd[0]}, beta, k0),
                 lambda: profile_dispersion_from_grams("vectorial", grams, {"M_d": np.repeat(Md, 2, 0), "K_d": np.repeat(Kd, 2, 0)}, beta, k0),
                 lambda: profile_dispersion_from_grams("vectorial", {"M": np.eye(2)}, None, beta, k0),
                 lambda: profile_bend_from_grams("vectorial", grams, {"M_wX": Md[0], "M_wY": Md[0]}, mg, beta, k0),
                 lambda: profile_bend_from_grams("vectorial", grams, {"M_wX": Md[0], "M_wY": Md[0], "K_wX": Kd[0], "K_wY": Kd[0]}, {}, beta, k0),
                 lambda: profile_sensitivity_from_grams("vectorial", grams, {"M_d": Md, "K_d": Kd}, beta, k0, cluster_rtol=-1.0)):
        with pytest.raises(ValueError):
            call()


# ---- guards: nothing touches the device ----------------------------------------------------------------------------
def _records(kind, em, k=3):
    rng = np.random.default_rng(2)
    if kind == "vectorial":
        return [{"Ex_dofs": rng.standard_normal(em.interior.size), "Ey_dofs": rng.standard_normal(em.interior.size),
                 "beta": 6.0 + i, "n_eff": 1.48 + 0.01 * i} for i in range(k)]
    return [{"field_vector": rng.standard_normal(em.N), "beta": 6.0 + i, "n_eff": 1.48 + 0.01 * i} for i in range(k)]


def test_new_entries_check_their_arguments_before_the_device(three, monkeypatch):
    g, mesh, em = three
    pg = p5(g)
    prof = pg.index_profile
    mf = ModeFields(mesh)
    monkeypatch.setattr(ModeFields, "_ensure_locator", lambda self: pytest.fail("the device was touched"))
    monkeypatch.setattr(_native, "Context", lambda *a, **kw: pytest.fail("the device was touched"))
    unit = prof.unit_tangents()
    foreign = p5_profile().disc((0, 0), 0.2, 1.6).tangent_eps(0.1)
    for kind in ("vectorial", "scalar"):
        modes = _records(kind, em)
        short = [dict(m) for m in modes]
        for m in short:
            for key in ("Ex_dofs", "Ey_dofs", "field_vector"):
                if key in m:
                    m[key] = m[key][:-1]
        nobeta = [{k: v for k, v in m.items() if k != "beta"} for m in modes]
        bad = [lambda: mf.profile_tangent_grams(modes, g, unit),                       # no profile
               lambda: mf.profile_tangent_grams(modes, pg, [foreign]), lambda: mf.profile_tangent_grams(modes, pg, ["x"]),
               lambda: mf.profile_tangent_grams(modes, pg, 3), lambda: mf.profile_tangent_grams(modes, pg, unit * 50),
               lambda: mf.profile_tangent_grams(modes, pg, unit, origin=(0.0, np.nan)),
               lambda: mf.profile_tangent_grams(modes, pg, unit, origin=(0.0,)),
               lambda: mf.profile_tangent_grams(modes, pg, ()), lambda: mf.profile_tangent_grams(short, pg, unit),
               lambda: mf.profile_tangent_grams(modes[0], pg, unit),
               lambda: profile_dispersion(modes, mf, g), lambda: profile_sensitivity(modes, mf, g),
               lambda: profile_bend_response(modes, mf, g),
               lambda: profile_dispersion(modes, mf, pg, dn_dlambda=(0.0, 0.0)), lambda: profile_dispersion(modes, mf, pg, dn_dlambda=foreign),
               lambda: profile_dispersion(modes, mf, pg, cluster_rtol=-1.0), lambda: profile_dispersion([], mf, pg),
               lambda: profile_dispersion(nobeta, mf, pg), lambda: profile_dispersion(short, mf, pg),
               lambda: profile_sensitivity(modes, mf, pg, tangents=[foreign]), lambda: profile_sensitivity(modes, mf, pg, tangents=[]),
               lambda: profile_sensitivity(modes, mf, pg, direction=[1.0, 2.0]), lambda: profile_sensitivity(modes, mf, pg, direction="x"),
               lambda: profile_sensitivity(nobeta, mf, pg), lambda: profile_sensitivity(short, mf, pg),
               lambda: profile_bend_response(modes, mf, pg, radius=0.0), lambda: profile_bend_response(modes, mf, pg, radius=np.nan),
               lambda: profile_bend_response(modes, mf, pg, radius=10.0),             # 2 |x| / R reaches 1 on this mesh
               lambda: profile_bend_response(modes, mf, pg, angle=[0.0, 1.0]),
               lambda: profile_bend_response(modes, mf, pg, origin=(np.inf, 0.0)), lambda: profile_bend_response(short, mf, pg)]
        for i, f in enumerate(bad):
            with pytest.raises(ValueError):
                f()
                pytest.fail(f"call {i} was accepted")
    # k = 0: empty arrays of the documented shapes
    none = mf.profile_tangent_grams([], pg, unit, moments=True)
    assert none == {}
    # the two-region entries still refuse the profiled geometry, and say where to go
    from pl_fem_vectoriel_amd import mode_dispersion
    with pytest.raises(ValueError, match="profile_grams.*profile_dispersion"):
        mode_dispersion(_records("scalar", em), mf, pg)


def test_tangent_result_shapes():
    for kind, names in (("vectorial", ("M", "K")), ("scalar", ("M",))):
        out = np.arange(5 * 2 * 9, dtype=np.float64).reshape(5, 2, 3, 3)
        res = ModeFields._tangent_result(kind, out, 3, True)
        assert set(res) == {n + s for n in names for s in ("_d", "_wX", "_wY")}
        assert res["M_d"].shape == (3, 3, 3) and np.array_equal(res["M_wY"], out[4, 0]) and np.array_equal(res["M_wX"], out[3, 0])
        assert set(ModeFields._tangent_result(kind, out[:3], 3, False)) == {n + "_d" for n in names}
        empty = ModeFields._tangent_result(kind, np.zeros((4, 2, 0, 0)), 2, True)
        assert empty["M_d"].shape == (2, 0, 0) and empty["M_wX"].shape == (0, 0)


def test_tangent_entries_refuse_bad_arguments_on_the_host(built_library):
    lib = _native.load_library()
    assert {"plfem_profile_tangent_gram_work_bytes", "plfem_profile_tangent_grams"} <= set(_native.EXPORTS)
    b = ctypes.c_int64(-1)
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)                                       # never dereferenced: the locator is checked first
    assert lib.plfem_profile_tangent_gram_work_bytes(null, 2, 22, 4, 0, 1, ctypes.byref(b)) == _native.PLFEM_EINVAL
    assert lib.plfem_profile_tangent_gram_work_bytes(null, 2, 22, 4, 0, 1, None) == _native.PLFEM_EINVAL
    for ncomp, k, ntan, nmap, mom in ((0, 5, 1, 0, 0), (3, 5, 1, 0, 0), (2, 0, 1, 0, 0), (2, 5, 0, 0, 0), (2, 5, 257, 0, 0), (1, 5, 4, 5, 1)):
        assert lib.plfem_profile_tangent_gram_work_bytes(null, ncomp, k, ntan, nmap, mom, ctypes.byref(b)) == _native.PLFEM_EINVAL
        assert lib.plfem_profile_tangent_grams(null, ncomp, k, one, 0, one, 3, 1.0, one, ntan, one, nmap, one, mom, one, one,
                                               1 << 30, one) == _native.PLFEM_EINVAL
    assert b.value == -1
    assert lib.plfem_profile_tangent_grams(null, 2, 5, None, 1, None, 3, 1.0, None, 1, None, 0, None, 0, None, None, 0,
                                           None) == _native.PLFEM_EINVAL
