"""Electric field, Poynting flux and power Grams on the GPU (plfem_flux_grams: k_flux_grams + k_overlap_reduce;
plfem_sample_efields: k_sample_efields) on seeded random DOF vectors against the NumPy emulation (tests/power_emulation.py),
against the existing Grams, against each other, against a closed-form quadratic field, bit for bit on repeats, dirty work
buffers and permuted modes, and on one small solve.

Meshes: unit_square_mesh(5) (300 quadrature points = 18.75 tiles of 16: a ragged last tile), unit_square_mesh(40) (1200
tiles > 768 workgroups: the grid-stride path), and the annulus of tests/topology_cases.py (a hole).  Materials: two
overlapping discs, the first with (0.75, 0.5) exactly on its rim; a ring plus a graded layer; the same over an 8 x 5
sampled map.

Tolerances.  Grams against the emulation: 1e-12 of each output's largest |entry|, the project's bar for Grams.  Sampled E
and Sz against the emulation: 1e-12 of the component's largest |value|.  M_w_core + M_w_rest against the existing Grams:
1e-13 of the largest |entry| (the same products, summed in another grouping).  The six-point sum of the sampled Sz against
the Gram power: 1e-11 relative."""
import ctypes

import numpy as np
import pytest

import power_cases as pc
import topology_cases as tc
from power_emulation import E_NAMES, NAMES, PowerEmulation
from pl_fem_vectoriel_amd import IndexProfile, ModeFields, ProfiledGeometry, _native, generate_mesh, mode_power, power_quantities_from_grams
from pl_fem_vectoriel_amd.mesh import unit_square_mesh
from pl_fem_vectoriel_amd.solver_fem import TrueVectorialMaxwellSolver

pytestmark = pytest.mark.gpu

KS = (1, 31, 32, 33, 65)
KMAX = 65
GRAM_TOL = 1e-12
SAMPLE_TOL = 1e-12
SUM_TOL = 1e-13
CROSS_TOL = 1e-11
NPTS = (1, 63, 64, 65, 257)


class Case:
    def __init__(self, mesh, device, seed):
        self.mesh = mesh
        self.mf = ModeFields(mesh, device=device)
        self.em = PowerEmulation(mesh.p, mesh.t)
        self.modes = pc.records(np.random.default_rng(seed), self.mf.nsolve, KMAX)
        self._ref = {}

    def reference(self, name, geometry):
        """The emulated Grams of all KMAX modes under the named geometry: computed once, never modified."""
        if name not in self._ref:
            self._ref[name] = self.em.flux_grams(pc.vals_of(self.modes), True, geometry)
            for v in self._ref[name].values():
                v.setflags(write=False)
        return self._ref[name]


@pytest.fixture(scope="module")
def cases(gpu_device, built_library):
    out = {"sq5": Case(unit_square_mesh(5), gpu_device, 1), "sq40": Case(unit_square_mesh(40), gpu_device, 2),
           "annulus": Case(tc.trimesh("annulus"), gpu_device, 3)}
    assert out["sq5"].mf.ne == 50 and (6 * 50) % 16 != 0                   # a ragged last tile
    assert out["sq40"].mf.ne == 3200 and 6 * 3200 // 16 > 768                # more tiles than workgroups
    yield out
    for c in out.values():
        c.mf.close()
    import torch
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def geoms():
    """Unit-square geometries by name; ``annulus_*`` are their counterparts on the annulus ([-12, 12]^2, hole of radius 5)."""
    ring = lambda: IndexProfile(1.2).ring((0.0, 0.0), 6.0, 9.0, 1.40).graded((7.0, 1.0), 2.5, 1.535, 1.45, 2)
    big = pc.discs([[7.0, 0.0], [8.5, -1.5]], [2.5, 2.0])
    return {"discs": pc.rim_discs(), "profile": pc.profiled(pc.ring_profile()), "map": pc.profiled(pc.map_profile()),
            "uniform": pc.no_discs(1.5),
            "profile, no discs": ProfiledGeometry(pc.no_discs(1.5), pc.ring_profile(), n_core=1.535, n_clad=1.2),
            "annulus_discs": big, "annulus_profile": ProfiledGeometry(big, ring(), n_core=1.535, n_clad=1.2)}


def assert_grams_close(got, ref, tol, what):
    for nm in NAMES:
        scale = np.max(np.abs(ref[nm])) if ref[nm].size else 0.0
        if scale == 0.0:
            assert np.all(got[nm] == 0.0), (what, nm)
            continue
        err = np.max(np.abs(got[nm] - ref[nm])) / scale
        print(f"{what} {nm}: {err:.2e}")
        assert err < tol, (what, nm, err)


@pytest.mark.parametrize("gname", ["discs", "profile", "map"])
@pytest.mark.parametrize("mname", ["sq5", "sq40"])
def test_flux_grams_match_the_emulation(cases, geoms, mname, gname):
    case, g = cases[mname], geoms[gname]
    ref = case.reference(gname, g)
    assert all(np.max(np.abs(ref[nm])) > 0 for nm in NAMES)                 # both regions hold quadrature points
    for k in KS:
        got = case.mf.flux_grams(case.modes[:k], g)
        assert set(got) == set(NAMES) and all(v.shape == (k, k) for v in got.values())
        assert_grams_close(got, {nm: ref[nm][:k, :k] for nm in NAMES}, GRAM_TOL, f"{mname} {gname} k={k}")
    full = case.mf.flux_grams(case.modes, g)
    for nm in ("M_w_core", "M_w_rest"):
        assert np.max(np.abs(full[nm] - full[nm].T)) <= GRAM_TOL * np.max(np.abs(full[nm]))
    assert np.max(np.abs(full["G_w_rest"] - full["G_w_rest"].T)) > 1e-3 * np.max(np.abs(full["G_w_rest"]))   # G_w is not symmetric


def test_flux_grams_on_a_holed_mesh(cases, geoms):
    case = cases["annulus"]
    for gname in ("annulus_discs", "annulus_profile"):
        g = geoms[gname]
        got = case.mf.flux_grams(case.modes[:33], g)
        ref = case.reference(gname, g)
        assert_grams_close(got, {nm: ref[nm][:33, :33] for nm in NAMES}, GRAM_TOL, f"annulus {gname}")


@pytest.mark.parametrize("mname", ["sq5", "sq40"])
def test_weighted_mass_is_that_of_the_existing_grams(cases, geoms, mname):
    case = cases[mname]
    modes = case.modes[:33]
    for gname in ("profile", "map", "profile, no discs"):
        g = geoms[gname]
        F = case.mf.flux_grams(modes, g)
        Mw = case.mf.profile_grams(modes, g)["M_w"]
        err = np.max(np.abs(F["M_w_core"] + F["M_w_rest"] - Mw)) / np.max(np.abs(Mw))
        print(f"{mname} {gname}: M_w_core + M_w_rest against profile_grams {err:.2e}")
        assert err < SUM_TOL, (gname, err)
    for gname in ("discs", "uniform"):
        g = geoms[gname]
        F = case.mf.flux_grams(modes, g)
        G = case.mf.grams(modes, g)
        Mw = G["M_core"] / g.n_core ** 2 + G["M_clad"] / g.n_clad ** 2
        err = np.max(np.abs(F["M_w_core"] + F["M_w_rest"] - Mw)) / np.max(np.abs(Mw))
        print(f"{mname} {gname}: M_w_core + M_w_rest against grams {err:.2e}")
        assert err < SUM_TOL, (gname, err)
    for gname in ("uniform", "profile, no discs"):                          # ncore = 0: everything is "rest"
        F = case.mf.flux_grams(modes, geoms[gname])
        assert np.all(F["M_w_core"] == 0.0) and np.all(F["G_w_core"] == 0.0)
        assert np.max(np.abs(F["M_w_rest"])) > 0 and np.max(np.abs(F["G_w_rest"])) > 0


@pytest.mark.parametrize("gname", ["discs", "map"])
def test_flux_grams_bits(cases, geoms, gname):
    """A repeat, a work buffer full of NaN bytes, and a permutation / subset of the modes: the same bits."""
    import torch
    case, g = cases["sq40"], geoms[gname]
    mf = case.mf
    k = 40                                                                   # two chunks
    modes = case.modes[:k]
    first = mf.flux_grams(modes, g)
    again = mf.flux_grams(modes, g)
    mat = mf._material(g)
    need = ctypes.c_int64(0)
    assert mf._lib.plfem_flux_gram_work_bytes(k, ctypes.byref(need)) == _native.PLFEM_OK
    work = torch.full((int(need.value) + 256,), 0xFF, dtype=torch.uint8, device=mf.tdev)
    dirty = mf._flux_grams_staged(mf._staged(pc.vals_of(modes)), mat, work=work)
    perm = np.random.default_rng(8).permutation(k)[:35]                      # a subset, permuted, still two chunks
    sub = mf.flux_grams([modes[i] for i in perm], g)
    for nm in NAMES:
        assert np.array_equal(first[nm], again[nm]), nm
        assert np.array_equal(first[nm], dirty[nm]), nm
        assert np.array_equal(first[nm][np.ix_(perm, perm)], sub[nm]), nm
        assert np.all(np.isfinite(first[nm]))


def _pool(case, rng):
    """Points in a fixed order: the exact rim point, three points outside the mesh, every vertex and edge midpoint (ties
    between elements), then random interior points."""
    mf = case.mf
    dl = mf.sym.array("doflocs").reshape(2, mf.N)
    outside = np.array([[-0.25, 1.5, 0.5], [0.5, 0.5, -1e-3]])
    rnd = rng.uniform(0.0, 1.0, (2, 160))
    return np.hstack([np.array([[0.75], [0.5]]), outside, dl, rnd])


@pytest.mark.parametrize("gname", ["discs", "profile", "map"])
def test_sample_e_matches_the_emulation(cases, geoms, gname):
    case, g = cases["sq5"], geoms[gname]
    mf, em = case.mf, case.em
    pool = _pool(case, np.random.default_rng(9))
    assert pool.shape[1] >= max(NPTS)
    modes = case.modes[:33]
    vals, beta, k0 = pc.vals_of(modes), pc.betas_of(modes), float(g.k0)
    for npts in NPTS:
        P = pool[:, :npts]
        got = mf.sample_e(modes, P, g)
        ref, eps, elem = em.sample_e(vals, P, True, beta, k0, g)
        assert np.array_equal(got["element"], elem), npts                    # every point: the same element, ties included
        assert np.allclose(got["eps"], eps, rtol=1e-14, atol=0), npts
        if gname == "discs":
            assert got["eps"][0] == g.n_core ** 2                            # the rim point belongs to the core: closed discs
        out = elem < 0
        if npts >= 4:
            assert out[1:4].all() and out.sum() == 3
        for c, nm in enumerate(E_NAMES):
            assert got[nm].shape == (33, npts)
            assert np.all(got[nm][:, out] == 0.0) and np.all(got["eps"][out] == 0.0)
            err = np.max(np.abs(got[nm] - ref[c])) / np.max(np.abs(ref[c]))
            print(f"{gname} npts={npts} {nm}: {err:.2e}")
            assert err < SAMPLE_TOL, (npts, nm, err)


def test_sample_e_on_a_holed_mesh(cases, geoms):
    case, g = cases["annulus"], geoms["annulus_profile"]
    modes = case.modes[:5]
    probes = tc.probe_points("annulus")
    P = np.hstack([probes[kind] for kind in ("random", "void", "rim")])
    nvoid = probes["void"].shape[1]
    got = case.mf.sample_e(modes, P, g)
    loc = case.em.locate(P)
    ref, eps, elem = case.em.sample_e(pc.vals_of(modes), P, True, pc.betas_of(modes), float(g.k0), g, located=loc)
    void = slice(probes["random"].shape[1], probes["random"].shape[1] + nvoid)
    assert np.all(got["element"][void] == -1) and np.all(got["eps"][void] == 0.0)
    same = got["element"] == elem
    assert np.all(same | (loc[3] > 1))                                       # (a point within 1e-8 of two elements may go to either)
    assert np.all(got["element"][-probes["rim"].shape[1]:] >= 0)
    for c, nm in enumerate(E_NAMES):
        assert np.all(got[nm][:, void] == 0.0)
        err = np.max(np.abs(got[nm][:, same] - ref[c][:, same])) / np.max(np.abs(ref[c]))
        assert err < SAMPLE_TOL, (nm, err)


@pytest.mark.parametrize("gname", ["discs", "profile"])
def test_the_two_kernels_agree_on_the_power(cases, geoms, gname):
    """sample_e at the mesh's own quadrature points, summed with |det J| w_q, is the power of mode_power; the same over the
    points of the core region is its core fraction."""
    case, g = cases["sq5"], geoms[gname]
    modes = case.modes[:33]
    q = mode_power(modes, case.mesh, g, fields=case.mf)
    qx, w = case.em.quadrature()
    res = case.mf.sample_e(modes, qx, g)
    assert np.array_equal(res["element"], np.repeat(np.arange(case.mf.ne), 6))     # every point in its own element
    power = res["Sz"] @ w
    err = np.max(np.abs(power - q["power"]) / np.abs(q["power"]))
    print(f"{gname}: six-point sum of Sz against the Gram power {err:.2e}")
    assert err < CROSS_TOL, err
    core = case.em.region_mask(g).reshape(-1)
    if gname == "discs":
        assert np.array_equal(core, res["eps"] == g.n_core ** 2)             # the returned eps shows the region
    frac = (res["Sz"][:, core] @ w[core]) / power
    err = np.max(np.abs(frac - q["core_fraction"]) / np.abs(q["core_fraction"]))
    print(f"{gname}: core fraction {err:.2e}")
    assert err < CROSS_TOL, err


def test_known_answer_through_the_kernels(gpu_device, built_library):
    """The quadratic fields of tests/test_power_host.py as all-DOF vectors (indexed = 0, through the C ABI): E and Sz at
    random interior points equal the closed forms, the Grams the analytic integrals, to 1e-12."""
    import torch
    mesh = unit_square_mesh(3)
    mf = ModeFields(mesh, device=gpu_device)
    try:
        mf._ensure_locator()
        vals = pc.ka_all_dof_vectors(mf.sym.array("doflocs").reshape(2, mf.N))
        staged = mf._staged(np.ascontiguousarray(vals))
        mat = mf._material(pc.ka_geometry())
        mf._set_index_map(None)
        out = np.empty((4, 2, 2))
        mf._work_call("plfem_flux_gram_work_bytes", {"k": 2}, "plfem_flux_grams",
                      (mf._loc, 2, 2, staged.data_ptr(), 0, *mf._material_args(mat)), (out,))
        Mw, Gw = pc.ka_grams()
        assert np.all(out[0] == 0.0) and np.all(out[2] == 0.0)
        assert np.max(np.abs(out[1] - Mw)) < 1e-12 * np.max(np.abs(Mw))
        assert np.max(np.abs(out[3] - Gw)) < 1e-12 * np.max(np.abs(Gw))
        P = np.random.default_rng(5).uniform(0.02, 0.98, (2, 200))
        with torch.cuda.stream(mf.stream):
            pd = torch.from_numpy(P).to(mf.tdev)
            bd = torch.tensor(pc.KA_BETA, dtype=torch.float64, device=mf.tdev)
            od = torch.empty((4, 2, 200), dtype=torch.float64, device=mf.tdev)
            ed = torch.empty(200, dtype=torch.int32, device=mf.tdev)
            mf._check(mf._lib.plfem_sample_efields(mf._loc, 2, 2, staged.data_ptr(), 0, bd.data_ptr(), pc.KA_K0,
                                                   *mf._material_args(mat), 200, pd.data_ptr(), od.data_ptr(), None,
                                                   ed.data_ptr()), "plfem_sample_efields")     # eps_dev = NULL
        got, ref = od.cpu().numpy(), pc.ka_closed_forms(P[0], P[1])
        assert np.all(ed.cpu().numpy() >= 0)
        for c, nm in enumerate(E_NAMES):
            err = np.max(np.abs(got[c] - ref[c])) / np.max(np.abs(ref[c]))
            print(f"known answer {nm}: {err:.2e}")
            assert err < 1e-12, (nm, err)
    finally:
        mf.close()


def test_power_of_solved_modes(gpu_device, built_library):
    """One small solve: the power quantities are finite, the cross power reproduces the emulation, a sampled grid is finite
    and reproduces bit for bit.  Power orthogonality and core fractions of the solver's modes are printed, not asserted:
    the pencil's sign convention is the reference's as coded."""
    g = tc.two_core_geometry()
    mesh = generate_mesh(g, 0.5, 0)
    solver = TrueVectorialMaxwellSolver(g, device=gpu_device)
    modes = solver.solve_vectorial_modes(mesh, n_modes_target=4)
    assert len(modes) >= 2
    mf = ModeFields(mesh, device=gpu_device, solver=solver)
    try:
        q = mode_power(modes, mesh, g, fields=mf)
        for nm in ("cross", "cross_core", "power", "core_fraction", "cross_sym", "orthogonality", "scale"):
            assert np.all(np.isfinite(q[nm])), nm
        em = PowerEmulation(mesh.p, mesh.t)
        ref = power_quantities_from_grams(em.flux_grams(pc.vals_of(modes), True, g), pc.betas_of(modes), float(g.k0))
        err = np.max(np.abs(q["cross"] - ref["cross"])) / np.max(np.abs(ref["cross"]))
        print(f"cross power against the emulation: {err:.2e}")
        assert err < 1e-10, err
        a = mf.sample_grid_e(modes, 33, 33, g)
        b = mf.sample_grid_e(modes, 33, 33, g)
        for nm in E_NAMES + ("eps", "element"):
            assert np.all(np.isfinite(a[nm])) and np.array_equal(a[nm], b[nm]), nm
        assert a["Ex"].shape == (len(modes), 33, 33) and a["eps"].shape == (33, 33)
        print(f"n_eff = {[round(float(m['n_eff']), 6) for m in modes]}")
        print(f"power = {q['power']}, core_fraction = {q['core_fraction']}, orthogonality.max() = {q['orthogonality'].max():.3e}")
    finally:
        mf.close()
