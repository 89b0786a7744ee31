"""Sampled index maps on the GPU (the map instances of k_element_matrices, k_profile_grams and k_mode_indicators) on the
sections of tests/map_cases.py: the assembled blocks of both pencils against the oracle with the same geometry, a map
outside the mesh and a cleared map against the layer-only path bit for bit, the modes of both solvers against the
oracle, independence of a cached context's and locator's history, the Gram and indicator kernels against their NumPy
emulations, the adaptive loop on a section without circles, and the argument checks of both new C entries on a live
context and locator."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from indicator_emulation import IndicatorEmulation
from map_cases import SquareMaps, layers_only_profile, m3, m3_index, m3l, outside_profile
from oracle import hfield, scalar
from oracle.compare import column_errors, mode_field_errors, stack_fields
from oracle.p2 import MeshTriLite
from pl_fem_vectoriel_amd import IndexProfile, ModeFields, ProfiledGeometry, _native, adaptive_solve, mode_error_indicators
from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver, _core_table
from profile_cases import three_core
from profile_gram_emulation import ProfileGramEmulation
from test_gpu_index_profile import EIG_TOL, KINDS, N_EFF_TOL, ORACLE_TOL, Section, _random_records, _same_records, _vals

pytestmark = pytest.mark.gpu
RECORD_KEYS = ("P_x", "P_y", "confinement", "core_overlap", "div_ratio", "PDL_dB")


def m3_small(base, n_clad=1.0) -> ProfiledGeometry:
    """The function of M3 on a coarser, smaller grid (17 x 13 over [-5, 7] x [-3, 6]): another map, in a smaller buffer."""
    x, y = np.linspace(-5.0, 7.0, 17), np.linspace(-3.0, 6.0, 13)
    X, Y = np.meshgrid(x, y)
    return ProfiledGeometry(base, IndexProfile(1.0).sampled(x, y, m3_index(X, Y)), n_clad=n_clad)


@pytest.fixture(scope="module")
def sections(gpu_device, built_library):
    g, mesh = three_core()
    sq = SquareMaps()
    out = {"M3": Section(g, m3(g), mesh), "M3L": Section(g, m3l(g), mesh)}
    for name in ("left", "left_out", "far", "two"):
        out[name] = Section(sq.base, sq.geometry(name), sq.mesh)
    out["square"] = sq
    return out


@pytest.mark.parametrize("name", ["M3", "M3L", "left", "far", "left_out", "two"])
def test_map_blocks_match_oracle(sections, name, gpu_device):
    """The test that pins the map at every quadrature point: a point on the wrong side of the extent's edge, in the
    wrong cell or with a swapped weight changes an entry by far more than the bars."""
    S = sections[name]
    sym = S.sym("vectorial")
    N, rowptr, colind = sym.N, sym.array("rowptr"), sym.array("colind")
    got = S.blocks("vectorial", S.pg, gpu_device)
    csr = lambda v: sp.csr_matrix((v, colind, rowptr), shape=(N, N))
    A, B, _, Dxx, Dyy, Dxy, Minv = hfield.assemble_hfield_system_fused(S.pg, S.om, eliminate_zeros=False)
    Ag = sp.bmat([[csr(got["Axx"]), csr(got["Axy"])], [csr(got["Ayx"]), csr(got["Ayy"])]], format="csr")
    ea, em = abs(Ag - A).max() / abs(A).max(), abs(csr(got["Minv"]) - Minv).max() / abs(Minv).max()
    print(f"{name} vectorial: A {ea:.1e} of max |A|, Minv {em:.1e} of max |Minv|")
    assert ea < 1e-12 and em < 1e-13
    for nm, R in (("Dxx", Dxx), ("Dyy", Dyy), ("Dxy", Dxy)):
        assert abs(csr(got[nm]) - R).max() < 1e-12 * abs(R).max(), nm
    sym = S.sym("scalar")
    N, rowptr, colind = sym.N, sym.array("rowptr"), sym.array("colind")
    got = S.blocks("scalar", S.pg, gpu_device)
    K, M, Me, _ = scalar.assemble(S.pg, S.om, eliminate_zeros=False)
    As = (K - S.pg.k0 ** 2 * Me).tocsr()
    ea, em = abs(csr(got["Axx"]) - As).max() / abs(As).max(), abs(csr(got["Minv"]) - M).max() / abs(M).max()
    print(f"{name} scalar: A {ea:.1e} of max |A|, M {em:.1e} of max |M|")
    assert ea <= 1e-12 and em <= 1e-13


def test_the_edge_variants_differ_where_the_target_point_weighs(sections, gpu_device):
    """x0 one ulp above the target's X puts that one point outside: the weighted block differs, the plain mass does not."""
    a, b = sections["left"].blocks("scalar", sections["left"].pg, gpu_device), sections["left_out"].blocks(
        "scalar", sections["left_out"].pg, gpu_device)
    assert not np.array_equal(a["Axx"], b["Axx"]) and np.array_equal(a["Minv"], b["Minv"])


@pytest.mark.parametrize("kind", KINDS)
def test_bit_identity_without_a_map(sections, kind, gpu_device):
    S = sections["M3L"]
    n_core = S.pg.n_core
    layers = ProfiledGeometry(S.g, layers_only_profile(), n_core=n_core)
    want = S.blocks(kind, layers, gpu_device)
    # a map wholly outside the mesh: the map instance, no point inside the extent
    got = S.blocks(kind, ProfiledGeometry(S.g, outside_profile(), n_core=n_core), gpu_device)
    for nm in _native.BLOCKS:
        assert np.array_equal(got[nm], want[nm]), nm
    # and without layers it is the homogeneous background
    bare = S.blocks(kind, ProfiledGeometry(S.g, outside_profile(layers=False), n_core=n_core), gpu_device)
    assert not np.array_equal(bare["Minv" if kind == "vectorial" else "Axx"], want["Minv" if kind == "vectorial" else "Axx"])
    # a layer-only profile after a map was set and cleared on the same context: the bits of a context that never saw one
    ctx = _native.Context(S.sym(kind), gpu_device, max_ncv=65)
    try:
        args = (_core_table(S.g), S.g.n_core ** 2, S.g.n_clad ** 2, S.g.k0)
        assemble = (lambda: ctx.assemble(*args, 1.0)) if kind == "vectorial" else (lambda: ctx.assemble_scalar(*args))
        ctx.set_index_profile(S.pg.index_profile)
        assemble()
        mapped = ctx.block_values("Axx")
        ctx.set_index_profile(layers.index_profile)
        assemble()
        for nm in _native.BLOCKS:
            assert np.array_equal(ctx.block_values(nm), want[nm]), nm
        assert not np.array_equal(mapped, want["Axx"])
        # and the step model after that
        ctx.set_index_profile(None)
        assemble()
        step = S.blocks(kind, S.g, gpu_device)
        for nm in _native.BLOCKS:
            assert np.array_equal(ctx.block_values(nm), step[nm]), nm
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def m3_clad(sections):
    """M3 at n_clad = 1.40: the reference's shift lands at n = 1.45."""
    S = sections["M3"]
    return Section(S.g, m3(S.g, 1.40), S.mesh)


@pytest.fixture(scope="module")
def m3_modes(m3_clad, gpu_device):
    S = m3_clad
    vsol = TrueVectorialMaxwellSolver(S.pg, device=gpu_device, eig_tol=EIG_TOL)
    ssol = ScalarHelmholtzSolver(S.pg, device=gpu_device, eig_tol=EIG_TOL)
    out = {"vectorial": vsol.solve_vectorial_modes(S.mesh, 10), "scalar": ssol.solve(S.mesh, 10),
           "vectorial_11": vsol.solve_vectorial_modes(S.mesh, 11)}
    vsol.clear_cache()
    ssol.clear_cache()
    return out


def test_map_modes_match_oracle(m3_clad, m3_modes):
    """Worst figures measured on the MI355X are in DESIGN section 26."""
    S = m3_clad
    modes = m3_modes["vectorial"]
    ref = hfield.solve_vectorial_modes(S.pg, S.om, n_modes_target=10, fused=True, tol=ORACLE_TOL)
    assert len(modes) == len(ref) == 22
    dn = max(abs(a["n_eff"] - b["n_eff"]) for a, b in zip(modes, ref))
    db = max(abs(a["beta"] - b["beta"]) for a, b in zip(modes, ref))
    # The 22nd record is one half of an exact pair of box modes whose other half the record count cuts off: alone it
    # has no defined field (the two solvers differ by 3.5e-5 there, n_eff agreeing to 1e-15).  The solves for one mode
    # more return that partner as their record 22, so the cluster-aware comparison sees the whole pair: the fields of
    # all 22 records are compared, the last one inside its complete cluster.
    more, more_ref = m3_modes["vectorial_11"], hfield.solve_vectorial_modes(S.pg, S.om, n_modes_target=11, fused=True, tol=ORACLE_TOL)
    assert len(more) == len(more_ref) >= 23
    assert all(abs(a["n_eff"] - b["n_eff"]) < 1e-12 for a, b in zip(more, modes))
    assert all(abs(a["n_eff"] - b["n_eff"]) < 1e-12 for a, b in zip(more_ref, ref))
    assert abs(more_ref[22]["n_eff"] - ref[21]["n_eff"]) < 1e-6 * ref[21]["n_eff"]          # the partner
    assert abs(more_ref[21]["n_eff"] - more_ref[20]["n_eff"]) > 1e-6 * ref[21]["n_eff"]     # and nothing else in the cluster
    pair = np.linalg.qr(np.stack([stack_fields(m) for m in more_ref[21:23]], axis=1))[0]
    last = stack_fields(modes[21]) / np.linalg.norm(stack_fields(modes[21]))
    out_of_pair = np.linalg.norm(last - pair @ (pair.T @ last))     # the 22nd record itself: inside the pair's eigenspace
    fes = np.concatenate([mode_field_errors(modes[:21], ref[:21]), [max(mode_field_errors(more[:23], more_ref[:23])[21], out_of_pair)]])
    fe = fes.max()
    print(f"vectorial: {len(modes)} records, max |dn_eff| {dn:.2e}, max |dbeta| {db:.2e}, field error {fe:.2e}")
    for i, (a, b) in enumerate(zip(modes, ref)):
        print(f"  record {i}: n_eff {b['n_eff']:.12f}, dn_eff {a['n_eff'] - b['n_eff']:+.1e}, field error {fes[i]:.1e}, "
              f"confinement {b['confinement']:.3f}")
    assert [m["n_eff"] for m in modes] == sorted((m["n_eff"] for m in modes), reverse=True)
    assert dn < N_EFF_TOL and db < 1e-9 and fe < 1e-6
    # record keys: only where the x / y split is defined, which an exact pair of box modes does not have
    # (the neighbours include the cut-off partner of the last record)
    ne = np.array([m["n_eff"] for m in more_ref[:23]])
    gap = np.full(len(ne), np.inf)
    gap[1:] = np.minimum(gap[1:], np.abs(np.diff(ne)))
    gap[:-1] = np.minimum(gap[:-1], np.abs(np.diff(ne)))
    isolated = (gap > 1e-6 * ne)[:22]
    confined = [i for i, m in enumerate(ref) if m["confinement"] > 0.5]
    assert len(confined) == 1 and isolated[confined[0]]
    worst = 0.0
    for i in np.flatnonzero(isolated):
        a, b = modes[i], ref[i]
        assert set(a) == set(b) and a["polarization"] == b["polarization"] and a["method"] == b["method"]
        for key in RECORD_KEYS:
            worst = max(worst, abs(a[key] - b[key]) / max(1.0, abs(b[key])))
            assert abs(a[key] - b[key]) <= 1e-6 * max(1.0, abs(b[key])), (i, key)
    print(f"vectorial: {int(isolated.sum())} isolated records (the confined one is record {confined[0]}), worst record key {worst:.2e}")

    modes = m3_modes["scalar"]
    ref = scalar.solve(S.pg, S.om, 10, tol=ORACLE_TOL)
    assert len(modes) == len(ref) == 13
    dn = max(abs(a["n_eff"] - b["n_eff"]) for a, b in zip(modes, ref))
    db = max(abs(a["beta"] - b["beta"]) for a, b in zip(modes, ref))
    V = np.stack([m["field_vector"] for m in modes], axis=1)
    U = np.stack([m["field_vector"] for m in ref], axis=1)
    fe = column_errors(V, U, np.array([m["n_eff"] for m in ref]), 1e-6).max()
    print(f"scalar: {len(modes)} records, max |dn_eff| {dn:.2e}, max |dbeta| {db:.2e}, field error {fe:.2e}")
    assert dn < N_EFF_TOL and db < 1e-9 and fe < 1e-6
    for a, b in zip(modes, ref):
        assert set(a) == set(b) and a["polarization"] == "scalar" and a["is_vectorial"] is False


@pytest.mark.parametrize("kind", KINDS)
def test_a_cached_context_carries_no_map_into_the_next_solve(sections, kind, gpu_device):
    S = sections["M3"]
    cls = ((lambda g: TrueVectorialMaxwellSolver(g, device=gpu_device, eig_tol=EIG_TOL)) if kind == "vectorial"
           else (lambda g: ScalarHelmholtzSolver(g, device=gpu_device)))
    solve = (lambda s: s.solve_vectorial_modes(S.mesh, 6)) if kind == "vectorial" else (lambda s: s.solve(S.mesh, 6))
    order = [m3(S.g, 1.40), S.g, m3l(S.g, 1.40), m3_small(S.g, 1.40), m3(S.g, 1.40)]   # ..., a smaller map after a larger one
    fresh = []
    for geo in order[:4]:
        s = cls(geo)
        fresh.append(solve(s))
        s.clear_cache()
    fresh.append(fresh[0])
    solver = cls(order[0])
    ctx = None
    for geo, want in zip(order, fresh):
        solver.geometry = geo
        _same_records(solve(solver), want)
        now = next(iter(solver._cache.values()))["ctx"]
        assert ctx is None or now is ctx
        ctx = now
    solver.clear_cache()
    assert any(a["n_eff"] != b["n_eff"] for a, b in zip(fresh[0], fresh[2]))
    assert any(a["n_eff"] != b["n_eff"] for a, b in zip(fresh[0], fresh[3]))


@pytest.fixture(scope="module")
def fields(sections, gpu_device):
    out = {"M3L": (ModeFields(sections["M3L"].mesh, device=gpu_device),
                   ProfileGramEmulation(sections["M3L"].mesh.p, sections["M3L"].mesh.t)),
           "far": (ModeFields(sections["far"].mesh, device=gpu_device),
                   ProfileGramEmulation(sections["far"].mesh.p, sections["far"].mesh.t))}
    yield out
    for mf, _ in out.values():
        mf.close()
    import torch
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k", [1, 33, 70])
@pytest.mark.parametrize("name", ["M3L", "far"])
def test_map_gram_kernel_matches_emulation(sections, fields, name, k):
    import torch
    S = sections[name]
    mf, em = fields[name]
    prof = S.pg.index_profile
    for kind in KINDS:
        modes = _random_records(kind, mf, k, seed=200 + k)
        G = mf.profile_grams(modes, S.pg)
        ref = em.profile_grams(_vals(modes), kind == "vectorial", prof)
        assert tuple(G) == tuple(ref)
        for nm in ref:
            err = np.abs(G[nm] - ref[nm]).max() / np.abs(ref[nm]).max()
            print(f"{name} {kind} k = {k} {nm}: {err:.2e} relative to max |G|")
            assert err <= 1e-12, nm
        again = mf.profile_grams(modes, S.pg)
        assert all(np.array_equal(G[nm], again[nm]) for nm in G)
        perm = np.random.default_rng(k).permutation(k)
        P = mf.profile_grams([modes[i] for i in perm], S.pg)
        assert all(np.array_equal(P[nm], G[nm][np.ix_(perm, perm)]) for nm in G)
        # a work buffer full of NaN: every partial block that is read is written first
        _, vals, _ = mf._check_records(modes)
        staged, _src = mf._stage(vals)
        need = ctypes.c_int64(0)
        assert mf._lib.plfem_profile_gram_work_bytes(vals.shape[0], k, ctypes.byref(need)) == _native.PLFEM_OK
        work = torch.full(((need.value + 256 + 7) // 8,), float("nan"), dtype=torch.float64, device=mf.tdev).view(torch.uint8)
        N = mf._profile_grams_staged(kind, staged, prof.table(), prof.eps_background, work=work, index_map=prof.index_map)
        assert all(np.array_equal(N[nm], G[nm]) for nm in G)


def test_rayleigh_defect_of_the_m3_records(m3_clad, m3_modes, fields):
    S = m3_clad
    mf, _ = fields["M3L"]                                            # the same mesh
    k0 = S.pg.k0
    for kind in KINDS:
        modes = m3_modes[kind]
        G = mf.profile_grams(modes, S.pg)
        beta = np.array([m["beta"] for m in modes])
        if kind == "vectorial":
            A, B, mu = G["K_w"] + G["D"] - k0 ** 2 * G["M"], G["M_w"], beta ** 2
        else:
            A, B, mu = G["S"] - k0 ** 2 * G["M_w"], G["M"], -beta ** 2
        defect = np.abs(np.diag(A) / np.diag(B) - mu) / np.abs(mu)
        print(f"{kind}: rayleigh defect max {defect.max():.2e} over {len(modes)} records")
        assert defect.max() <= 1e-10


def test_a_cached_locator_carries_no_map_into_the_next_call(sections, fields, gpu_device):
    S = sections["M3L"]
    mf, _ = fields["M3L"]
    geos = [m3(S.g), ProfiledGeometry(S.g, layers_only_profile(), n_core=1.54), m3l(S.g), m3_small(S.g), S.g]
    for kind in KINDS:
        modes = _random_records(kind, mf, 5, seed=7)
        for m, b in zip(modes, np.linspace(5.0, 6.0, 5)):
            m["beta"] = float(b)
        other = ModeFields(S.mesh, device=gpu_device)
        try:
            want = []
            for geo in geos:
                # a locator that saw nothing but this call
                one = ModeFields(S.mesh, device=gpu_device)
                want.append((one.profile_grams(modes, geo) if geo is not S.g else one.grams(modes, geo),
                             one.indicators(modes, geo)["eta2"]))
                one.close()
            for geo, (G, eta2) in zip(geos, want):
                got = other.profile_grams(modes, geo) if geo is not S.g else other.grams(modes, geo)
                assert all(np.array_equal(got[nm], G[nm]) for nm in G)
                assert np.array_equal(other.indicators(modes, geo)["eta2"], eta2)
            assert not np.array_equal(want[0][0]["M_w"], want[3][0]["M_w"]) and not np.array_equal(want[0][1], want[1][1])
        finally:
            other.close()


@pytest.mark.parametrize("name", ["M3L", "far", "left"])
def test_map_indicators_match_emulation(sections, name, gpu_device):
    S = sections[name]
    mf = ModeFields(S.mesh, device=gpu_device)
    emu = IndicatorEmulation(S.mesh.p, S.mesh.t)
    k0, alpha = S.pg.k0, 0.75
    try:
        for kind in KINDS:
            k = 5
            modes = _random_records(kind, mf, k, seed=31)
            rng = np.random.default_rng(32)
            beta = k0 * rng.uniform(1.2, 1.5, k)
            for m, b in zip(modes, beta):
                m["beta"] = float(b)
            got = mf.indicators(modes, S.pg, alpha_p=alpha)["eta2"]
            lam = beta * beta if kind == "vectorial" else -(beta * beta)
            want = emu.eta2(_vals(modes), kind == "vectorial", lam, k0, alpha, S.pg.index_profile.epsilon)
            err = np.abs(got - want).max() / np.abs(want).max()
            print(f"{name} {kind}: indicator error {err:.1e} of the largest output")
            assert got.shape == want.shape == (k, S.mesh.t.shape[1]) and np.all(np.isfinite(got)) and np.all(got > 0)
            assert err <= 1e-12
            assert np.array_equal(mf.indicators(modes, S.pg, alpha_p=alpha)["eta2"], got)
    finally:
        mf.close()


def test_adaptive_solve_on_a_section_without_circles(m3_clad, gpu_device):
    S = m3_clad
    solver = ScalarHelmholtzSolver(S.pg, device=gpu_device)
    modes, mesh, history = adaptive_solve(solver, S.mesh, 10, n_track=3, theta=0.3, max_dofs=200000, max_steps=3)
    solver.clear_cache()
    assert len(history) == 3 and history[0]["ne"] == 4055 < history[1]["ne"] < history[2]["ne"] and mesh is history[-1]["mesh"]
    for h in history:
        assert np.all(np.isfinite(h["totals"])) and np.all(h["totals"] > 0)
        print(f"adaptive: N = {h['N']}, ne = {h['ne']}, n_eff[:3] = {h['n_eff'][:3]}, totals = {h['totals']}")
    assert np.all(history[-1]["totals"] < history[0]["totals"])
    ref = scalar.solve(S.pg, MeshTriLite(mesh.p, mesh.t), 10, tol=ORACLE_TOL)
    dn = max(abs(a["n_eff"] - b["n_eff"]) for a, b in zip(modes, ref))
    print(f"adaptive: {len(modes)} records on {mesh.t.shape[1]} elements against the oracle on that mesh: max |dn_eff| {dn:.2e}")
    assert len(modes) == len(ref) > 0 and dn < N_EFF_TOL
    eta2, totals = mode_error_indicators(modes[:3], mesh, S.pg)
    assert np.array_equal(totals, history[-1]["totals"]) and eta2.shape == (3, mesh.t.shape[1])


def _bad_maps():
    E = np.full((5, 4), 2.0)
    with_value = lambda v: np.where(np.arange(20).reshape(5, 4) == 13, v, 2.0)
    bad = [(E, 1, 5), (E, 4, 1), (E, 0, 5), (E, 4, 0), (E, -4, 5), (E, 8193, 2), (E, 2, 8193), (E, 8192, 4096), (E, 0, 0),
           (None, 4, 5)]
    bad = [(e, nx, ny, 0.0, 0.0, 0.25, 0.25) for e, nx, ny in bad]
    bad += [(with_value(v), 4, 5, 0.0, 0.0, 0.25, 0.25) for v in (np.nan, np.inf, 0.0, -2.0)]
    bad += [(E, 4, 5, x0, y0, 0.25, 0.25) for x0, y0 in ((np.nan, 0.0), (0.0, np.inf), (-np.inf, 0.0), (0.0, np.nan))]
    bad += [(E, 4, 5, 0.0, 0.0, dx, dy) for dx, dy in ((0.0, 0.25), (0.25, 0.0), (-0.25, 0.25), (0.25, -0.25), (np.nan, 0.25),
                                                       (0.25, np.inf), (1e-320, 0.25), (0.25, 1e-320))]
    return E, bad


def test_map_argument_errors_on_a_live_context_and_locator(sections, gpu_device):
    S = sections["far"]
    lib = _native.load_library()
    good, bad = _bad_maps()
    ptr = lambda t: None if t is None else np.ascontiguousarray(t, dtype=np.float64).ctypes.data_as(ctypes.c_void_p)
    ctx = _native.Context(S.sym("scalar"), gpu_device, max_ncv=65)
    mf = ModeFields(S.mesh, device=gpu_device)
    mf._ensure_locator()
    modes = _random_records("scalar", mf, 3, seed=1)
    args = (_core_table(S.g), S.g.n_core ** 2, S.g.n_clad ** 2, S.g.k0)
    try:
        # the section's own map in force on both handles
        ctx.set_index_profile(S.pg.index_profile)
        ctx.assemble_scalar(*args)
        before = {nm: ctx.block_values(nm) for nm in ("Axx", "Minv")}
        G = mf.profile_grams(modes, S.pg)
        for case in bad:
            keep = ptr(case[0])
            assert lib.plfem_set_index_map(ctx._h, keep, *case[1:]) == _native.PLFEM_EINVAL, case[1:]
            assert b"plfem_set_index_map" in lib.plfem_last_error(ctx._h)
            assert lib.plfem_locator_set_index_map(mf._loc, keep, *case[1:]) == _native.PLFEM_EINVAL, case[1:]
            assert b"plfem_locator_set_index_map" in lib.plfem_locator_last_error(mf._loc)
        # every rejected call left both handles as they were
        ctx.assemble_scalar(*args)
        assert all(np.array_equal(ctx.block_values(nm), before[nm]) for nm in before)
        prof = S.pg.index_profile
        _, vals, _ = mf._check_records(modes)
        staged, _src = mf._stage(vals)
        need = ctypes.c_int64(0)
        assert lib.plfem_profile_gram_work_bytes(1, 3, ctypes.byref(need)) == _native.PLFEM_OK
        work = _native.device_scratch(need.value + 512, mf.tdev)
        out = np.zeros((3, 3, 3))
        table = prof.table()
        rc = lib.plfem_profile_grams(mf._loc, 1, 3, ctypes.c_void_p(staged.data_ptr()), 0, ptr(table), table.shape[0],
                                     prof.eps_background, ctypes.c_void_p((work.data_ptr() + 255) & ~255), ctypes.c_int64(need.value),
                                     out.ctypes.data_as(ctypes.c_void_p))
        assert rc == _native.PLFEM_OK and np.array_equal(out[1], G["M_w"])
        with pytest.raises(ValueError, match="plfem_set_index_map"):
            ctx.set_index_map((np.full((5, 4), -1.0), 0.0, 0.0, 0.25, 0.25))
        # a good map, then a clear (twice: nothing left to free), on both handles
        for entry, h in ((lib.plfem_set_index_map, ctx._h), (lib.plfem_locator_set_index_map, mf._loc)):
            assert entry(h, ptr(good), 4, 5, 0.0, 0.0, 0.25, 0.25) == _native.PLFEM_OK
            assert entry(h, None, 0, 0, np.nan, np.nan, np.nan, np.nan) == _native.PLFEM_OK       # clears: nothing else is read
            assert entry(h, None, 0, 0, 0.0, 0.0, 0.0, 0.0) == _native.PLFEM_OK
        # a map without layers needs a background: plfem_set_index_profile(ctx, NULL, 0, eps_bg) gives it
        assert lib.plfem_set_index_profile(ctx._h, None, 0, np.nan) == _native.PLFEM_OK
        assert lib.plfem_set_index_map(ctx._h, ptr(good), 4, 5, 0.0, 0.0, 0.25, 0.25) == _native.PLFEM_OK
        with pytest.raises(ValueError, match="background"):
            ctx.assemble_scalar(*args)
        assert lib.plfem_set_index_profile(ctx._h, None, 0, 2.0) == _native.PLFEM_OK
        ctx.assemble_scalar(_core_table(S.g), -1.0, 0.0, S.g.k0)          # eps_core / eps_clad are not read under a map
        homogeneous = ctx.block_values("Axx")                                # the map is 2.0 everywhere, as is the background
        ctx.set_index_profile(None)
        ctx.assemble_scalar(_core_table(S.g)[:0], 2.0, 2.0, S.g.k0)
        # (the interpolant of a constant carries the rounding of 1 - a and of three sums: a few ulps of 2.0)
        step = ctx.block_values("Axx")
        assert np.abs(homogeneous - step).max() <= 1e-14 * np.abs(step).max() and np.abs(step).max() > 0
    finally:
        mf.close()
        ctx.close()
