"""Tangent Grams of index profiles on the GPU (k_profile_point_weights, k_weighted_grams): the kernels against their NumPy
emulation on layers, graded cores, closed-rim ties and maps; identities with the existing Gram kernels; the bit
contract (repeats, permutations, subsets, work-buffer contents, column groups); the argument checks of the C ABI on a
live locator; and group index, index sensitivity and bend response of profile solves against the step-model entries
and against finite differences of GPU re-solves."""
import copy
import ctypes

import numpy as np
import pytest

from pl_fem_vectoriel_amd import (IndexProfile, ModeFields, ProfiledGeometry, _native, bend_response, core_decomposition,
                                  mode_dispersion, profile_bend_response, profile_dispersion, profile_sensitivity)
from pl_fem_vectoriel_amd.dispersion import _clusters
from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver
from map_cases import m3, m3l
from profile_cases import own_discs, p5, p5_profile, three_core, tie_square
from tangent_gram_emulation import TangentGramEmulation, moved_profile, random_tangent

pytestmark = pytest.mark.gpu
KINDS = ("vectorial", "scalar")
EIG_TOL = 1e-10
ORIGIN = (0.3, -0.2)


# ---- what the tests share --------------------------------------------------------------------------------------------
def whole_profile_tangent(prof):
    """The tangent d eps = eps: the profile itself, values and map."""
    m = prof.index_map
    return prof.tangent_eps(prof.eps_background, prof.table()[:, 4:6], None if m is None else m[0])


def nine_tangents(prof):
    """P5's nine: distinct dn per layer with centre != edge on the graded one, the graded layer alone, the background
    and the five layers one by one, and the profile itself -- more than two column groups."""
    dn = np.array([[0.010, 0.010], [-0.020, -0.020], [0.030, -0.015], [0.040, 0.040], [-0.050, -0.050]])
    graded = np.zeros((5, 2))
    graded[2] = (0.02, 0.05)
    return [prof.tangent_index(0.005, dn), prof.tangent_index(dn_layers=graded)] + prof.unit_tangents() + [whole_profile_tangent(prof)]


def case_tangents(name, prof):
    if name == "p5":
        t = nine_tangents(prof)
        assert len(t) == 9
        return t
    if name == "square":
        return [random_tangent(prof, seed=21), whole_profile_tangent(prof)] + prof.unit_tangents()[-3:]
    if name == "m3":                                                     # a map only, with a tangent map
        return [random_tangent(prof, seed=22), whole_profile_tangent(prof)]
    return [random_tangent(prof, seed=23), random_tangent(prof, seed=24, with_map=False), whole_profile_tangent(prof)]


def _random_records(kind, mf, k, seed):
    rng = np.random.default_rng(seed)
    if kind == "vectorial":
        return [{"Ex_dofs": rng.standard_normal(mf.nsolve), "Ey_dofs": rng.standard_normal(mf.nsolve)} for _ in range(k)]
    return [{"field_vector": rng.standard_normal(mf.N)} for _ in range(k)]


def _vals(modes):
    if "Ex_dofs" in modes[0]:
        return np.stack([np.array([m["Ex_dofs"] for m in modes]), np.array([m["Ey_dofs"] for m in modes])])
    return np.array([m["field_vector"] for m in modes])[None]


@pytest.fixture(scope="module")
def sections(gpu_device, built_library):
    g, mesh = three_core()
    _, gt, pgt, mesht = tie_square()
    return {"p5": (g, p5(g), mesh), "m3": (g, m3(g), mesh), "m3l": (g, m3l(g), mesh), "own": (g, own_discs(g), mesh),
            "square": (gt, pgt, mesht)}


@pytest.fixture(scope="module")
def fields(sections, gpu_device):
    three = (ModeFields(sections["p5"][2], device=gpu_device), TangentGramEmulation(sections["p5"][2].p, sections["p5"][2].t))
    square = (ModeFields(sections["square"][2], device=gpu_device),
              TangentGramEmulation(sections["square"][2].p, sections["square"][2].t))
    out = {"p5": three, "m3": three, "m3l": three, "own": three, "square": square}
    yield out
    three[0].close()
    square[0].close()
    import torch
    torch.cuda.empty_cache()


# ---- the kernels against the emulation -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 33, 70])
@pytest.mark.parametrize("name", ["p5", "square", "m3", "m3l"])
def test_tangent_gram_kernels_match_emulation(sections, fields, name, k):
    _, pg, _ = sections[name]
    mf, em = fields[name]
    prof = pg.index_profile
    tans = case_tangents(name, prof)
    for kind in KINDS:
        modes = _random_records(kind, mf, k, seed=200 + k)
        G = mf.profile_tangent_grams(modes, pg, tans, moments=True, origin=ORIGIN)
        ref = em.named(em.tangent_grams(_vals(modes), kind == "vectorial", prof, tans, True, ORIGIN), len(tans), True)
        assert set(G) == set(ref) == {n + s for n in (("M", "K") if kind == "vectorial" else ("M",)) for s in ("_d", "_wX", "_wY")}
        for nm in ref:
            assert G[nm].shape == ref[nm].shape == ((len(tans), k, k) if nm.endswith("_d") else (k, k))
            err = np.abs(G[nm] - ref[nm]).max() / np.abs(ref[nm]).max()
            print(f"{name} {kind} k = {k} {nm}: {err:.2e} relative to max |G|")
            assert err <= 1e-12, nm
            if nm.endswith("_d"):                                        # and per column: a small column hides behind no large one
                for c in range(len(tans)):
                    assert np.abs(G[nm][c] - ref[nm][c]).max() <= 1e-12 * np.abs(ref[nm][c]).max(), (nm, c)


# ---- identities with the existing kernels ----------------------------------------------------------------------------
def _close(a, b, scale=None):
    return np.abs(a - b).max() <= 1e-12 * (np.abs(b).max() if scale is None else scale)


@pytest.mark.parametrize("name", ["p5", "m3l"])
def test_the_profile_as_its_own_tangent_gives_the_profile_grams(sections, fields, name):
    _, pg, _ = sections[name]
    mf, _ = fields[name]
    t = whole_profile_tangent(pg.index_profile)
    for kind in KINDS:
        modes = _random_records(kind, mf, 33, seed=5)
        G, T = mf.profile_grams(modes, pg), mf.profile_tangent_grams(modes, pg, [t])
        if kind == "scalar":
            assert _close(T["M_d"][0], G["M_w"])
        else:                                                            # dw = -eps / eps^2 = -w
            assert _close(T["M_d"][0], -G["M_w"]) and _close(T["K_d"][0], -G["K_w"])


def test_step_model_tangents_give_the_region_and_moment_grams(sections, fields):
    g, pg, _ = sections["own"]
    mf, _ = fields["own"]
    prof = pg.index_profile
    ec, el = g.n_core ** 2, g.n_clad ** 2
    tans = [prof.tangent_eps(0.0, 1.0), prof.tangent_eps(1.0, 0.0)]       # d eps = 1 on the discs, on the background
    for kind in KINDS:
        modes = _random_records(kind, mf, 33, seed=6)
        G, P = mf.grams(modes, g), mf.moment_grams(modes, g, origin=ORIGIN)
        T = mf.profile_tangent_grams(modes, pg, tans, moments=True, origin=ORIGIN)
        if kind == "scalar":
            assert _close(T["M_d"][0], G["M_core"]) and _close(T["M_d"][1], G["M_clad"])
            for a in "XY":
                assert _close(T["M_w" + a], ec * P["M_core_" + a] + el * P["M_clad_" + a])
        else:
            assert _close(T["M_d"][0], -G["M_core"] / ec ** 2) and _close(T["M_d"][1], -G["M_clad"] / el ** 2)
            assert _close(T["K_d"][0], -G["K_core"] / ec ** 2) and _close(T["K_d"][1], -G["K_clad"] / el ** 2)
            for a in "XY":
                assert _close(T["M_w" + a], P["M_core_" + a] / ec + P["M_clad_" + a] / el)
                assert _close(T["K_w" + a], P["K_core_" + a] / ec + P["K_clad_" + a] / el)


@pytest.fixture(scope="module")
def plain_modes(sections, gpu_device):
    """Solver modes of the plain three-core geometry (the step model), both kinds."""
    g, _, mesh = sections["own"]
    vsol = TrueVectorialMaxwellSolver(g, device=gpu_device, eig_tol=EIG_TOL)
    ssol = ScalarHelmholtzSolver(g, device=gpu_device, eig_tol=EIG_TOL)
    out = {"vectorial": vsol.solve_vectorial_modes(mesh, 10), "scalar": ssol.solve(mesh, 10)}
    vsol.clear_cache()
    ssol.clear_cache()
    return out


def test_profile_response_agrees_with_the_step_model_entries(sections, fields, plain_modes):
    g, pg, _ = sections["own"]
    mf, _ = fields["own"]
    prof = pg.index_profile
    dn = (-0.012, -0.017)                                                # dn/dlambda of core and cladding, um^-1
    for kind in KINDS:
        modes = plain_modes[kind]
        a = mode_dispersion(modes, mf, g, dn_dlambda=dn)
        b = profile_dispersion(modes, mf, pg, dn_dlambda=prof.tangent_index(dn[1], dn[0]))
        e_ng = np.abs(a["n_g"] - b["n_g"]).max()
        assert set(a) - {"grams"} <= set(b) and np.array_equal(a["cluster"], b["cluster"])
        c = core_decomposition(modes, mf, g, direction=[1.0, -0.5, 0.25])
        d = profile_sensitivity(modes, mf, pg, direction=[0.0, 1.0, -0.5, 0.25])
        assert d["dneff_dp"].shape == (len(modes), 4) and d["sensitivity"].shape == (4, len(modes), len(modes))
        e_dn = max(np.abs(c["dneff_dn"] - d["dneff_dp"][:, 1:]).max(), np.abs(c["dneff_direction"] - d["dneff_direction"]).max())
        e = bend_response(modes, mf, g, radius=[4000.0, -9000.0], angle=0.7, origin=ORIGIN)
        f = profile_bend_response(modes, mf, pg, radius=[4000.0, -9000.0], angle=0.7, origin=ORIGIN)
        assert set(e) - {"grams", "moment_grams"} <= set(f)
        e_dk = np.abs(e["dneff_dkappa"] - f["dneff_dkappa"]).max()
        e_c = max(np.abs(e["centroid"] - f["centroid"]).max(), np.abs(e["width_d4sigma"] - f["width_d4sigma"]).max())
        e_r = np.nanmax(np.abs(e["n_eff_ritz"] - f["n_eff_ritz"]))
        defect = max(r["rayleigh_defect"].max() for r in (b, d, f))
        print(f"{kind}: n_g {e_ng:.1e}, dn_eff/dn {e_dn:.1e}, dn_eff/dkappa {e_dk:.1e}, centroid / width {e_c:.1e}, "
              f"n_eff_ritz {e_r:.1e}, rayleigh defect {defect:.1e}")
        assert e_ng <= 1e-9 and e_dn <= 1e-9 and e_dk <= 1e-9 and e_c <= 1e-9 and e_r <= 1e-9 and defect <= 1e-10


# ---- bits ------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(a[nm], b[nm]) for nm in a)


def test_repeats_permutations_subsets_work_contents_and_column_groups_give_the_same_bits(sections, fields):
    import torch
    _, pg, _ = sections["p5"]
    mf, _ = fields["p5"]
    prof = pg.index_profile
    tans = nine_tangents(prof)
    k = 33
    for kind in KINDS:
        modes = _random_records(kind, mf, k, seed=7)
        G = mf.profile_tangent_grams(modes, pg, tans, moments=True, origin=ORIGIN)
        assert _same(G, mf.profile_tangent_grams(modes, pg, tans, moments=True, origin=ORIGIN))
        perm = np.random.default_rng(k).permutation(k)
        P = mf.profile_tangent_grams([modes[i] for i in perm], pg, tans, moments=True, origin=ORIGIN)
        assert _same(P, {nm: v[..., perm[:, None], perm[None, :]] for nm, v in G.items()})
        S = mf.profile_tangent_grams(modes[:20], pg, tans, moments=True, origin=ORIGIN)      # one chunk instead of two
        assert _same(S, {nm: v[..., :20, :20] for nm, v in G.items()})
        # a work buffer full of NaN: every partial block and every point weight that is read is written first
        _, vals, _ = mf._check_records(modes)
        staged, _src = mf._stage(vals)
        need = ctypes.c_int64(0)
        assert mf._lib.plfem_profile_tangent_gram_work_bytes(mf._loc, vals.shape[0], k, len(tans), 0, 1,
                                                             ctypes.byref(need)) == _native.PLFEM_OK
        work = torch.full(((need.value + 256 + 7) // 8,), float("nan"), dtype=torch.float64, device=mf.tdev).view(torch.uint8)
        assert _same(G, mf._profile_tangent_grams_staged(kind, staged, prof, tans, True, np.array(ORIGIN), work=work))
        # a column's bits depend neither on the other columns of the call nor on its group: alone, without the moments,
        # and in another order
        for c in (0, 5, 8):
            alone = mf.profile_tangent_grams(modes, pg, [tans[c]])
            assert all(np.array_equal(alone[nm][0], G[nm][c]) for nm in alone), c
        back = mf.profile_tangent_grams(modes, pg, tans[::-1][:7])
        assert all(np.array_equal(back[nm], G[nm][::-1][:7]) for nm in back)
        mom = mf.profile_tangent_grams(modes, pg, (), moments=True, origin=ORIGIN)
        assert set(mom) == set(G) and mom["M_d"].shape == (0, k, k)
        assert all(np.array_equal(mom[nm], G[nm]) for nm in mom if not nm.endswith("_d"))


def test_more_tangent_maps_than_one_call_takes(sections, fields):
    _, pg, _ = sections["m3l"]
    mf, _ = fields["m3l"]
    prof = pg.index_profile
    tans = [random_tangent(prof, seed=30 + i, with_map=(i % 4 != 3)) for i in range(13)]     # ten maps: two calls
    modes = _random_records("scalar", mf, 5, seed=8)
    G = mf.profile_tangent_grams(modes, pg, tans, moments=True, origin=ORIGIN)
    for c in (0, 3, 9, 12):
        alone = mf.profile_tangent_grams(modes, pg, [tans[c]])
        assert np.array_equal(alone["M_d"][0], G["M_d"][c]), c
    mom = mf.profile_tangent_grams(modes, pg, (), moments=True, origin=ORIGIN)
    assert np.array_equal(mom["M_wX"], G["M_wX"]) and np.array_equal(mom["M_wY"], G["M_wY"])
    # a later call on a geometry without a map: the locator's map is cleared, and tangent maps are refused by the library
    _, p5g, _ = sections["p5"]
    assert mf.profile_tangent_grams(modes, p5g, p5g.index_profile.unit_tangents()[:1])["M_d"].shape == (1, 5, 5)
    need = ctypes.c_int64(0)
    assert mf._lib.plfem_profile_tangent_gram_work_bytes(mf._loc, 1, 5, 1, 1, 0, ctypes.byref(need)) == _native.PLFEM_EINVAL


# ---- the C ABI on a live locator -------------------------------------------------------------------------------------
def test_tangent_argument_errors_on_a_live_locator(sections, fields):
    _, pg, mesh = sections["m3l"]
    mf, em = fields["m3l"]
    lib = _native.load_library()
    prof = pg.index_profile
    mf._ensure_locator()
    mf._set_index_map(prof.index_map)
    modes = _random_records("vectorial", mf, 3, seed=1)
    _, vals, _ = mf._check_records(modes)
    staged, _src = mf._stage(vals)
    E = prof.index_map[0]
    ny, nx = E.shape
    table = prof.table()
    rows = np.ascontiguousarray(np.stack([t.row() for t in prof.unit_tangents()]))           # (3, 5)
    maps = np.ascontiguousarray(np.stack([0.1 * E, 0.2 * E]))
    which = np.array([0, -1, 1], dtype=np.int32)
    origin = np.array(ORIGIN)
    need = ctypes.c_int64(0)
    size = lambda ncomp, k, ntan, nmap, mom, out=need: lib.plfem_profile_tangent_gram_work_bytes(mf._loc, ncomp, k, ntan, nmap, mom,
                                                                                                  None if out is None else ctypes.byref(out))
    # the documented layout and its bound
    for ncomp, nout in ((1, 1), (2, 2)):
        for k, ntan, nmap, mom in ((1, 1, 0, 0), (22, 9, 0, 1), (33, 0, 0, 1), (70, 256, 8, 1), (32, 3, 2, 0)):
            assert size(ncomp, k, ntan, nmap, mom) == _native.PLFEM_OK
            nc, ncol, a = (k + 31) // 32, ntan + 2 * mom, lambda b: (b + 255) // 256 * 256
            want = (a(8 * ncol * nout * k * k) + a(8 * 4 * nout * nc * nc * 768 * 1024) + a(8 * 4 * 6 * mf.ne) + a(8 * max(1, ntan) * 129) +
                    a(4 * max(1, ntan)) + a(8 * max(1, nmap * nx * ny)))
            assert need.value == want
            assert want <= 8 * (ncol * nout * k * k + 4 * nout * nc * nc * 786432 + 24 * mf.ne + 129 * max(1, ntan) + max(1, nmap * nx * ny)) \
                + 4 * max(1, ntan) + 6 * 256
    keep = ctypes.c_int64(-7)
    for bad in ((0, 3, 3, 2, 1), (3, 3, 3, 2, 1), (2, 0, 3, 2, 1), (2, 3, -1, 0, 1), (2, 3, 257, 0, 1), (2, 3, 0, 0, 0), (2, 3, 3, 4, 1),
                (2, 3, 3, -1, 1), (2, 3, 9, 9, 1)):
        assert size(*bad, out=keep) == _native.PLFEM_EINVAL and keep.value == -7, bad
    assert size(2, 3, 3, 2, 1, out=None) == _native.PLFEM_EINVAL
    assert size(2, 3, 3, 2, 1) == _native.PLFEM_OK
    work = _native.device_scratch(need.value + 512, mf.tdev)
    wp = (work.data_ptr() + 255) & ~255
    out = np.zeros((5, 2, 3, 3))
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def call(ncomp=2, k=3, modes_ptr=staged.data_ptr(), t=table, nlayer=2, bg=1.0, r=rows, ntan=3, m=maps, nmap=2, w_=which, mom=1,
             o=origin, w=wp, wb=None, res=out):
        return lib.plfem_profile_tangent_grams(mf._loc, ncomp, k, ctypes.c_void_p(modes_ptr), 1, ptr(t), nlayer, bg, ptr(r), ntan, ptr(m),
                                               nmap, ptr(w_), mom, ptr(o), ctypes.c_void_p(w), ctypes.c_int64(need.value if wb is None else wb),
                                               ptr(res))

    def with_entry(a, idx, v):
        b = a.copy()
        b[idx] = v
        return b

    bad_table = with_entry(table, (0, 3), -1.0)
    rejected = [dict(ncomp=0), dict(ncomp=3), dict(k=0), dict(ntan=-1), dict(ntan=257), dict(ntan=0, nmap=0, mom=0), dict(nmap=-1),
                dict(nmap=4), dict(ntan=9, nmap=9), dict(t=bad_table), dict(nlayer=65), dict(nlayer=-1), dict(bg=0.0), dict(bg=np.nan),
                dict(t=None), dict(modes_ptr=0), dict(r=None), dict(m=None), dict(w_=None), dict(o=None), dict(w=0), dict(res=None),
                dict(w_=with_entry(which, 0, 2)), dict(w_=with_entry(which, 2, -2)), dict(r=with_entry(rows, (1, 2), np.nan)),
                dict(r=with_entry(rows, (0, 0), np.inf)), dict(m=with_entry(maps, (1, 0, 0), np.nan)), dict(o=np.array([np.inf, 0.0])),
                dict(o=np.array([0.0, np.nan])), dict(wb=need.value - 1), dict(w=wp + 8)]
    for kw in rejected:
        assert call(**kw) == _native.PLFEM_EINVAL, kw
        assert lib.plfem_locator_last_error(mf._loc).startswith(b"plfem_profile_tangent_grams: "), kw
    assert not out.any()
    assert call() == _native.PLFEM_OK and out.any()
    # the accepted call is the emulation's: tangent 0 with map 0, tangent 1 without, tangent 2 with map 1
    unit = prof.unit_tangents()
    tans = [prof.tangent_eps(unit[0].d_eps_background, unit[0].d_layers, maps[0]), unit[1],
            prof.tangent_eps(unit[2].d_eps_background, unit[2].d_layers, maps[1])]
    ref = em.tangent_grams(vals, True, prof, tans, True, ORIGIN)
    assert all(np.abs(out[c, o] - ref[c, o]).max() <= 1e-12 * np.abs(ref[c, o]).max() for c in range(5) for o in range(2))
    # no maps and a null index array; and tangent maps without a map on the locator are refused
    assert call(m=None, nmap=0, w_=None) == _native.PLFEM_OK
    mf._set_index_map(None)
    assert size(2, 3, 3, 2, 1, out=keep) == _native.PLFEM_EINVAL and keep.value == -7
    assert call() == _native.PLFEM_EINVAL and b"map on the locator" in lib.plfem_locator_last_error(mf._loc)
    assert call(m=None, nmap=0, w_=None) == _native.PLFEM_OK


# ---- physics: finite differences of GPU re-solves --------------------------------------------------------------------
def _unit_rows(modes):
    x = _vals(modes).transpose(1, 0, 2).reshape(len(modes), -1)
    return x / np.linalg.norm(x, axis=1)[:, None]


def _mu(kind, modes):
    b = np.array([m["beta"] for m in modes])
    return b ** 2 if kind == "vectorial" else -b ** 2


def _groups(label):
    """The clusters and singletons of ``label`` as index arrays, in record order of their first member."""
    seen, out = set(), []
    for i, c in enumerate(label):
        if c < 0:
            out.append(np.array([i]))
        elif c not in seen:
            seen.add(c)
            out.append(np.nonzero(label == c)[0])
    return out


def group_means(kind, modes, label, values, resolves, fd):
    """Means over the groups of ``label`` of ``values`` (k,) and of the finite difference ``fd(records+, records-)`` of the
    group's records in the two re-solves, for the groups that can be compared.

    A group is matched to a group of the same size of each re-solve -- the re-solve's own clusters under the same
    tolerance -- by subspace overlap: every member's projection on the span of the matched group has norm above 0.999.
    The group that the end of a mode list may have cut is left out, and so is a group whose gap to its nearest neighbour
    moved by more than 1 % of the gap in either re-solve.  Returns ``[(group, mean value, mean fd)]``."""
    X, mu = _unit_rows(modes), _mu(kind, modes)
    tol = 1e-6
    groups = _groups(label)
    last = len(modes) - 1
    matched = {}
    for side, other in enumerate(resolves):
        Y, muo = _unit_rows(other), _mu(kind, other)
        og = [h for h in _groups(_clusters(muo, tol * float(np.abs(muo).max()))) if len(other) - 1 not in h]
        for gi, G in enumerate(groups):
            if last in G:
                continue
            for H in og:
                if len(H) != len(G):
                    continue
                Q, _ = np.linalg.qr(Y[H].T)
                if np.all(np.linalg.norm(X[G] @ Q, axis=1) > 0.999):
                    matched.setdefault(gi, {})[side] = H
                    break
    both = [gi for gi in matched if len(matched[gi]) == 2]
    mean = {gi: float(mu[groups[gi]].mean()) for gi in both}
    out = []
    for gi in both:
        others = [gj for gj in both if gj != gi]
        if not others:
            continue
        gj = min(others, key=lambda j: abs(mean[j] - mean[gi]))
        gap = mean[gi] - mean[gj]
        moved = 0.0
        for side, other in enumerate(resolves):
            muo = _mu(kind, other)
            moved = max(moved, abs((muo[matched[gi][side]].mean() - muo[matched[gj][side]].mean()) - gap))
        if moved > 0.01 * abs(gap):
            continue
        G = groups[gi]
        plus, minus = ([resolves[s][int(i)] for i in matched[gi][s]] for s in (0, 1))
        out.append((G, float(np.mean(values[G])), float(fd(plus, minus))))
    return out


class Solvers:
    """Both solvers on one mesh, re-aimed at other geometries of the same mesh (analysis and context are reused)."""

    def __init__(self, geometry, mesh, device, n_modes=10):
        self.mesh, self.n_modes = mesh, n_modes
        self.sol = {"vectorial": TrueVectorialMaxwellSolver(geometry, device=device, eig_tol=EIG_TOL),
                    "scalar": ScalarHelmholtzSolver(geometry, device=device, eig_tol=EIG_TOL)}

    def solve(self, kind, geometry):
        s = self.sol[kind]
        s.geometry, s.k0 = geometry, geometry.k0
        return s.solve_vectorial_modes(self.mesh, self.n_modes) if kind == "vectorial" else s.solve(self.mesh, self.n_modes)

    def close(self):
        for s in self.sol.values():
            s.clear_cache()


def at_k0(geometry, profile, s):
    """``geometry`` at k0 s with ``profile``."""
    g = copy.copy(ProfiledGeometry(geometry, profile, n_core=geometry.n_core, n_clad=geometry.n_clad))
    g.k0, g.wavelength = geometry.k0 * s, geometry.wavelength / s
    return g


def p5_with(layer, dn):
    """P5 with the index of ``layer`` (2: the graded core, centre and edge; 4: the last step core) moved by ``dn``."""
    d = [dn if l == layer else 0.0 for l in range(5)]
    return (IndexProfile(1.0).disc((0.8, 1.4), 9.0, 1.45 + d[0]).ring((5.0, 0.0), 1.3, 2.2, 1.40 + d[1])
            .graded((0.0, 0.0), 1.5, 1.535 + d[2], 1.50 + d[2], 2).disc((5.0, 0.0), 1.3, 1.530 + d[3]).disc((-2.5, 4.33), 1.1, 1.540 + d[4]))


DN_DLAMBDA = dict(dn_background=0.0, dn_layers=[[-0.0120, -0.0120], [-0.0135, -0.0135], [-0.0110, -0.0150], [-0.0125, -0.0125],
                                               [-0.0140, -0.0140]])
DELTA = 1e-5


@pytest.fixture(scope="module")
def p5_solves(sections, gpu_device):
    g, pg, mesh = sections["p5"]
    assert np.array_equal(p5_with(None, 0.0).table(), p5_profile().table())
    S = Solvers(pg, mesh, gpu_device)
    prof = pg.index_profile
    deps_dk0 = prof.tangent_index(**DN_DLAMBDA).scaled(-(2.0 * np.pi / pg.k0) / pg.k0)
    out = {}
    for kind in KINDS:
        out[kind] = {"base": S.solve(kind, pg)}
        out[kind]["k0"] = [S.solve(kind, at_k0(pg, moved_profile(prof, deps_dk0, eps_of=lambda e, d, s=s: e + (s * DELTA * pg.k0) * d), 1 + s * DELTA))
                           for s in (1, -1)]
        for layer in (2, 4):
            out[kind][layer] = [S.solve(kind, at_k0(pg, p5_with(layer, s * DELTA), 1.0)) for s in (1, -1)]
    S.close()
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_group_index_and_sensitivity_of_p5_against_finite_differences_of_gpu_solves(sections, fields, p5_solves, kind):
    """Measured on an MI355X (worst group, vectorial / scalar): see DESIGN.md section 30."""
    _, pg, _ = sections["p5"]
    mf, _ = fields["p5"]
    prof = pg.index_profile
    modes = p5_solves[kind]["base"]
    res = profile_dispersion(modes, mf, pg, dn_dlambda=prof.tangent_index(**DN_DLAMBDA), cluster_rtol=1e-6)
    h = 2 * DELTA * pg.k0
    rows = group_means(kind, modes, res["cluster"], res["n_g"], p5_solves[kind]["k0"],
                       lambda p, m: np.mean([(a["beta"] - b["beta"]) / h for a, b in zip(p, m)]))
    worst = max(abs(v - f) for _, v, f in rows)
    print(f"{kind}: n_g of {len(rows)} groups of {len(modes)} records, worst |HF - FD| = {worst:.2e}; "
          f"rayleigh defect {res['rayleigh_defect'].max():.1e}")
    assert len(rows) >= 3 and worst <= 1e-6 and res["rayleigh_defect"].max() <= 1e-10
    sens = profile_sensitivity(modes, mf, pg, cluster_rtol=1e-6)
    assert sens["rayleigh_defect"].max() <= 1e-10
    for layer in (2, 4):
        rows = group_means(kind, modes, sens["cluster"], sens["dneff_dp"][:, layer + 1], p5_solves[kind][layer],
                           lambda p, m: np.mean([(a["n_eff"] - b["n_eff"]) / (2 * DELTA) for a, b in zip(p, m)]))
        worst = max(abs(v - f) for _, v, f in rows)
        big = max(abs(f) for _, _, f in rows)
        print(f"{kind}: dn_eff/dn of layer {layer + 1}, {len(rows)} groups, worst |HF - FD| = {worst:.2e} (largest {big:.3f})")
        assert len(rows) >= 3 and worst <= 1e-6
    bend = profile_bend_response(modes, mf, pg, radius=20000.0, angle=0.3, origin=ORIGIN, cluster_rtol=1e-6)
    assert bend["rayleigh_defect"].max() <= 1e-10 and np.all(np.isfinite(bend["dneff_dkappa"]))
