"""Pixel gradients of sampled index maps on the GPU (k_map_point_keys, the sort, k_map_cell_ranges, k_point_densities,
k_map_gather): the kernels against their NumPy emulation on one-cell maps, boundary ties, the clamped cell, layers over
the map and a map far finer than the mesh; the identity with the tangent-Gram kernel; a map outside the mesh; the bit
contract (repeats, permutations, subsets, work-buffer contents, chunks of fields); the argument checks of the C ABI on a
live locator; and the gradient of n_eff against finite differences of GPU re-solves."""
import ctypes

import numpy as np
import pytest

from pl_fem_vectoriel_amd import (IndexProfile, ModeFields, ProfiledGeometry, _native, index_map_gradient,
                                  profile_sensitivity)
from map_cases import M3_X, M3_Y, SQUARE_BG, SquareMaps, m3, m3_index, m3l, outside_profile
from map_gradient_emulation import MapGradientEmulation
from profile_cases import three_core
from test_gpu_profile_tangent import Solvers, _random_records, _vals, at_k0, group_means

pytestmark = pytest.mark.gpu
KINDS = ("vectorial", "scalar")
DELTA = 1e-5


# ---- what the tests share --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sections(gpu_device, built_library):
    """name -> (profiled geometry, mesh name)."""
    g, mesh = three_core()
    sq = SquareMaps()
    out = {"m3": (m3(g), "three"), "m3l": (m3l(g), "three")}
    for nm in ("two", "left", "left_out", "far"):
        out[nm] = (sq.geometry(nm), "square")
    # a map far finer than the mesh: 257 x 193 random indices over the square; nearly every node sees no point
    rng = np.random.default_rng(19)
    fine = sq._paint(IndexProfile(SQUARE_BG).sampled(np.linspace(-0.05, 1.05, 257), np.linspace(0.1, 0.95, 193),
                                                      rng.uniform(1.25, 1.5, (193, 257))))
    out["fine"] = (ProfiledGeometry(sq.base, fine, n_core=1.535, n_clad=SQUARE_BG), "square")
    out["_mesh"] = {"three": mesh, "square": sq.mesh}
    return out


@pytest.fixture(scope="module")
def fields(sections, gpu_device):
    out = {nm: (ModeFields(mesh, device=gpu_device), MapGradientEmulation(mesh.p, mesh.t)) for nm, mesh in sections["_mesh"].items()}
    yield out
    for mf, _ in out.values():
        mf.close()
    import torch
    torch.cuda.empty_cache()


def _of(sections, fields, name):
    pg, which = sections[name]
    return (pg,) + fields[which]


def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(a[nm], b[nm]) for nm in a)


# ---- the kernels against the emulation -------------------------------------------------------------------------------
CASES = [(name, k) for name in ("two", "left", "left_out", "far", "m3", "m3l") for k in (1, 17, 33, 70)] + [("fine", 1)]


@pytest.mark.parametrize("name,k", CASES)
def test_map_gradient_kernels_match_emulation(sections, fields, name, k):
    pg, mf, em = _of(sections, fields, name)
    prof = pg.index_profile
    ny, nx = prof.index_map[0].shape
    for kind in KINDS:
        modes = _random_records(kind, mf, k, seed=300 + k)
        G = mf.index_map_densities(modes, pg)
        ref = em.named(*em.map_gradients(_vals(modes), kind == "vectorial", prof))
        assert tuple(G) == tuple(ref) == (("M_px", "K_px", "support") if kind == "vectorial" else ("M_px", "support"))
        assert G["support"].dtype == np.int32 and np.array_equal(G["support"], ref["support"])
        if name == "fine":
            assert (ref["support"] == 0).mean() > 0.9
        for nm in ref:
            if nm == "support":
                continue
            assert G[nm].shape == ref[nm].shape == (k, ny, nx)
            worst = 0.0
            for r in range(k):
                top = np.abs(ref[nm][r]).max()
                assert top > 0
                worst = max(worst, np.abs(G[nm][r] - ref[nm][r]).max() / top)
            print(f"{name} {kind} k = {k} {nm}: {worst:.2e} relative to each plane's max")
            assert worst <= 1e-12, nm
            assert np.all(G[nm][:, ref["support"] == 0] == 0.0)


# ---- the identity with the tangent-Gram kernel -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m3", "m3l", "far"])
def test_contraction_with_a_tangent_map_is_the_tangent_gram_diagonal(sections, fields, name):
    pg, mf, _ = _of(sections, fields, name)
    prof = pg.index_profile
    k = 5
    for kind in KINDS:
        modes = _random_records(kind, mf, k, seed=9)
        G = mf.index_map_densities(modes, pg)
        for seed in (1, 2):
            D = np.random.default_rng(seed).uniform(-1.0, 1.0, prof.index_map[0].shape)
            T = mf.profile_tangent_grams(modes, pg, [prof.tangent_eps(0.0, 0.0, D)])
            for px, td in (("M_px", "M_d"), ("K_px", "K_d")) if kind == "vectorial" else (("M_px", "M_d"),):
                got = (D[None] * G[px]).sum(axis=(1, 2))
                scale = (np.abs(D)[None] * np.abs(G[px])).sum(axis=(1, 2))
                err = np.abs(got - np.diag(T[td][0])) / scale
                print(f"{name} {kind} {px}, D {seed}: {err.max():.2e} of sum |D| |{px}|")
                assert err.max() <= 1e-12, (px, seed)


# ---- a map outside the mesh ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [True, False])
def test_a_map_outside_the_mesh_gives_exact_zeros(sections, fields, layers):
    import torch
    mf, _ = fields["three"]
    prof = outside_profile(layers)
    for kind in KINDS:
        modes = _random_records(kind, mf, 3, seed=4)
        _, vals, _ = mf._check_records(modes)
        mf._ensure_locator()
        staged, _src = mf._stage(vals)
        mf._set_index_map(prof.index_map)
        need = ctypes.c_int64(0)
        assert mf._lib.plfem_index_map_gradient_work_bytes(mf._loc, vals.shape[0], 3, ctypes.byref(need)) == _native.PLFEM_OK
        work = torch.full((need.value + 256,), 0xFF, dtype=torch.uint8, device=mf.tdev)
        G = mf._index_map_densities_staged(kind, staged, prof, work=work)
        for nm, v in G.items():
            assert v.shape[-2:] == (5, 6) and not v.any(), nm


# ---- bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m3l", "two"])
def test_repeats_permutations_subsets_work_contents_and_chunks_give_the_same_bits(sections, fields, name):
    import torch
    pg, mf, _ = _of(sections, fields, name)
    prof = pg.index_profile
    k = 33
    for kind in KINDS:
        modes = _random_records(kind, mf, k, seed=7)
        G = mf.index_map_densities(modes, pg)
        assert _same(G, mf.index_map_densities(modes, pg))
        planes = [nm for nm in G if nm != "support"]
        perm = np.random.default_rng(k).permutation(k)
        P = mf.index_map_densities([modes[i] for i in perm], pg)
        assert all(np.array_equal(P[nm], G[nm][perm]) for nm in planes) and np.array_equal(P["support"], G["support"])
        S = mf.index_map_densities(modes[5:25], pg)
        assert all(np.array_equal(S[nm], G[nm][5:25]) for nm in planes)
        A, B = mf.index_map_densities(modes[:16], pg), mf.index_map_densities(modes[16:], pg)
        assert all(np.array_equal(np.concatenate([A[nm], B[nm]]), G[nm]) for nm in planes)
        assert np.array_equal(A["support"], G["support"]) and np.array_equal(B["support"], G["support"])
        # the identity basis is the modes; a basis row that picks one mode gives that mode's planes
        E = mf.index_map_densities(modes, pg, basis=np.eye(k)[[3, 20]])
        assert all(np.array_equal(E[nm], G[nm][[3, 20]]) for nm in planes)
        # a caller's work buffer: poisoned with 0xFF bytes, zeroed, and against the fresh one of the calls above
        _, vals, _ = mf._check_records(modes)
        staged, _src = mf._stage(vals)
        mf._set_index_map(prof.index_map)
        need = ctypes.c_int64(0)
        assert mf._lib.plfem_index_map_gradient_work_bytes(mf._loc, vals.shape[0], k, ctypes.byref(need)) == _native.PLFEM_OK
        for fill in (0xFF, 0):
            work = torch.full((need.value + 256,), fill, dtype=torch.uint8, device=mf.tdev)
            assert _same(G, mf._index_map_densities_staged(kind, staged, prof, work=work)), fill


# ---- the C ABI on a live locator -------------------------------------------------------------------------------------
def test_map_gradient_argument_errors_on_a_live_locator(sections, fields):
    pg, mf, em = _of(sections, fields, "m3l")
    lib = _native.load_library()
    prof = pg.index_profile
    mf._ensure_locator()
    mf._set_index_map(prof.index_map)
    modes = _random_records("vectorial", mf, 3, seed=1)
    _, vals, _ = mf._check_records(modes)
    staged, _src = mf._stage(vals)
    ny, nx = prof.index_map[0].shape
    table = prof.table()
    need, keep = ctypes.c_int64(0), ctypes.c_int64(-7)
    size = lambda ncomp, k, out=need: lib.plfem_index_map_gradient_work_bytes(mf._loc, ncomp, k, None if out is None else ctypes.byref(out))
    for ncomp, k in ((1, 1), (2, 3), (2, 256), (1, 70)):
        assert size(ncomp, k) == _native.PLFEM_OK
        nout, a, nq = ncomp, lambda b: (b + 255) // 256 * 256, 6 * mf.ne
        fixed = (a(8 * k * nout * nx * ny) + a(4 * nx * ny) + 4 * a(4 * nq) + 3 * a(8 * nq) + a(8 * 16 * nout * nq) +
                 2 * a(4 * (nx - 1) * (ny - 1)))
        print(f"ncomp = {ncomp}, k = {k}: {need.value} bytes, {need.value - fixed} of them the sort's")
        assert fixed < need.value <= fixed + 16 * nq + (4 << 20)               # the rest: the sort's temporary storage
    for bad in ((0, 3), (3, 3), (2, 0), (2, -1), (2, 257)):
        assert size(*bad, out=keep) == _native.PLFEM_EINVAL and keep.value == -7, bad
    assert size(2, 3, out=None) == _native.PLFEM_EINVAL
    assert size(2, 3) == _native.PLFEM_OK
    work = _native.device_scratch(need.value + 512, mf.tdev)
    wp = (work.data_ptr() + 255) & ~255
    out = np.zeros((3, 2, ny, nx))
    sup = np.zeros((ny, nx), dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def call(ncomp=2, k=3, modes_ptr=staged.data_ptr(), t=table, nlayer=2, bg=1.0, w=wp, wb=None, res=out, s=sup):
        return lib.plfem_index_map_gradients(mf._loc, ncomp, k, ctypes.c_void_p(modes_ptr), 1, ptr(t), nlayer, bg, ctypes.c_void_p(w),
                                             ctypes.c_int64(need.value if wb is None else wb), ptr(res), ptr(s))

    bad_table = table.copy()
    bad_table[0, 3] = -1.0
    rejected = [dict(ncomp=0), dict(ncomp=3), dict(k=0), dict(k=257), dict(t=bad_table), dict(nlayer=65), dict(nlayer=-1), dict(bg=0.0),
                dict(bg=np.nan), dict(t=None), dict(modes_ptr=0), dict(w=0), dict(res=None), dict(wb=need.value - 1), dict(w=wp + 8)]
    for kw in rejected:
        assert call(**kw) == _native.PLFEM_EINVAL, kw
        assert lib.plfem_locator_last_error(mf._loc).startswith(b"plfem_index_map_gradients: "), kw
    assert not out.any() and not sup.any()
    assert call() == _native.PLFEM_OK and out.any() and sup.any()
    ref, rsup = em.map_gradients(vals, True, prof)
    assert np.array_equal(sup, rsup)
    assert all(np.abs(out[r, o] - ref[r, o]).max() <= 1e-12 * np.abs(ref[r, o]).max() for r in range(3) for o in range(2))
    first = out.copy()
    assert call(s=None) == _native.PLFEM_OK and np.array_equal(out, first)           # the support is optional
    # a result past 2^27 doubles is refused: 2048 x 2048 pixels take 16 vectorial fields, not 17
    big = np.full((2048, 2048), 2.0)
    mf._check(_native.set_index_map_call(lib.plfem_locator_set_index_map, mf._loc, (big, -7.0, -5.0, 0.01, 0.01)), "set map")
    out[:] = 0.0
    assert size(2, 17, out=keep) == _native.PLFEM_EINVAL and keep.value == -7 and size(2, 16) == _native.PLFEM_OK
    assert call(k=17) == _native.PLFEM_EINVAL and b"2^27" in lib.plfem_locator_last_error(mf._loc)
    # no map on the locator
    mf._set_index_map(None)
    assert size(2, 3, out=keep) == _native.PLFEM_EINVAL and keep.value == -7
    assert call() == _native.PLFEM_EINVAL and b"no map on the locator" in lib.plfem_locator_last_error(mf._loc)
    assert not out.any()


# ---- physics: finite differences of GPU re-solves --------------------------------------------------------------------
def _dn_map():
    """A smooth index change on M3's grid, both signs, max |Dn| = 1."""
    X, Y = np.meshgrid(M3_X, M3_Y)
    d = np.exp(-((X - 0.3) ** 2 + (Y - 0.2) ** 2) / 4.0) - 0.8 * np.exp(-((X - 5.0) ** 2 + Y ** 2) / 3.0) \
        + 0.6 * np.exp(-((X + 2.5) ** 2 + (Y - 4.33) ** 2) / 2.0) * np.cos(X + Y)
    return d / np.abs(d).max()


@pytest.fixture(scope="module")
def m3_solves(sections, gpu_device):
    pg, _ = sections["m3"]
    mesh = sections["_mesh"]["three"]
    X, Y = np.meshgrid(M3_X, M3_Y)
    n0, Dn = m3_index(X, Y), _dn_map()
    assert np.array_equal(IndexProfile(1.0).sampled(M3_X, M3_Y, n0).index_map[0], pg.index_profile.index_map[0])
    S = Solvers(pg, mesh, gpu_device)
    out = {"Dn": Dn}
    for kind in KINDS:
        out[kind] = {"base": S.solve(kind, pg),
                     "moved": [S.solve(kind, at_k0(pg, IndexProfile(1.0).sampled(M3_X, M3_Y, n0 + s * DELTA * Dn), 1.0)) for s in (1, -1)]}
    S.close()
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_gradient_of_m3_against_finite_differences_of_gpu_solves(sections, fields, m3_solves, kind):
    """Measured on an MI355X (worst group, vectorial / scalar): see DESIGN.md section 32."""
    pg, mf, _ = _of(sections, fields, "m3")
    prof = pg.index_profile
    modes, Dn = m3_solves[kind]["base"], m3_solves["Dn"]
    res = index_map_gradient(modes, mf, pg, cluster_rtol=1e-6)
    k = len(modes)
    assert res["dneff_dn"].shape == res["dneff_deps_cluster"].shape == (k,) + Dn.shape and res["norm"].shape == (k,)
    assert np.array_equal(res["support"], res["densities"]["support"]) and np.all(res["dneff_dn"][:, res["support"] == 0] == 0.0)
    along = (Dn[None] * res["dneff_dn_cluster"]).sum(axis=(1, 2))
    rows = group_means(kind, modes, res["cluster"], along, m3_solves[kind]["moved"],
                       lambda p, m: np.mean([(a["n_eff"] - b["n_eff"]) / (2 * DELTA) for a, b in zip(p, m)]))
    worst = max(abs(v - f) for _, v, f in rows)
    big = max(abs(f) for _, _, f in rows)
    print(f"{kind}: dn_eff along Dn, {len(rows)} groups of {k} records, worst |HF - FD| = {worst:.2e} (largest {big:.3f})")
    assert len(rows) >= 3 and worst <= 1e-6
    sens = profile_sensitivity(modes, mf, pg, tangents=[prof.tangent_index(dn_map=Dn)], cluster_rtol=1e-6)
    single = res["cluster"] < 0
    assert np.array_equal(sens["cluster"], res["cluster"]) and single.sum() >= 1
    plain = (Dn[None] * res["dneff_dn"]).sum(axis=(1, 2))
    e = np.abs(sens["dneff_dp"][:, 0] - plain)[single].max()
    print(f"{kind}: against profile_sensitivity on {single.sum()} non-degenerate records: {e:.2e}")
    assert e <= 1e-9
