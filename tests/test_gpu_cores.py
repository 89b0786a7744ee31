"""Per-core Grams on the GPU (k_core_owner, k_core_count, k_core_fill, k_core_grams, k_overlap_reduce): the kernels against
the NumPy emulation (tests/core_gram_emulation.py) on seeded random DOF values for core tables that exercise every path
of the compaction and the tiling, against ModeFields.grams, bit identity under repeats, mode subsets and a NaN-filled
work buffer, argument errors at the C ABI, and core_decomposition end to end at C1 L = 0 with both solvers:
d n_eff / d n_core against finite differences of three GPU solves."""
import copy
import ctypes

import numpy as np
import pytest

from core_gram_emulation import CoreGramEmulation
from core_ties import Ties, jittered_square_mesh
from pl_fem_vectoriel_amd import MCFGeometry, ModeFields, _native, core_decomposition, generate_mesh
from pl_fem_vectoriel_amd.fields import CORE_GRAM_NAMES
from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver

pytestmark = pytest.mark.gpu

KS = (1, 33, 70)
KMAX = 70


def discs(positions, radii):
    """A geometry of the package with the given core discs (no PML: only the real permittivity is read)."""
    g = MCFGeometry(7, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55, use_complex_pml=False)
    g.positions = g.core_positions = np.atleast_2d(np.asarray(positions, dtype=np.float64))
    g.core_radii = np.asarray(radii, dtype=np.float64).reshape(-1)
    g.n_cores = len(g.core_radii)
    return g


def spread_discs(bbox, n=8):
    """n x n small discs spread over the box: n = 8 fills the 64-core table."""
    x = np.linspace(bbox[0], bbox[1], n + 2)[1:-1]
    y = np.linspace(bbox[2], bbox[3], n + 2)[1:-1]
    X, Y = np.meshgrid(x, y)
    return discs(np.column_stack([X.ravel(), Y.ravel()]), np.full(n * n, 0.3 * min(x[1] - x[0], y[1] - y[0])))


def records(rng, kind, nrows, k):
    if kind == "vectorial":
        return [{"Ex_dofs": rng.standard_normal(nrows), "Ey_dofs": rng.standard_normal(nrows),
                 "beta": float(rng.uniform(5, 10))} for _ in range(k)]
    return [{"field_vector": rng.standard_normal(nrows)} for _ in range(k)]


def vals(modes):
    if "Ex_dofs" in modes[0]:
        return np.stack([np.array([m["Ex_dofs"] for m in modes]), np.array([m["Ey_dofs"] for m in modes])])
    return np.array([m["field_vector"] for m in modes])[None]


def few_point_discs(em, bbox):
    """Four discs around one quadrature point in the middle of the mesh: one that owns no point (it lies between the
    quadrature points), one with fewer than 16 points, one with more whose count is no multiple of 16, and a large one;
    the later ones contain the earlier ones, so the highest index takes the shared points."""
    qx, qy = (a.reshape(-1) for a in em.basis.qx)
    cx, cy = 0.5 * (bbox[0] + bbox[1]), 0.5 * (bbox[2] + bbox[3])
    d = np.sort(np.hypot(qx - cx, qy - cy))
    mid = lambda i: 0.5 * (d[i - 1] + d[i])                       # a radius holding exactly i points
    far = (cx + 0.3 * (bbox[1] - bbox[0]), cy + 0.25 * (bbox[3] - bbox[2]))
    dfar = np.sort(np.hypot(qx - far[0], qy - far[1]))
    return discs([far, far, (cx, cy), (cx, cy)], [0.5 * dfar[0], 0.5 * (dfar[4] + dfar[5]), mid(21), mid(150)])


class Case:
    def __init__(self, mesh, device, seed):
        self.mesh = mesh
        self.mf = ModeFields(mesh, device=device)
        self.em = CoreGramEmulation(mesh.p, mesh.t)
        rng = np.random.default_rng(seed)
        self.modes = {"vectorial": records(rng, "vectorial", self.mf.nsolve, KMAX),
                      "scalar": records(rng, "scalar", self.mf.N, KMAX)}
        self.tables = {}
        self._features = {}

    def reference(self, kind, geometry):
        """The emulated per-core Grams of all KMAX modes (the features are evaluated once per kind)."""
        v, indexed = vals(self.modes[kind]), kind == "vectorial"
        if kind not in self._features:
            self._features[kind] = self.em.flat_features(v, indexed)
        return self.em.core_grams(v, indexed, geometry, features=self._features[kind])


@pytest.fixture(scope="module")
def cases(c1_geometry, gpu_device, built_library):
    c1 = Case(generate_mesh(c1_geometry, 1.0, 0), gpu_device, 1)
    T = Ties(jittered_square_mesh(8))
    sq = Case(T.mesh, gpu_device, 2)
    ov = discs([(0.0, 0.0), (1.2, 0.3)], [1.5, 1.0])
    c1.tables = {"1 core": discs([(0.0, 0.0)], [1.5]), "c1": c1_geometry, "64 cores": spread_discs(c1.mf.bbox),
                 "overlapping": ov, "few points": few_point_discs(c1.em, c1.mf.bbox)}
    sq.tables = {"ties": T.geometry(), "64 cores": spread_discs(sq.mf.bbox), "few points": few_point_discs(sq.em, sq.mf.bbox),
                 "overlapping": discs([(0.4, 0.5), (0.6, 0.5)], [0.25, 0.2])}
    sq.ties = T
    out = {"c1": c1, "sq": sq}
    yield out
    for c in out.values():
        c.mf.close()
    import torch
    torch.cuda.empty_cache()


def test_core_tables_cover_the_paths(cases):
    """The tables of the comparison below, by the emulation: an empty core, one under a tile, a count off the tile size,
    shared points, every slot of the 64-core table, and the tie discs decided as the reference decides them."""
    for case in cases.values():
        pts = case.em.core_grams(np.ones((1, 1, case.mf.N)), False, case.tables["few points"])["points"]
        assert pts[0] == 0 and 0 < pts[1] < 16 and pts[2] == 0 and pts[3] == 150 and pts[3] % 16
        g = case.tables["overlapping"]
        both = np.ones_like(case.em.core_mask(g))
        for (cx, cy), r in zip(g.positions, g.core_radii):
            both &= (case.em.basis.qx[0] - cx) ** 2 + (case.em.basis.qx[1] - cy) ** 2 <= r * r
        assert both.sum() >= 10
        assert np.atleast_2d(case.tables["64 cores"].positions).shape[0] == 64
    T = cases["sq"].ties
    assert np.array_equal(cases["sq"].em.core_owner(cases["sq"].tables["ties"]) >= 0, T.core(cases["sq"].tables["ties"]))
    assert any(T.flips)


@pytest.mark.parametrize("kind", ["vectorial", "scalar"])
@pytest.mark.parametrize("mesh", ["c1", "sq"])
def test_kernel_matches_emulation(cases, mesh, kind):
    case = cases[mesh]
    mf, em = case.mf, case.em
    worst = 0.0
    for tname, g in case.tables.items():
        ref_all = case.reference(kind, g)
        ncore = ref_all["points"].size
        for k in KS:
            C = mf.core_grams(case.modes[kind][:k], g)
            assert set(C) == set(CORE_GRAM_NAMES[kind]) | {"points"}
            assert C["points"].dtype == np.int64 and np.array_equal(C["points"], ref_all["points"]), (tname, k)
            for nm in CORE_GRAM_NAMES[kind]:
                ref = ref_all[nm][:, :k, :k]
                assert C[nm].shape == (ncore, k, k)
                scale = np.abs(ref.sum(0)).max()
                err = np.abs(C[nm] - ref).max() / scale
                worst = max(worst, err)
                assert err <= 1e-12, (tname, k, nm, err)
                assert (C[nm][ref_all["points"] == 0] == 0).all(), (tname, k, nm)      # exact zeros, not small numbers
    print(f"{mesh} {kind}: worst error {worst:.2e} of max |sum_c G_c|")


@pytest.mark.parametrize("mesh", ["c1", "sq"])
def test_cores_sum_to_the_core_region_of_mode_grams(cases, mesh):
    case = cases[mesh]
    for kind in ("vectorial", "scalar"):
        modes = case.modes[kind][:33]
        for tname, g in case.tables.items():
            G, C = case.mf.grams(modes, g), case.mf.core_grams(modes, g)
            M = C["Mx"] + C["My"] if kind == "vectorial" else C["M"]
            scale = np.abs(G["M_core"]).max()
            if scale == 0:
                assert (M == 0).all()
                continue
            assert np.abs(M.sum(0) - G["M_core"]).max() <= 1e-12 * scale, (kind, tname)
            if kind == "vectorial":
                assert np.abs(C["K"].sum(0) - G["K_core"]).max() <= 1e-12 * np.abs(G["K_core"]).max(), tname


def _same(a, b):
    return all(np.array_equal(a[nm], b[nm]) for nm in a)


@pytest.mark.parametrize("mesh", ["c1", "sq"])
def test_repeats_subsets_and_a_nan_filled_work_buffer_give_the_same_bits(cases, mesh, monkeypatch):
    case = cases[mesh]
    mf = case.mf
    g = case.tables["64 cores"]
    rng = np.random.default_rng(5)
    subsets = [rng.permutation(KMAX), np.array([31, 32, 33, 0, 69, 64, 63, 1]), np.arange(KMAX)[::-3], np.array([65])]
    for kind in ("vectorial", "scalar"):
        modes = case.modes[kind]
        C = mf.core_grams(modes, g)
        assert _same(C, mf.core_grams(modes, g))
        for I in subsets:
            CI = mf.core_grams([modes[i] for i in I], g)
            for nm in CORE_GRAM_NAMES[kind]:
                assert np.array_equal(CI[nm], C[nm][:, I][:, :, I]), (kind, len(I), nm)
            assert np.array_equal(CI["points"], C["points"])
        plain = {tname: mf.core_grams(modes[:33], t) for tname, t in case.tables.items()}
        with monkeypatch.context() as mp:
            mp.setattr(_native, "SCRATCH_FILL", float("nan"))          # work buffer and staging target start as NaN
            for tname, t in case.tables.items():
                assert _same(plain[tname], mf.core_grams(modes[:33], t)), (kind, tname)
        assert _native.SCRATCH_FILL is None


def test_argument_errors_at_the_c_abi(cases):
    mf = cases["sq"].mf
    mf._ensure_locator()
    lib = mf._lib
    import torch
    k, ncore = 3, 2
    staged, _ = mf._stage(vals(cases["sq"].modes["scalar"][:k]))
    cores = np.array([[0.3, 0.3, 0.1], [0.7, 0.7, 0.1]])
    need = ctypes.c_int64(-1)
    for ncomp_, k_, ncore_ in ((0, k, ncore), (3, k, ncore), (1, 0, ncore), (1, -2, ncore), (1, k, 0), (1, k, 65)):
        assert lib.plfem_core_gram_work_bytes(mf._loc, ncomp_, k_, ncore_, ctypes.byref(need)) == _native.PLFEM_EINVAL
    assert lib.plfem_core_gram_work_bytes(mf._loc, 1, k, ncore, None) == _native.PLFEM_EINVAL and need.value == -1
    assert lib.plfem_core_gram_work_bytes(mf._loc, 1, k, ncore, ctypes.byref(need)) == _native.PLFEM_OK
    nbytes = int(need.value)
    assert nbytes >= ncore * k * k * 8 + 2 * 6 * mf.ne * 4
    work = torch.empty(nbytes + 256, dtype=torch.uint8, device=mf.tdev)
    aligned = (work.data_ptr() + 255) & ~255
    out = np.zeros((ncore, 1, k, k))
    pts = np.full(ncore, -7, dtype=np.int64)
    good = dict(ncomp=1, k=k, modes=staged.data_ptr(), cores=cores.ctypes.data, ncore=ncore, work=aligned, nbytes=nbytes,
                out=out.ctypes.data, pts=pts.ctypes.data)

    def call(**kw):
        a = {**good, **kw}
        return lib.plfem_core_grams(mf._loc, a["ncomp"], a["k"], ctypes.c_void_p(a["modes"]), 0, ctypes.c_void_p(a["cores"]),
                                    a["ncore"], ctypes.c_void_p(a["work"]), ctypes.c_int64(a["nbytes"]),
                                    ctypes.c_void_p(a["out"]), ctypes.c_void_p(a["pts"]))

    bad = [dict(ncomp=0), dict(ncomp=3), dict(k=0), dict(ncore=0), dict(ncore=65), dict(modes=None), dict(cores=None),
           dict(work=None), dict(out=None), dict(pts=None), dict(nbytes=nbytes - 1), dict(work=aligned + 8)]
    for kw in bad:
        assert call(**kw) == _native.PLFEM_EINVAL, kw
        assert "plfem_core_grams" in lib.plfem_locator_last_error(mf._loc).decode(), kw
    assert (out == 0).all() and (pts == -7).all()
    assert call() == _native.PLFEM_OK
    ref = cases["sq"].em.core_grams(vals(cases["sq"].modes["scalar"][:k]), False, discs(cores[:, :2], cores[:, 2]))
    assert np.array_equal(pts, ref["points"])
    assert np.abs(out[:, 0] - ref["M"]).max() <= 1e-12 * np.abs(ref["M"].sum(0)).max()


# -- end to end at C1 L = 0 -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1(c1_geometry, gpu_device, built_library):
    mesh = generate_mesh(c1_geometry, 1.0, 0)
    vsol = TrueVectorialMaxwellSolver(c1_geometry, device=gpu_device, eig_tol=1e-10)
    ssol = ScalarHelmholtzSolver(c1_geometry, device=gpu_device, eig_tol=1e-10)
    vec = vsol.solve_vectorial_modes(mesh, 20)
    scal = ssol.solve(mesh, 10)
    mf = ModeFields(mesh, device=gpu_device, solver=vsol)
    yield {"mesh": mesh, "vsol": vsol, "ssol": ssol, "vec": vec, "scal": scal, "mf": mf}
    mf.close()
    vsol.clear_cache()
    ssol.clear_cache()
    import torch
    torch.cuda.empty_cache()


def test_decomposition_of_solver_modes(c1, c1_geometry):
    g = c1_geometry
    for modes in (c1["vec"], c1["scal"]):
        before = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in m.items()} for m in modes]
        res = core_decomposition(modes, c1["mf"], g, n_cores=np.full(7, g.n_core), direction=np.ones(7))
        k = len(modes)
        print(f"{k} modes: rayleigh defect max {res['rayleigh_defect'].max():.2e}; power in the cores "
              f"{res['power'].sum(1).min():.4f}..{res['power'].sum(1).max():.4f}; points {res['points'].tolist()}; "
              f"clusters {int(res['cluster'].max()) + 1}")
        assert res["power"].shape == (k, 7) and res["dneff_dn"].shape == (k, 7) and res["sensitivity"].shape == (7, k, k)
        assert np.abs(res["power"].sum(1) + res["power_clad"] - 1).max() <= 1e-12
        assert res["rayleigh_defect"].max() <= 1e-10
        assert (res["points"] > 0).all() and (res["power"] >= 0).all()
        if "Ex_dofs" in modes[0]:
            assert np.abs(res["power_x"] + res["power_y"] - res["power"]).max() <= 1e-14
            assert ((res["pdl_db"] >= 0) & (res["pdl_db"] <= 50)).all()
        # every core at n_core: the Ritz values are the modes' own n_eff, to the Rayleigh defect
        ne = np.sort([m["n_eff"] for m in modes])[::-1]
        assert np.abs(res["n_eff_ritz"] - ne).max() <= 1e-9
        for a, b in zip(modes, before):
            assert set(a) == set(b)
            for key in a:
                assert np.array_equal(a[key], b[key]) if isinstance(b[key], np.ndarray) else a[key] == b[key]
        again = core_decomposition(modes, c1["mf"], g, direction=np.ones(7))
        assert np.array_equal(res["dneff_dn"], again["dneff_dn"]) and np.array_equal(res["power"], again["power"])
        assert np.array_equal(res["dneff_direction"], again["dneff_direction"])


def _fd(solver, solve, mesh, geometry, modes, delta=1e-5):
    """beta at n_core +- delta of each mode, matched by a unique |cos| > 0.999 partner (nan otherwise), from two more solves on
    the same mesh object and the same solver (its analysis and context are reused)."""
    out = []
    x = vals(modes).transpose(1, 0, 2).reshape(len(modes), -1)
    x = x / np.linalg.norm(x, axis=1)[:, None]
    g0 = solver.geometry
    try:
        for s in (delta, -delta):
            g = copy.copy(geometry)
            g.n_core = geometry.n_core + s
            solver.geometry = g
            other = solve(mesh)
            y = vals(other).transpose(1, 0, 2).reshape(len(other), -1)
            c = np.abs(x @ (y / np.linalg.norm(y, axis=1)[:, None]).T)
            b = np.array([other[int(np.argmax(r))]["beta"] for r in c])
            b[(c > 0.999).sum(1) != 1] = np.nan
            out.append(b)
    finally:
        solver.geometry = g0
    return out, 2 * delta


def test_index_sensitivity_against_finite_differences_of_gpu_solves(c1, c1_geometry):
    mesh = c1["mesh"]
    cases = (("vectorial", c1["vsol"], lambda m: c1["vsol"].solve_vectorial_modes(m, 20), c1["vec"], 1.0),
             ("scalar", c1["ssol"], lambda m: c1["ssol"].solve(m, 10), c1["scal"], -1.0))
    for kind, solver, solve, modes, sgn in cases:
        res = core_decomposition(modes, c1["mf"], c1_geometry, direction=np.ones(7))
        (bp, bm), h = _fd(solver, solve, mesh, c1_geometry, modes)
        mu = sgn * np.array([m["beta"] for m in modes]) ** 2
        mup, mum = sgn * bp ** 2, sgn * bm ** 2
        errs = []
        for i in range(len(modes)):
            j = int(np.argsort(np.abs(mu - mu[i]))[1])
            moved = max(abs((mup[i] - mup[j]) - (mu[i] - mu[j])), abs((mum[i] - mum[j]) - (mu[i] - mu[j])))
            if not np.isfinite(moved) or abs(mu[i] - mu[j]) < 100 * moved:
                continue
            errs.append(abs(res["dneff_direction"][i] - (bp[i] - bm[i]) / (h * c1_geometry.k0)))
        print(f"{kind}: {len(errs)} of {len(modes)} modes compared, worst |dn_eff/dn_core (HF) - (FD)| = {max(errs):.2e}")
        assert len(errs) >= 3
        assert max(errs) <= 1e-6
