"""Coordinate-weighted Grams on the GPU (k_moment_grams, k_overlap_reduce): the kernel against the NumPy emulation
(tests/moment_gram_emulation.py) on seeded random DOF values for mode counts and core tables that exercise every path of
the tiling and the region branch, the origin-shift identity against ModeFields.grams, bit identity under repeats, mode
subsets and a NaN-filled work buffer, argument errors at the C ABI, and bend_response end to end at C1 L = 0 with both
solvers."""
import ctypes

import numpy as np
import pytest

from core_ties import Ties, jittered_square_mesh
from moment_gram_emulation import MomentGramEmulation
from pl_fem_vectoriel_amd import (ModeFields, _native, bend_propagate, bend_quantities_from_grams, bend_response,
                                  generate_mesh)
from pl_fem_vectoriel_amd.fields import MOMENT_GRAM_NAMES
from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver
from test_gpu_cores import discs, records, vals

pytestmark = pytest.mark.gpu

KS = (1, 33, 70)        # one lane block; past one 32-mode chunk; three chunks with a ragged last one
KMAX = 70
ORIGIN = (0.37, -1.21)


def no_cores():
    g = discs([(0.0, 0.0)], [1.0])
    g.positions = g.core_positions = np.zeros((0, 2))
    g.core_radii = np.zeros(0)
    g.n_cores = 0
    return g


def empty_disc(em, bbox):
    """A disc in the middle of the mesh that holds no quadrature point (half the distance to the nearest one)."""
    qx, qy = (a.reshape(-1) for a in em.basis.qx)
    cx, cy = 0.5 * (bbox[0] + bbox[1]) + 0.01, 0.5 * (bbox[2] + bbox[3]) - 0.02
    return discs([(cx, cy)], [0.5 * np.hypot(qx - cx, qy - cy).min()])


class Case:
    def __init__(self, mesh, device, seed):
        self.mesh = mesh
        self.mf = ModeFields(mesh, device=device)
        self.em = MomentGramEmulation(mesh.p, mesh.t)
        rng = np.random.default_rng(seed)
        self.modes = {"vectorial": records(rng, "vectorial", self.mf.nsolve, KMAX),
                      "scalar": records(rng, "scalar", self.mf.N, KMAX)}
        self.tables = {}
        self._features = {}

    def reference(self, kind, geometry, origin=ORIGIN):
        """The emulated moment Grams of all KMAX modes (the features are evaluated once per kind)."""
        v, indexed = vals(self.modes[kind]), kind == "vectorial"
        if kind not in self._features:
            self._features[kind] = self.em.flat_features(v, indexed)
        return self.em.moment_grams(v, indexed, geometry, origin, features=self._features[kind])


@pytest.fixture(scope="module")
def cases(c1_geometry, gpu_device, built_library):
    c1 = Case(generate_mesh(c1_geometry, 1.0, 0), gpu_device, 11)
    assert c1.mf.ne == 11313
    T = Ties(jittered_square_mesh(8))
    sq = Case(T.mesh, gpu_device, 12)
    c1.tables = {"no cores": no_cores(), "1 core": discs([(0.0, 0.0)], [1.5]), "c1": c1_geometry,
                 "empty disc": empty_disc(c1.em, c1.mf.bbox)}
    sq.tables = {"no cores": no_cores(), "ties": T.geometry(), "empty disc": empty_disc(sq.em, sq.mf.bbox),
                 "1 core": discs([(0.45, 0.55)], [0.2])}
    sq.ties = T
    out = {"c1": c1, "sq": sq}
    yield out
    for c in out.values():
        c.mf.close()
    import torch
    torch.cuda.empty_cache()


def test_core_tables_cover_the_region_branch(cases):
    """By the emulation: a table without cores and a disc that owns no point put every point in the cladding, the others
    split the points, and the tie discs are decided as the reference decides them."""
    for case in cases.values():
        for tname, g in case.tables.items():
            n = int(case.em.core_mask(g).sum())
            assert (n == 0) == (tname in ("no cores", "empty disc")), tname
            assert n < 6 * case.mf.ne
    T = cases["sq"].ties
    assert np.array_equal(cases["sq"].em.core_mask(cases["sq"].tables["ties"]), T.core(cases["sq"].tables["ties"]))
    assert any(T.flips)


@pytest.mark.parametrize("kind", ["vectorial", "scalar"])
@pytest.mark.parametrize("mesh", ["c1", "sq"])
def test_kernel_matches_emulation(cases, mesh, kind):
    case = cases[mesh]
    mf = case.mf
    worst = 0.0
    for tname, g in case.tables.items():
        ref_all = case.reference(kind, g)
        ncore = int(case.em.core_mask(g).sum())
        for k in KS:
            P = mf.moment_grams(case.modes[kind][:k], g, origin=ORIGIN)
            assert tuple(P) == MOMENT_GRAM_NAMES[kind]
            for nm in MOMENT_GRAM_NAMES[kind]:
                ref = ref_all[nm][:k, :k]
                assert P[nm].shape == (k, k)
                if "core" in nm and ncore == 0:
                    assert (P[nm] == 0).all(), (tname, k, nm)              # exact zeros, not small numbers
                    continue
                err = np.abs(P[nm] - ref).max() / np.abs(ref).max()
                worst = max(worst, err)
                assert err <= 1e-12, (tname, k, nm, err)
    print(f"{mesh} {kind}: worst error {worst:.2e} of max |output|")


@pytest.mark.parametrize("mesh", ["c1", "sq"])
def test_origin_shift_against_mode_grams(cases, mesh):
    case = cases[mesh]
    o = ORIGIN
    for kind in ("vectorial", "scalar"):
        modes = case.modes[kind][:33]
        g = case.tables["1 core"]
        G, P0, P1 = case.mf.grams(modes, g), case.mf.moment_grams(modes, g), case.mf.moment_grams(modes, g, origin=o)
        forms = ("M", "K") if kind == "vectorial" else ("M",)
        for f in forms:
            for r in ("core", "clad"):
                for ax, oo in (("X", o[0]), ("Y", o[1])):
                    a, b = P1[f"{f}_{r}_{ax}"], P0[f"{f}_{r}_{ax}"] - oo * G[f"{f}_{r}"]
                    scale = np.abs(P0[f"{f}_{r}_{ax}"]).max() + abs(oo) * np.abs(G[f"{f}_{r}"]).max()
                    assert np.abs(a - b).max() <= 1e-12 * scale, (kind, f, r, ax)
        M = G["M_core"] + G["M_clad"]
        MX = P0["M_core_X"] + P0["M_clad_X"]
        b = P0["M_XX"] - 2 * o[0] * MX + o[0] ** 2 * M
        scale = np.abs(P0["M_XX"]).max() + 2 * abs(o[0]) * np.abs(MX).max() + o[0] ** 2 * np.abs(M).max()
        assert np.abs(P1["M_XX"] - b).max() <= 1e-12 * scale, kind


def _same(a, b):
    return all(np.array_equal(a[nm], b[nm]) for nm in a)


@pytest.mark.parametrize("mesh", ["c1", "sq"])
def test_repeats_subsets_and_a_nan_filled_work_buffer_give_the_same_bits(cases, mesh, monkeypatch):
    case = cases[mesh]
    mf = case.mf
    g = case.tables["c1" if mesh == "c1" else "ties"]
    rng = np.random.default_rng(5)
    subsets = [rng.permutation(KMAX), np.array([31, 32, 33, 0, 69, 64, 63, 1]), np.arange(KMAX)[::-3], np.array([65])]
    for kind in ("vectorial", "scalar"):
        modes = case.modes[kind]
        P = mf.moment_grams(modes, g, origin=ORIGIN)
        assert _same(P, mf.moment_grams(modes, g, origin=ORIGIN))
        for I in subsets:
            PI = mf.moment_grams([modes[i] for i in I], g, origin=ORIGIN)
            for nm in MOMENT_GRAM_NAMES[kind]:
                assert np.array_equal(PI[nm], P[nm][I][:, I]), (kind, len(I), nm)
        plain = {tname: mf.moment_grams(modes[:33], t, origin=ORIGIN) for tname, t in case.tables.items()}
        with monkeypatch.context() as mp:
            mp.setattr(_native, "SCRATCH_FILL", float("nan"))          # work buffer and staging target start as NaN
            for tname, t in case.tables.items():
                assert _same(plain[tname], mf.moment_grams(modes[:33], t, origin=ORIGIN)), (kind, tname)
        assert _native.SCRATCH_FILL is None


def test_argument_errors_at_the_c_abi(cases):
    case = cases["sq"]
    mf = case.mf
    mf._ensure_locator()
    lib = mf._lib
    import torch
    k, ncore = 3, 2
    staged, _ = mf._stage(vals(case.modes["scalar"][:k]))
    cores = np.array([[0.3, 0.3, 0.1], [0.7, 0.7, 0.1]])
    origin = np.array(ORIGIN)
    nan_o, inf_o = np.array([np.nan, 0.0]), np.array([0.0, -np.inf])
    need = ctypes.c_int64(-1)
    for ncomp_, k_ in ((0, k), (3, k), (1, 0), (1, -2)):
        assert lib.plfem_moment_gram_work_bytes(ncomp_, k_, ctypes.byref(need)) == _native.PLFEM_EINVAL
    assert lib.plfem_moment_gram_work_bytes(1, k, None) == _native.PLFEM_EINVAL and need.value == -1
    assert lib.plfem_moment_gram_work_bytes(1, k, ctypes.byref(need)) == _native.PLFEM_OK
    nbytes = int(need.value)
    work = torch.empty(nbytes + 256, dtype=torch.uint8, device=mf.tdev)
    aligned = (work.data_ptr() + 255) & ~255
    out = np.zeros((7, k, k))
    good = dict(ncomp=1, k=k, modes=staged.data_ptr(), cores=cores.ctypes.data, ncore=ncore, origin=origin.ctypes.data,
                work=aligned, nbytes=nbytes, out=out.ctypes.data)

    def call(**kw):
        a = {**good, **kw}
        return lib.plfem_moment_grams(mf._loc, a["ncomp"], a["k"], ctypes.c_void_p(a["modes"]), 0, ctypes.c_void_p(a["cores"]),
                                      a["ncore"], ctypes.c_void_p(a["origin"]), ctypes.c_void_p(a["work"]),
                                      ctypes.c_int64(a["nbytes"]), ctypes.c_void_p(a["out"]))

    bad = [dict(ncomp=0), dict(ncomp=3), dict(k=0), dict(ncore=-1), dict(ncore=65), dict(modes=None), dict(cores=None),
           dict(origin=None), dict(origin=nan_o.ctypes.data), dict(origin=inf_o.ctypes.data), dict(work=None), dict(out=None),
           dict(nbytes=nbytes - 1), dict(work=aligned + 8)]
    for kw in bad:
        assert call(**kw) == _native.PLFEM_EINVAL, kw
        assert "plfem_moment_grams" in lib.plfem_locator_last_error(mf._loc).decode(), kw
    assert (out == 0).all()
    assert call() == _native.PLFEM_OK
    ref = case.em.moment_grams(vals(case.modes["scalar"][:k]), False, discs(cores[:, :2], cores[:, 2]), ORIGIN)
    for i, nm in enumerate(MOMENT_GRAM_NAMES["scalar"]):
        assert np.abs(out[i] - ref[nm]).max() <= 1e-12 * np.abs(ref[nm]).max(), nm
    assert call(ncore=0, cores=None) == _native.PLFEM_OK             # no table is needed without cores
    assert (out[:2] == 0).all()


# -- end to end at C1 L = 0 -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1(c1_geometry, gpu_device, built_library):
    mesh = generate_mesh(c1_geometry, 1.0, 0)
    vsol = TrueVectorialMaxwellSolver(c1_geometry, device=gpu_device, eig_tol=1e-10)
    ssol = ScalarHelmholtzSolver(c1_geometry, device=gpu_device, eig_tol=1e-10)
    vec = vsol.solve_vectorial_modes(mesh, 20)
    scal = ssol.solve(mesh, 10)
    mf = ModeFields(mesh, device=gpu_device, solver=vsol)
    yield {"mesh": mesh, "vec": vec, "scal": scal, "mf": mf, "em": MomentGramEmulation(mesh.p, mesh.t)}
    mf.close()
    vsol.clear_cache()
    ssol.clear_cache()
    import torch
    torch.cuda.empty_cache()


def test_bend_response_of_solver_modes(c1, c1_geometry):
    g, em = c1_geometry, c1["em"]
    radii, angles, o = np.array([np.inf, 8000.0, -4000.0]), np.array([0.0, 0.3, 2.0]), (0.5, -0.25)
    for modes in (c1["vec"], c1["scal"]):
        kind = "vectorial" if "Ex_dofs" in modes[0] else "scalar"
        k = len(modes)
        before = [{key: (v.copy() if isinstance(v, np.ndarray) else v) for key, v in m.items()} for m in modes]
        res = bend_response(modes, c1["mf"], g, radius=radii, angle=angles, origin=o)
        for a, b in zip(modes, before):
            assert set(a) == set(b)
            for key in a:
                assert np.array_equal(a[key], b[key]) if isinstance(b[key], np.ndarray) else a[key] == b[key]
        v, beta = vals(modes), np.array([m["beta"] for m in modes])
        emu = bend_quantities_from_grams(kind, em.moment_grams(v, kind == "vectorial", g, o), em.grams(v, kind == "vectorial", g),
                                         beta, g.k0, (g.n_core ** 2, g.n_clad ** 2), curvature=1 / radii, angle=angles)
        print(f"{kind}, {k} modes: rayleigh defect max {res['rayleigh_defect'].max():.2e}; |dneff/dkappa| up to "
              f"{np.abs(res['dneff_dkappa']).max():.3f} um; D4-sigma {res['width_d4sigma'].min():.2f}..{res['width_d4sigma'].max():.2f} "
              f"um; shifts at R = 4 mm up to {np.nanmax(np.abs(res['n_eff_ritz'][2] - res['n_eff_ritz'][0])):.2e}; clusters "
              f"{int(res['cluster'].max()) + 1}")
        assert res["rayleigh_defect"].max() <= 1e-10
        assert res["centroid"].shape == (k, 2) and res["second_moment"].shape == (k, 2, 2) and res["width_d4sigma"].shape == (k, 2)
        assert res["coupling"].shape == (2, k, k) and res["dneff_dkappa"].shape == (3, k)
        assert res["n_eff_ritz"].shape == (3, k) and res["mixing"].shape == (3, k, k)
        assert np.array_equal(res["cluster"], emu["cluster"])
        for nm in ("centroid", "second_moment", "width_d4sigma", "coupling", "dneff_dkappa", "n_eff_ritz", "beta_ritz"):
            assert np.isfinite(res[nm]).all(), nm
            err = np.abs(res[nm] - emu[nm]).max() / np.abs(emu[nm]).max()
            assert err <= 1e-10, (kind, nm, err)
        # the straight fibre: the Ritz values are the records' own n_eff, to the Rayleigh defect
        ne = np.sort([m["n_eff"] for m in modes])[::-1]
        assert np.abs(res["n_eff_ritz"][0] - ne).max() <= 1e-9
        assert set(res["grams"]) | set(res["moment_grams"]) >= set(MOMENT_GRAM_NAMES[kind])
        again = bend_response(modes, c1["mf"], g, radius=radii, angle=angles, origin=o)
        assert all(np.array_equal(res[nm], again[nm]) for nm in ("dneff_dkappa", "coupling", "n_eff_ritz", "centroid"))
        if kind == "scalar":
            T = bend_propagate(res, [[500.0, 1 / 8000.0, 0.3], [200.0, 0.0, 0.0]])["transfer"]
            B = res["pencil"]["B"]
            assert np.abs(T.conj().T @ B @ T - B).max() <= 1e-12
