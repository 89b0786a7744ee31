"""Mode-field kernels (k_stage_modes, k_sample_fields, k_field_overlap, k_mode_grams, k_overlap_reduce) past one 32-mode
chunk, on seeded random DOF values, against the NumPy emulations (tests/fields_emulation.py, tests/gram_emulation.py) and
against closed-form integrals of quadratics; bit-identical sub-blocks and repeats; exact staging; one solver path past 32
modes; and the core test on quadrature points exactly on a core circle (tests/core_ties.py)."""
import ctypes
import time

import numpy as np
import pytest
import scipy.sparse as sp

from core_ties import Ties, jittered_square_mesh
from fields_emulation import overlap as em_overlap
from gram_emulation import GramEmulation
from oracle import hfield
from oracle.p2 import MeshTriLite, P2Basis
from pl_fem_vectoriel_amd import MCFGeometry, ModeFields, _native, generate_mesh, mode_dispersion, mode_overlap
from pl_fem_vectoriel_amd.mesh import unit_square_mesh
from pl_fem_vectoriel_amd.solver_fem import TrueVectorialMaxwellSolver, _core_table

pytestmark = pytest.mark.gpu

KS = (1, 31, 32, 33, 64, 65, 70)
PAIRS = ((1, 65), (33, 70), (70, 1), (32, 33), (64, 65))
KMAX = 70
SAMPLE_TOL = 1e-12      # sampled values against the emulation, of the largest reference value of the component
OVERLAP_TOL = 1e-12     # overlap matrices against the emulation, of the largest reference entry


def discs(positions, radii):
    """A geometry of the package with the given core discs (no PML: only the real permittivity is read)."""
    g = MCFGeometry(7, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55, use_complex_pml=False)
    g.positions = g.core_positions = np.asarray(positions, dtype=np.float64)
    g.core_radii = np.asarray(radii, dtype=np.float64)
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


class Case:
    def __init__(self, mesh, device, seed):
        self.mesh = mesh
        self.mf = ModeFields(mesh, device=device)
        self.em = GramEmulation(mesh.p, mesh.t)
        rng = np.random.default_rng(seed)
        self.modes = {"vectorial": records(rng, "vectorial", self.mf.nsolve, KMAX),
                      "scalar": records(rng, "scalar", self.mf.N, KMAX)}
        self.qloc = self.em.locate(self.em.quadrature()[0])          # own quadrature points located in this mesh


@pytest.fixture(scope="module")
def cases(c1_geometry, gpu_device, built_library):
    c1 = Case(generate_mesh(c1_geometry, 0.5, 0), gpu_device, 1)
    sq = Case(unit_square_mesh(5), gpu_device, 2)
    assert (6 * sq.mf.ne) % 64 != 0 and (6 * sq.mf.ne) % 16 != 0    # partial last tile in both kernels
    assert 6 * sq.mf.ne < 64 * 1024                                    # fewer workgroups than OVL_BLOCKS / GRAM_BLOCKS
    out = {"c1": c1, "sq": sq}
    yield out
    for c in out.values():
        c.mf.close()
    import torch
    torch.cuda.empty_cache()


def weights(case, c1_geometry):
    return {"none": None, "c1": c1_geometry, "64 cores": spread_discs(case.mf.bbox)}


def test_staging_is_an_exact_transpose(cases):
    mf = cases["sq"].mf
    mf._ensure_locator()
    rng = np.random.default_rng(3)
    for ncomp in (1, 2):
        for k in (1, 32, 33, 70):
            for nrows in (1, 31, 33, 1027):
                v = rng.standard_normal((ncomp, k, nrows))
                dst, _ = mf._stage(v)
                assert np.array_equal(dst.cpu().numpy(), v.transpose(0, 2, 1)), (ncomp, k, nrows)


def _sample_points(case, rng):
    mf = case.mf
    x0, x1, y0, y1 = mf.bbox
    dx, dy = 0.1 * (x1 - x0), 0.1 * (y1 - y0)
    rnd = np.vstack([rng.uniform(x0 - dx, x1 + dx, 700), rng.uniform(y0 - dy, y1 + dy, 700)])
    dl = mf.sym.array("doflocs").reshape(2, mf.N)                     # vertices first, then edge midpoints
    pick = rng.choice(mf.N, min(300, mf.N), replace=False)
    return np.hstack([rnd, dl[:, pick], case.mesh.p[:, :50]])


@pytest.mark.parametrize("mesh", ["c1", "sq"])
def test_sampling_matches_emulation_past_one_chunk(cases, mesh):
    case = cases[mesh]
    mf, em = case.mf, case.em
    P = _sample_points(case, np.random.default_rng(4))
    loc = em.locate(P)
    for kind in ("vectorial", "scalar"):
        indexed = kind == "vectorial"
        names = ("Hx", "Hy", "Hz_im") if indexed else ("u",)
        allm = case.modes[kind]
        beta = np.array([m["beta"] for m in allm]) if indexed else None
        ref_all, elem_em = em.sample(vals(allm), P, indexed, beta=beta, located=loc)   # mode k is row k of every k
        for k in KS:
            modes = allm[:k]
            ref = ref_all[:, :k]
            for npts in (1, 255, 257, P.shape[1]):
                out = mf.sample(modes, P[:, :npts])
                e_gpu, e_em, near = out["element"], elem_em[:npts], loc[3][:npts]
                same = e_gpu == e_em
                assert (same | (near >= 2)).all(), (kind, k, npts)
                assert (e_gpu[(e_em < 0) & (near == 0)] == -1).all()
                for c, nm in enumerate(names):
                    r = ref[c][:, :npts]
                    scale = np.abs(ref[c]).max()
                    assert out[nm].shape == (k, npts)
                    # the gradient jumps across elements: Hz_im is compared where both chose one element
                    cols = same if nm == "Hz_im" else slice(None)
                    err = np.abs(out[nm][:, cols] - r[:, cols]).max(initial=0.0)
                    assert err <= SAMPLE_TOL * scale, (kind, k, npts, nm, err / scale)
                    assert (out[nm][:, e_gpu < 0] == 0).all()


@pytest.mark.parametrize("mesh", ["c1", "sq"])
def test_overlap_matches_emulation_for_unequal_chunk_counts(cases, mesh, c1_geometry):
    case = cases[mesh]
    mf, em = case.mf, case.em
    for kind in ("vectorial", "scalar"):
        indexed = kind == "vectorial"
        for wname, w in weights(case, c1_geometry).items():
            if w is not None:
                assert np.atleast_2d(w.positions).shape[0] <= 64
            allm = case.modes[kind]
            ref_all = em_overlap(em, vals(allm), em, vals(allm), indexed, weight=w, located=case.qloc)
            for ka, kb in PAIRS:
                A, B = allm[:ka], allm[KMAX - kb:]
                O = mode_overlap(A, mf, B, mf, weight=w)
                ref = ref_all[:ka, KMAX - kb:]
                assert O.shape == (ka, kb)
                err = np.abs(O - ref).max() / np.abs(ref).max()
                assert err <= OVERLAP_TOL, (kind, wname, ka, kb, err)


@pytest.mark.parametrize("mesh", ["c1", "sq"])
def test_grams_match_emulation_past_one_chunk(cases, mesh, c1_geometry):
    case = cases[mesh]
    mf, em = case.mf, case.em
    for kind in ("vectorial", "scalar"):
        indexed = kind == "vectorial"
        for wname, w in weights(case, c1_geometry).items():
            if w is None:
                continue
            ref_all = em.grams(vals(case.modes[kind]), indexed, w)
            for k in KS:
                G = mf.grams(case.modes[kind][:k], w)
                ref = {nm: v[:k, :k] for nm, v in ref_all.items()}
                for nm in ref:
                    scale = np.abs(ref[nm]).max()
                    assert G[nm].shape == (k, k)
                    if scale == 0:          # no quadrature point in a core of this geometry
                        assert (G[nm] == 0).all(), (kind, wname, k, nm)
                        continue
                    err = np.abs(G[nm] - ref[nm]).max() / scale
                    assert err <= 1e-12, (kind, wname, k, nm, err)


def _subsets():
    rng = np.random.default_rng(5)
    return [rng.permutation(KMAX), np.array([31, 32, 33, 0, 69, 64, 63, 1]), np.arange(KMAX)[::-3],
            np.array([65]), np.concatenate([np.arange(30, 40), np.arange(60, 70)])]


@pytest.mark.parametrize("mesh", ["c1", "sq"])
def test_sub_blocks_and_repeats_are_bit_identical(cases, mesh, c1_geometry):
    """The sum order of an entry depends on the tiling of the mesh and the lane's place in its 2 x 2 block, not on the
    chunk its modes fall in: any subset / permutation of the modes gives the same bits."""
    case = cases[mesh]
    mf = case.mf
    g = spread_discs(mf.bbox)
    for kind in ("vectorial", "scalar"):
        modes = case.modes[kind]
        full = mode_overlap(modes, mf, modes, mf, weight=g)
        assert np.array_equal(full, mode_overlap(modes, mf, modes, mf, weight=g))
        G = mf.grams(modes, g)
        again = mf.grams(modes, g)
        assert all(np.array_equal(G[nm], again[nm]) for nm in G)
        subsets = _subsets()
        for I, J in zip(subsets, subsets[1:] + subsets[:1]):
            sub = mode_overlap([modes[i] for i in I], mf, [modes[j] for j in J], mf, weight=g)
            assert np.array_equal(sub, full[I][:, J]), (kind, len(I), len(J))
        for I in subsets[:3]:
            GI = mf.grams([modes[i] for i in I], g)
            for nm in G:
                assert np.array_equal(GI[nm], G[nm][I][:, I]), (kind, len(I), nm)


def test_sixty_five_cores_are_refused_at_the_c_abi(cases):
    mf = cases["sq"].mf
    mf._ensure_locator()
    lib = mf._lib
    import torch
    modes = cases["sq"].modes["scalar"][:3]
    staged, _ = mf._stage(vals(modes))
    cores = np.zeros((65, 3))
    cores[:, 2] = 0.01
    need = ctypes.c_int64(0)
    assert lib.plfem_gram_work_bytes(1, 3, ctypes.byref(need)) == _native.PLFEM_OK
    work = torch.empty(int(need.value) + 256, dtype=torch.uint8, device=mf.tdev)
    aligned = (work.data_ptr() + 255) & ~255
    out = np.zeros((3, 3, 3))
    rc = lib.plfem_mode_grams(mf._loc, 1, 3, ctypes.c_void_p(staged.data_ptr()), 0, cores.ctypes.data_as(ctypes.c_void_p),
                              65, ctypes.c_void_p(aligned), ctypes.c_int64(int(need.value)), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == _native.PLFEM_EINVAL and "64" in lib.plfem_locator_last_error(mf._loc).decode()
    assert lib.plfem_overlap_work_bytes(3, 3, ctypes.byref(need)) == _native.PLFEM_OK
    work = torch.empty(int(need.value) + 256, dtype=torch.uint8, device=mf.tdev)
    aligned = (work.data_ptr() + 255) & ~255
    o = np.zeros((3, 3))
    rc = lib.plfem_field_overlap(mf._loc, ctypes.c_void_p(staged.data_ptr()), 3, 0, mf._loc, ctypes.c_void_p(staged.data_ptr()),
                                 3, 0, 1, cores.ctypes.data_as(ctypes.c_void_p), 65, 2.0, 1.0, ctypes.c_void_p(aligned),
                                 ctypes.c_int64(int(need.value)), o.ctypes.data_as(ctypes.c_void_p))
    assert rc == _native.PLFEM_EINVAL and "64" in lib.plfem_locator_last_error(mf._loc).decode()
    assert (out == 0).all() and (o == 0).all()
    mf.stream.synchronize()


# -- closed form: quadratics are reproduced exactly by P2 and integrated exactly by the six-point rule ----------------
EXP = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2))        # monomials 1, x, y, x^2, xy, y^2


def _mono_gram():
    """G[i, j] = integral over the unit square of m_i m_j."""
    return np.array([[1.0 / ((a + c + 1) * (b + d + 1)) for (c, d) in EXP] for (a, b) in EXP])


def _derivative(axis):
    """D with coeffs(d f / d axis) = D @ coeffs(f)."""
    D = np.zeros((6, 6))
    for j, e in enumerate(EXP):
        if e[axis]:
            lower = list(e)
            lower[axis] -= 1
            D[EXP.index(tuple(lower)), j] = e[axis]
    return D


def _eval(C, x, y):
    return C @ np.array([x ** a * y ** b for a, b in EXP])


def _quadratic_records(mesh, C):
    dl = P2Basis(MeshTriLite(mesh.p, mesh.t)).doflocs
    return [{"field_vector": f} for f in _eval(C, dl[0], dl[1])]


def test_closed_form_quadratics_on_two_triangulations(gpu_device, built_library):
    meshes = (unit_square_mesh(6), jittered_square_mesh(6, seed=1))
    rng = np.random.default_rng(6)
    Cs = [rng.standard_normal((KMAX, 6)), rng.standard_normal((KMAX, 6))]
    mfs = [ModeFields(m, device=gpu_device) for m in meshes]
    recs = [_quadratic_records(m, C) for m, C in zip(meshes, Cs)]
    Gm = _mono_gram()
    Dx, Dy = _derivative(0), _derivative(1)
    g = spread_discs((0.0, 1.0, 0.0, 1.0))
    pts = rng.uniform(0, 1, (2, 2000))
    try:
        for mf, rec, C in zip(mfs, recs, Cs):
            u = mf.sample(rec, pts)["u"]
            ref = _eval(C, pts[0], pts[1])
            assert np.abs(u - ref).max() <= 1e-12 * np.abs(ref).max()
            G = mf.grams(rec, g)
            ff = C @ Gm @ C.T
            ss = C @ (Dx.T @ Gm @ Dx + Dy.T @ Gm @ Dy) @ C.T
            assert np.abs(G["M_core"] + G["M_clad"] - ff).max() <= 1e-12 * np.abs(ff).max()
            assert np.abs(G["S"] - ss).max() <= 1e-12 * np.abs(ss).max()
            assert np.abs(G["M_core"]).max() > 0.01 * np.abs(ff).max()      # the cores hold a real share
        for a, b in ((0, 1), (1, 0)):
            O = mode_overlap(recs[a], mfs[a], recs[b], mfs[b])
            ref = Cs[a] @ Gm @ Cs[b].T
            assert np.abs(O - ref).max() <= 1e-12 * np.abs(ref).max(), (a, b)
    finally:
        for mf in mfs:
            mf.close()


def test_nineteen_core_solve_past_one_chunk(gpu_device, built_library):
    g = MCFGeometry(19, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55)
    mesh = generate_mesh(g, 0.35, 0)
    solver = TrueVectorialMaxwellSolver(g, device=gpu_device, eig_tol=1e-10)
    t0 = time.perf_counter()
    modes = solver.solve_vectorial_modes(mesh, 40)
    mf = ModeFields(mesh, device=gpu_device, solver=solver)
    try:
        res = mode_dispersion(modes, mf, g)
        print(f"19 cores: {len(modes)} vectorial modes, rayleigh defect max {res['rayleigh_defect'].max():.2e}, "
              f"{time.perf_counter() - t0:.2f} s")
        assert len(modes) > 32
        assert res["rayleigh_defect"].max() <= 1e-10
        G = mf.grams(modes, g)
        ref = GramEmulation(mesh.p, mesh.t).grams(vals(modes), True, g)
        for nm in ref:
            assert np.abs(G[nm] - ref[nm]).max() <= 1e-12 * np.abs(ref[nm]).max(), nm
    finally:
        mf.close()
        solver.clear_cache()


# -- core-boundary ties ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ties(gpu_device, built_library):
    T = Ties(jittered_square_mesh(8))
    g = T.geometry()
    mf = ModeFields(T.mesh, device=gpu_device)
    yield {"T": T, "g": g, "core": T.core(g), "mf": mf}
    mf.close()


def _flip_report(T, core, got_core_weight):
    w = T.basis.dx
    return (f"reference core weight {w[core].sum():.17g}, device {got_core_weight:.17g}, "
            f"difference {(got_core_weight - w[core].sum()) / w.min():.3f} of the smallest weight")


def test_ties_core_mass_of_the_constant(ties):
    T, g, core, mf = ties["T"], ties["g"], ties["core"], ties["mf"]
    one = [{"field_vector": np.ones(mf.N)}]
    G = mf.grams(one, g)
    w = T.basis.dx
    print(_flip_report(T, core, G["M_core"][0, 0]))
    assert abs(G["M_core"][0, 0] - w[core].sum()) <= 1e-12 * w.sum()
    assert abs(G["M_clad"][0, 0] - w[~core].sum()) <= 1e-12 * w.sum()


def test_ties_weighted_overlap(ties):
    T, g, core, mf = ties["T"], ties["g"], ties["core"], ties["mf"]
    one = [{"field_vector": np.ones(mf.N)}]
    O = mode_overlap(one, mf, one, mf, weight=g)[0, 0]
    w = T.basis.dx
    ref = (w * np.where(core, 1 / g.n_core ** 2, 1 / g.n_clad ** 2)).sum()
    assert abs(O - ref) <= 1e-12 * w.sum(), (O - ref) / w.min()


def test_ties_assembled_minv_block(ties, gpu_device):
    T, g = ties["T"], ties["g"]
    sym = _native.Symbolic(T.mesh.p, T.mesh.t)
    ctx = _native.Context(sym, gpu_device, max_ncv=65)
    try:
        ctx.assemble(_core_table(g), g.n_core ** 2, g.n_clad ** 2, g.k0, 1.0)
        N = sym.N
        G = sp.csr_matrix((ctx.block_values("Minv"), sym.array("colind"), sym.array("rowptr")), shape=(N, N))
    finally:
        ctx.close()
    basis = P2Basis(MeshTriLite(T.mesh.p, T.mesh.t))
    em = hfield.element_matrices(g, basis)["mass_eps_inv"]
    R = hfield.assemble_hfield_system_fused(g, basis.mesh, eliminate_zeros=False)[6]
    ed = basis.element_dofs
    rows = np.broadcast_to(ed.T[:, :, None], em.shape).ravel()
    cols = np.broadcast_to(ed.T[:, None, :], em.shape).ravel()
    mag = np.broadcast_to(np.abs(em).max(axis=(1, 2), keepdims=True), em.shape)
    M = sp.coo_matrix((mag.ravel(), (rows, cols)), shape=(N, N)).tocsr()
    D = abs(G - R)
    D.eliminate_zeros()
    viol = D - 1e-13 * M
    assert viol.max() <= 0.0, D.max()
