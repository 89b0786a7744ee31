"""Results must not depend on what the device memory held before, on the calls made on a context earlier, or on the pinned
blocks, streams and events a context inherits from the process-wide pools.

* Prior contents: every buffer the Python host hands to the library (context slab, locator memory, work buffers, output
  tensors) is pre-filled through ``_native.SCRATCH_FILL`` with 0.0, a quiet NaN (caught wherever a value is read and
  multiplied by a structural zero, or accumulated) and 3e100 (finite: survives the comparisons a NaN hides).  One fixed
  script of ABI calls per case (workspace_cases.run_script), bit-identical results under every fill; the zero fill runs
  twice as the control of the comparison itself.  The NaN run's solve is also checked against SuperLU of the oracle's
  pencil, so that three equally wrong runs cannot pass.
* Call history: each sequence of earlier calls ends in a probe whose results equal, bit for bit, the probe on a new context.
* Recycling: a small context after a large one has come and gone, a context created straight after another was closed, and
  the same probe as the first context of a fresh process."""
import functools
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import pivot_cases as pc
import workspace_cases as wc
from pl_fem_vectoriel_amd import MCFGeometry, ModeFields, _native, generate_mesh, mode_overlap
from pl_fem_vectoriel_amd.solver_fem import _core_table, shift_estimate

pytestmark = pytest.mark.gpu
FILLED = ("nan", "huge")


def filled(fill_name, fn, *args):
    """fn(*args) with every scratch buffer and output pre-filled (monkeypatched for the duration of the call)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_native, "SCRATCH_FILL", wc.FILLS[fill_name])
        return fn(*args)


def assert_same(got, want, what):
    diff = wc.differences(got, want)
    assert not diff, (what, diff)


# ---- 2. prior contents: the solver ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scripts(c1_geometry, gpu_device, built_library):
    @functools.lru_cache(maxsize=None)
    def get(name, fill_name):
        return filled(fill_name, wc.run_script, wc.data(name, c1_geometry), gpu_device)
    return get


def test_the_fill_reaches_the_buffers(gpu_device, built_library):
    """The seam itself: None allocates and does nothing else; a value writes that bit pattern over the whole buffer, its size
    rounded up to 8 bytes, for scratch and for outputs of any dtype."""
    import torch
    tdev = torch.device("cuda", gpu_device)
    assert _native.SCRATCH_FILL is None
    assert _native.device_scratch(13, tdev).shape == (13,)
    assert _native.device_output((3, 5), torch.int32, tdev).shape == (3, 5)
    for name, value in wc.FILLS.items():
        want = np.array([value]).view(np.uint64)[0]
        s = filled(name, _native.device_scratch, 13, tdev)
        assert s.dtype == torch.uint8 and s.shape == (16,)
        assert (s.cpu().numpy().view(np.uint64) == want).all(), name
        o = filled(name, _native.device_output, (3, 5), torch.int32, tdev)
        assert o.dtype == torch.int32 and o.shape == (3, 5) and o.is_contiguous()
        assert (o.cpu().numpy().ravel()[:14].view(np.uint64) == want).all(), name
        d = filled(name, _native.device_output, (2, 3), torch.float64, tdev)
        assert (d.cpu().numpy().view(np.uint64) == want).all(), name


@pytest.mark.parametrize("name", wc.CASES)
def test_zero_fill_control_is_deterministic(scripts, name):
    """The zero fill twice: a difference here is a determinism finding of its own, not one of the fill.  Also what the
    script must reach: no perturbed pivot, a thick restart in both eigen-solves, finite factors, and the P = 1 solve after
    the P = 4 one (d_fvec in its P = 1 layout straight after the P = 4 layout) equal to the one before."""
    a, b = scripts(name, "zero"), scripts(name, "zero_again")
    assert_same(b, a, name)
    stats = wc.named(a["lanczos_stats"], wc.LANCZOS_STATS)
    assert stats["nconv"] == wc.K and stats["restarts"] >= 1 and stats["n_block_solves"] > 0, stats
    modes = wc.named(a["modes_stats"], wc.modes_stats_names())       # plfem_solve_modes depends on the d_BV / d_BV2 swap
    assert modes["nconv"] == wc.K and modes["restarts"] >= 1 and modes["n_block_solves"] > 0, modes
    assert modes["refined"] == 0 and modes["pivot_perturbations"] == 0, modes
    assert a["perturbations"][0] == 0 and a["factor_nonfinite"][0] == 0
    assert np.array_equal(a["solve_r0_again"], a["solve_r0"])
    assert all(np.isfinite(v).all() for v in a.values())


@pytest.mark.parametrize("fill", FILLED)
@pytest.mark.parametrize("name", wc.CASES)
def test_results_do_not_depend_on_workspace_contents(scripts, name, fill):
    assert_same(scripts(name, fill), scripts(name, "zero"), (name, fill))


@pytest.mark.parametrize("name", wc.CASES)
def test_nan_fill_solves_match_splu(scripts, name, c1_geometry):
    """The bar of test_shift_invert_solve_matches_splu on the NaN run: 1e-9 of the SuperLU solution with 0 and 1 refinement
    passes and through the block sweeps, Dirichlet entries exactly zero."""
    d = wc.data(name, c1_geometry)
    run = scripts(name, "nan")
    lu = spla.splu(d.pencil)
    n2 = d.n2
    cols = [d.rhs[k] for k in ("random", "leaf", "root", "random2")]
    got = [("r0", run["solve_r0"], cols[0]), ("r1", run["solve_r1"], cols[0]), ("again", run["solve_r0_again"], cols[0])]
    got += [(f"block {u}", run["solve_block"][u * n2:(u + 1) * n2], cols[u]) for u in range(4)]
    for what, x, b in got:
        xs = lu.solve(b[d.idx])
        rest = np.delete(x, d.idx)
        assert rest.size == 0 or np.abs(rest).max() == 0.0, (name, what)
        err = np.linalg.norm(x[d.idx] - xs) / np.linalg.norm(xs)
        assert err < 1e-9, (name, what, err)


# ---- 2. prior contents: the field kernels ------------------------------------------------------------------------------
K_FIELDS = 33            # one past the 32-mode chunk (test_gpu_field_shapes.py)


class FieldInputs:
    """Two meshes, seeded records of both kinds on each, sample points of every kind (host only)."""

    def __init__(self, g):
        def records(rng, kind, nrows, k):
            if kind == "vectorial":
                return [{"Ex_dofs": rng.standard_normal(nrows), "Ey_dofs": rng.standard_normal(nrows),
                         "beta": float(rng.uniform(5, 10))} for _ in range(k)]
            return [{"field_vector": rng.standard_normal(nrows)} for _ in range(k)]

        self.g = g
        self.fine, self.coarse = generate_mesh(g, 0.5, 0), generate_mesh(g, 1.0, 0)
        rng = np.random.default_rng(18)
        self.modes = {}
        for tag, mesh in (("fine", self.fine), ("coarse", self.coarse)):
            sym = _native.Symbolic(mesh.p, mesh.t)
            self.modes[tag] = {"vectorial": records(rng, "vectorial", sym.nsolve, K_FIELDS),
                               "scalar": records(rng, "scalar", sym.N, K_FIELDS)}
            if tag == "fine":
                dl = sym.array("doflocs").reshape(2, sym.N)
                nv = sym.nv
        p = self.fine.p
        x0, x1, y0, y1 = p[0].min(), p[0].max(), p[1].min(), p[1].max()
        w, h = x1 - x0, y1 - y0
        inside = np.vstack([rng.uniform(x0 + 0.3 * w, x1 - 0.3 * w, 57), rng.uniform(y0 + 0.3 * h, y1 - 0.3 * h, 57)])
        vertices, edges = dl[:, :nv][:, ::97], dl[:, nv:][:, ::211]           # mesh vertices, edge midpoints
        outside = np.array([[x0 - 0.1 * w, x1 + 0.2 * w, 0.5 * (x0 + x1), x0 - w, x1 + 1e-6 * w],
                            [0.5 * (y0 + y1), y1 + 0.1 * h, y0 - 0.3 * h, y1 + h, 0.5 * (y0 + y1)]])
        self.points = np.hstack([inside, vertices, outside, edges])
        self.outside = np.zeros(self.points.shape[1], dtype=bool)
        self.outside[inside.shape[1] + vertices.shape[1]:][:outside.shape[1]] = True
        self.xf = np.array([[0.0, 0.0, 0.3], [1.0, 0.05, 0.0], [-2.0, 0.0, -0.7], [0.5, 0.01, 1.1]])      # 4 x 3 far field
        self.yf = np.array([[0.0, 0.0, -0.2], [0.7, 0.03, 0.0], [0.0, 0.0, 0.9]])


def run_fields(fi, device):
    """Every field entry point on NEW ModeFields objects (locator memory, work buffers and outputs under the current fill)."""
    out = {}
    mf, mc = ModeFields(fi.fine, device=device), ModeFields(fi.coarse, device=device)
    try:
        for kind in ("vectorial", "scalar"):
            modes = fi.modes["fine"][kind]
            for nm, v in mf.sample(modes, fi.points).items():
                out[f"{kind}/sample/{nm}"] = v
            for nm, v in mf.sample_grid(modes, 5, 4).items():
                out[f"{kind}/grid/{nm}"] = v
            for nm, v in mf.grams(modes, fi.g).items():
                out[f"{kind}/gram/{nm}"] = v
            out[f"{kind}/quartic"] = mf.quartic(modes[:5], fi.g, (1.0, 0.25))
            out[f"{kind}/project"] = mf.project(modes, fi.xf, fi.yf)
            out[f"{kind}/overlap"] = mode_overlap(modes, mf, fi.modes["coarse"][kind], mc, weight=fi.g)
            out[f"{kind}/overlap_back"] = mode_overlap(fi.modes["coarse"][kind], mc, modes, mf)
    finally:
        mf.close()
        mc.close()
    return out


@pytest.fixture(scope="module")
def field_runs(c1_geometry, gpu_device, built_library):
    fi = FieldInputs(c1_geometry)

    @functools.lru_cache(maxsize=None)
    def get(fill_name):
        return filled(fill_name, run_fields, fi, gpu_device)
    get.inputs = fi
    return get


def test_field_zero_fill_control_is_deterministic(field_runs):
    a = field_runs("zero")
    assert_same(field_runs("zero_again"), a, "fields")
    assert a["vectorial/project"].shape == (2, K_FIELDS, 3, 4) and a["scalar/quartic"].shape == (15, 15)
    assert a["vectorial/overlap"].shape == (K_FIELDS, K_FIELDS) and a["scalar/grid/u"].shape == (K_FIELDS, 4, 5)


@pytest.mark.parametrize("fill", ("zero",) + FILLED)
def test_field_results_do_not_depend_on_buffer_contents(field_runs, fill):
    """Bit-identical to the zero fill (the zero run itself: the properties below only); every output entry written -- no
    float64 entry holds a NaN or 3e100 pre-fill, every int32 element entry lies in [-1, ne) (the halves of the two patterns
    read as int32 are 0, 0x7ff80000, 0xb85f253b (negative) and 0x54cb6e83: the last three are no element of these meshes, and a 0 left
    by the NaN pattern is caught by the bit comparison of the 3e100 run); a point outside the mesh gets element -1 and value
    0, a point inside an element, on an edge or on a vertex an element."""
    run, fi = field_runs(fill), field_runs.inputs
    if fill != "zero":
        assert_same(run, field_runs("zero"), fill)
    ne = fi.fine.t.shape[1]
    assert ne < 0x54cb6e83
    for key, v in run.items():
        if key.endswith("/element"):
            assert v.dtype == np.int32 and (v >= -1).all() and (v < ne).all(), (fill, key)
        else:
            assert v.dtype.kind in "fc" and np.isfinite(v).all() and (np.abs(v) < 1e50).all(), (fill, key)
    for kind, names in (("vectorial", ("Hx", "Hy", "Hz_im")), ("scalar", ("u",))):
        el = run[f"{kind}/sample/element"]
        assert el.dtype == np.int32 and (el[fi.outside] == -1).all() and (el[~fi.outside] >= 0).all(), (fill, kind)
        for nm in names:
            v = run[f"{kind}/sample/{nm}"]
            assert v.shape == (K_FIELDS, fi.points.shape[1])
            assert (v[:, fi.outside] == 0.0).all() and v[:, :57].any(axis=0).all(), (fill, kind, nm)
        g = run[f"{kind}/grid/element"]
        assert g.shape == (4, 5) and (g[0, 0] == -1) and (g >= 0).any()        # (the corner of the disc's bounding box)


# ---- 3. call history on one context --------------------------------------------------------------------------------------
HISTORY_CASE = "c1_h05_l24_vec"


@pytest.fixture(scope="module")
def fresh(c1_geometry, gpu_device, built_library):
    """Probes on NEW contexts (one context per probe, closed afterwards), computed once."""
    @functools.lru_cache(maxsize=None)
    def get(name, probe, *args):
        d = wc.data(name, c1_geometry)
        ctx = d.context(gpu_device)
        try:
            if probe == "modes":
                return wc.probe_modes(ctx, d)[0]
            d.assemble(ctx)
            if probe == "eigs":
                return wc.probe_eigs(ctx, d)
            ctx.factor(d.sigma)
            return wc.probe_solves(ctx, d, args)
        finally:
            ctx.close()
    return get


@pytest.fixture()
def history(c1_geometry, gpu_device, built_library):
    """(data, context) of a case for one sequence; the contexts are closed afterwards."""
    made = []

    def get(name=HISTORY_CASE):
        d = wc.data(name, c1_geometry)
        made.append(d.context(gpu_device))
        return d, made[-1]
    yield get
    for ctx in made:
        ctx.close()


def test_second_shift_after_a_lanczos_run(history, fresh):
    """factor(s1) -> lanczos leaves basis vectors in the union the next factorisation takes its Schur arenas and panels from."""
    d, ctx = history()
    d.assemble(ctx)
    wc.probe_eigs(ctx, d, sigma=0.97 * d.sigma)
    assert_same(wc.probe_eigs(ctx, d), fresh(HISTORY_CASE, "eigs"), "second shift")


def test_solve_modes_after_another_cross_section(history, fresh):
    """solve_modes at another wavelength and core radius on the same mesh, then the probe's own cross-section."""
    d, ctx = history()
    other = MCFGeometry(7, 8.0, 1.3, 1.535, 1.0, wavelength_um=1.31)
    first, _ = wc.probe_modes(ctx, d, cores=_core_table(other), k0=other.k0, sigma=shift_estimate(other))
    want = fresh(HISTORY_CASE, "modes")
    assert not np.array_equal(first["evals"], want["evals"])
    got, st = wc.probe_modes(ctx, d)
    assert_same(got, want, "second cross-section")
    assert st["pivot_perturbations"] == 0 and st["refined"] is False


@pytest.mark.parametrize("tree,perturb", [("sq10_l16_vec", 1e-6), ("sq16_l32_sca", 1e-4)])
def test_clean_pencil_after_replaced_pivots_and_a_refined_pass(history, fresh, c1_geometry, tree, perturb):
    """Earlier: a planted pencil of pivot_cases.py whose pairs are replaced (counted, D^-1 holds the replacements), solved with
    a refinement pass; then a solve_modes whose a-posteriori check fails on a perturbed factor (D^-1 of the root front scaled
    by 1 + perturb: enough for the first pass to miss the bound, little enough for one refinement pass to meet it), so that its
    refined second pass runs (refine_steps raised inside the call).  The clean probe: no perturbation, not refined, and the bits of a new
    context -- which also says that refine_steps is back at the caller's 0 (a first pass with refinement gives other bits)."""
    d, ctx = history(tree)
    ref = pc.reference(f"{tree}:all_at_once", c1_geometry)
    d.assemble(ctx)
    ctx.debug_set_elements(pc.tree_data(tree, c1_geometry).device_elements(ref.Ke))
    ctx.factor(0.0)
    assert ctx.timings()["pivot_perturbations"] == ref.count > 0
    b = wc.dev(ctx, d.rhs["random"])
    assert np.isfinite(ctx.solve(b, 1).cpu().numpy()).all()
    wc.probe_solves(ctx, d, ("block",))
    ctx.debug_set_perturb(perturb)
    try:
        _, st = wc.probe_modes(ctx, d)
    finally:
        ctx.debug_set_perturb(0.0)
    assert st["refined"] is True and st["true_residual_first"] > wc.RESIDUAL_TOL >= st["true_residual"]
    got, st = wc.probe_modes(ctx, d)
    assert st["pivot_perturbations"] == 0 and st["refined"] is False
    assert_same(got, fresh(tree, "modes"), tree)
    d.assemble(ctx)
    assert_same(wc.probe_eigs(ctx, d), fresh(tree, "eigs"), (tree, "refine_steps"))


def test_normal_call_after_no_convergence(history, fresh):
    d, ctx = history()
    d.assemble(ctx)
    ctx.factor(d.sigma)
    with pytest.raises(_native.ArpackLikeNoConvergence) as ei:
        ctx.lanczos(wc.K, wc.NCV, wc.TOL, 1, d.sigma)
    assert ei.value.stats["restarts"] == 1 and ei.value.stats["nconv"] < wc.K
    # the same through plfem_solve_modes: the exception carries the current Ritz pairs (Context.modes_dev)
    with pytest.raises(_native.ArpackLikeNoConvergence) as ei:
        ctx.solve_modes(d.cores, d.eps_core, d.eps_clad, d.k0, d.alpha_p, d.sigma, wc.K, wc.NCV, wc.TOL, 1, wc.RESIDUAL_TOL,
                        d.tol_refined)
    assert tuple(ei.value.eigenvectors.shape) == (wc.K, d.n2) and ei.value.stats["nconv"] < wc.K
    assert_same(wc.probe_eigs(ctx, d), fresh(HISTORY_CASE, "eigs"), "after PLFEM_ENOCONV")


def test_scalar_solve_after_cmt_coupling(history, fresh):
    """plfem_cmt_coupling borrows the MINV slot, counters[2] (the Lanczos rank flag) and d_Hcols: the context refuses every
    call that needs the pencil until it is assembled again, the flag is back at 0, and the reassembled context is a new one."""
    import torch
    name = "c1_h05_l24_sca"
    d, ctx = history(name)
    d.assemble(ctx)
    ctx.factor(d.sigma)
    rng = np.random.default_rng(3)
    fi, fj = (torch.from_numpy(rng.standard_normal((5, d.n2))).to(ctx.tdev) for _ in range(2))
    ctx.cmt_coupling(fi, fj, d.cores, d.eps_core, d.eps_clad)
    b = wc.dev(ctx, d.rhs["random"])
    for call in (lambda: ctx.factor(d.sigma), lambda: ctx.solve(b, 0), lambda: ctx.spmv("A", b), lambda: ctx.spmv("B", b),
                 lambda: ctx.residuals(np.ones(1), b.reshape(1, -1))):
        with pytest.raises(RuntimeError):
            call()
    assert not ctx.debug_copy("counters", 0, 4)[2:].any()
    d.assemble(ctx)
    assert_same(wc.probe_eigs(ctx, d), fresh(name, "eigs"), "after cmt_coupling")
    ctx.factor(d.sigma)
    assert_same(wc.probe_solves(ctx, d, ("single", "block")), fresh(name, "solves", "single", "block"), "after cmt_coupling")


@pytest.mark.parametrize("order", [("block", "single"), ("single", "block")])
def test_single_and_block_solves_in_either_order(history, fresh, order):
    """One factor; d_fvec and its siblings go from the P = 4 layout to the P = 1 layout and back."""
    d, ctx = history()
    d.assemble(ctx)
    ctx.factor(d.sigma)
    got = wc.probe_solves(ctx, d, order + order)
    want = fresh(HISTORY_CASE, "solves", "single", "block")
    assert_same(got, want, order)
    assert_same(wc.probe_solves(ctx, d, order[::-1]), want, order[::-1])


# ---- 4. recycled process-wide resources ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_after_large(c1_geometry, gpu_device, built_library):
    """(B first, B after A): B = the small context (max_ncv 12), A = a large one (c1_h10_vec, max_ncv 65) created, used and
    closed while the first B is still open -- so the second B cannot get the first one's pinned block back and takes, best
    fit, a larger one with its old PIN_* contents, and A's streams and events."""
    d = wc.data(wc.SMALL, c1_geometry)
    first_ctx = d.context(gpu_device, max_ncv=wc.SMALL_NCV)
    try:
        first = wc.probe_modes(first_ctx, d, wc.SMALL_K, wc.SMALL_NCV)[0]
        a = wc.data(wc.LARGE, c1_geometry)
        actx = a.context(gpu_device)
        try:
            big, _ = wc.probe_modes(actx, a)
            assert np.isfinite(big["evals"]).all()
        finally:
            actx.close()
        second = wc.small_probe(gpu_device, c1_geometry)
    finally:
        first_ctx.close()
    return first, second


def test_small_context_after_a_large_one(small_after_large):
    first, second = small_after_large
    assert np.isfinite(first["modes_int"]).all()
    assert_same(second, first, "B after A")


def test_small_context_matches_a_fresh_process(small_after_large, tmp_path, gpu_device):
    """The same probe as the first context of a new process (empty pools, a new allocator): one child, no exec."""
    out = tmp_path / "probe.npz"
    flags = ["-s"] if sys.flags.no_user_site else []
    res = subprocess.run([sys.executable, *flags, wc.__file__, str(out), str(gpu_device)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    with np.load(out) as z:
        child = {k: z[k] for k in z.files}
    assert_same(small_after_large[1], child, "B in a fresh process")


def test_context_created_straight_after_a_close(c1_geometry, gpu_device, built_library):
    """A context closed at once (its staged upload may still be in flight) and another created immediately on a different
    mesh of similar upload size, so that it takes the staging block just released: its device-built colind / slot_row are
    the host's, its block values those of an undisturbed third context."""
    a, b = wc.data("c1_h05_l24_vec", c1_geometry), wc.data(wc.SAME_SIZE_SQUARE.name, c1_geometry)
    assert a.sym.ne == b.sym.ne and not np.array_equal(a.sym.array("edof"), b.sym.array("edof"))
    for first, second in ((a, b), (b, a)):
        first.context(gpu_device).close()
        ctx = second.context(gpu_device)
        try:
            nnz = second.sym.nnz
            assert np.array_equal(ctx.debug_copy("colind", 0, nnz), second.sym.array("colind").astype(np.float64))
            assert np.array_equal(ctx.debug_copy("slot_row", 0, nnz), second.sym.array("slot_row").astype(np.float64))
            second.assemble(ctx)
            got = {n: ctx.block_values(n) for n in _native.BLOCKS}
        finally:
            ctx.close()
        third = second.context(gpu_device)
        try:
            second.assemble(third)
            assert_same(got, {n: third.block_values(n) for n in _native.BLOCKS}, second.name)
        finally:
            third.close()
