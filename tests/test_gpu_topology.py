"""The device kernels on meshes that are no disc and no square (topology_cases.py): a hole, two parts, two parts that meet
in one vertex, a strip one element wide.  Pattern, assembly and sparse products against the oracle; the two Lanczos
drivers end to end on a two-part section, a holed one and one whose every eigenvalue is double, against a dense
eigensolve of the oracle's pencil; the field kernels (sampling, overlap, posed overlap, error indicators) against their
NumPy emulations at the hole's rim, in the hole, in the gap and at the pinch vertex.  Every bound is that of the existing
test of the same kernel, imported from there.  (The factorisation and the sweeps on these meshes: the topology cases of
operator_cases.py in test_gpu_operator_forms.py.)"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import front_emulation as fe
import lanczos_emulation as le
import operator_cases as oc
import topology_cases as tc
from assembly_checks import check_blocks, scalar_refs, vectorial_refs
from fields_emulation import overlap as em_overlap
from indicator_emulation import IndicatorEmulation, eps_of
from oracle import hfield, scalar
from oracle.p2 import MeshTriLite, P2Basis
from pl_fem_vectoriel_amd import ModeFields, _native, mode_overlap, mode_overlap_poses
from pl_fem_vectoriel_amd.solver_fem import _core_table
from pose_overlap_emulation import IDENTITY, posed_overlap
from test_gpu_field_shapes import OVERLAP_TOL, SAMPLE_TOL, records, vals
from test_gpu_fields import ANY_DOF_TOL, OWN_DOF_TOL
from test_gpu_indicators import ALPHA, K0, TOL as INDICATOR_TOL, material_args
from test_gpu_lanczos_drivers import TOL as EIG_TOL, check_converged, check_pairs, maxiter_of, solve
from test_gpu_parity import SPMV_TOL
from test_gpu_pose_overlap import POSED_TOL

pytestmark = pytest.mark.gpu
PENCILS = (2, 1)
LEAF = 24                           # the analyses of this file (their structural facts: topology_cases.EXPECT)
K, NCV = 12, 28                     # the tight basis of test_gpu_lanczos_drivers.TIGHT


def kind_of(dpn):
    return "vec" if dpn == 2 else "sca"


def geometry_of(name, c1_geometry):
    return tc.two_core_geometry() if name in ("twins", "pair") else c1_geometry


# ---- assembled contexts ------------------------------------------------------------------------------------------------
class Section:
    """A topology mesh under one pencil: analysis, assembled context, the oracle's pencil on full-length vectors."""

    def __init__(self, name, dpn, device, g):
        import torch
        self.torch, self.name, self.dpn, self.g = torch, f"{name}_{kind_of(dpn)}", dpn, g
        self.mesh = tc.trimesh(name)
        self.sym = _native.Symbolic(self.mesh.p, self.mesh.t, leaf_elems=LEAF, dofs_per_node=dpn, dirichlet=dpn == 2)
        self.ctx = _native.Context(self.sym, device, max_ncv=65)
        if dpn == 2:
            self.ctx.assemble(_core_table(g), g.n_core ** 2, g.n_clad ** 2, g.k0, 1.0)
        else:
            self.ctx.assemble_scalar(_core_table(g), g.n_core ** 2, g.n_clad ** 2, g.k0)
        self.N, self.n2 = self.sym.N, self.ctx.n2
        _K, self.idx, self.sigma, self.A_int, self.B_int, self.Ke = oc.host_pencil(self.sym, self.mesh, g, dpn)
        E = sp.csr_matrix((np.ones(self.idx.size), (self.idx, np.arange(self.idx.size))), shape=(self.n2, self.idx.size))
        self._full = {"A": (E @ self.A_int @ E.T).tocsr(), "B": (E @ self.B_int @ E.T).tocsr()}
        self.pencil = self                  # (check_converged reads c.pencil.matrix("B"))

    def matrix(self, which):
        return self._full[which]

    def live_rows(self):
        live = np.zeros(self.n2, dtype=bool)
        live[self.idx] = True
        return live

    def embed(self, v):
        full = np.zeros(self.n2)
        full[self.idx] = v
        return self.torch.from_numpy(full).cuda(self.ctx.device)

    @functools.cached_property
    def dense(self):
        """(lam, X, components): dense scipy.linalg.eigh of the oracle's restricted pencil, nearest sigma first."""
        return le.dense_reference(self._full["A"], self._full["B"], self.live_rows(), self.sigma)

    @functools.cached_property
    def emulated_replacements(self):
        """Pivots the emulation of the factorisation at sigma replaces on this tree."""
        logs = {}
        fe.factor(fe.FrontTree(self.sym), self.Ke, logs=logs)
        return sum(len(v) for v in logs.values())


@pytest.fixture(scope="module")
def sections(c1_geometry, gpu_device, built_library):
    @functools.lru_cache(maxsize=None)
    def get(name, dpn):
        return Section(name, dpn, gpu_device, geometry_of(name, c1_geometry))
    yield get
    import torch
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ["annulus", "bowtie", "comb"])
def test_device_built_pattern_equals_the_hosts(sections, name):
    s = sections(name, 2)
    nnz = s.sym.info["nnz"]
    np.testing.assert_array_equal(s.ctx.debug_copy("colind", 0, nnz).astype(np.int64), s.sym.array("colind"))
    np.testing.assert_array_equal(s.ctx.debug_copy("slot_row", 0, nnz).astype(np.int64), s.sym.array("slot_row"))


@pytest.mark.parametrize("dpn", PENCILS, ids=kind_of)
@pytest.mark.parametrize("name", ["annulus", "bowtie", "strip1"])
def test_assembled_blocks_match_oracle(sections, name, dpn):
    s = sections(name, dpn)
    g, om = s.g, MeshTriLite(s.mesh.p, s.mesh.t)
    basis = P2Basis(om)
    if dpn == 2:
        A, _B, _, Dxx, Dyy, Dxy, Minv = hfield.assemble_hfield_system_fused(g, om, eliminate_zeros=False)
        refs = vectorial_refs(A, Minv, Dxx, Dxy, Dyy, hfield.element_matrices(g, basis), g.k0 ** 2, s.N)
    else:
        Kst, M, Me, basis = scalar.assemble(g, om, eliminate_zeros=False)
        refs = scalar_refs(Kst, M, Me, scalar.element_matrices(g, basis), g.k0 ** 2)
    worst = check_blocks(s.ctx, s.sym, basis, refs)
    print(f"\n{s.name}: worst slot error {worst:.2e} of its magnitude (bound 1e-13)")


@pytest.mark.parametrize("dpn", PENCILS, ids=kind_of)
@pytest.mark.parametrize("name", ["annulus", "bowtie", "strip1"])
def test_spmv_matches_restricted_pencil(sections, name, dpn):
    s = sections(name, dpn)
    x = np.random.default_rng(0).standard_normal(len(s.idx))
    xd = s.embed(x)
    for which, M in (("A", s.A_int), ("B", s.B_int)):
        y = s.ctx.spmv(which, xd).cpu().numpy()
        ref = M @ x
        err = np.abs(y[s.idx] - ref).max() / (abs(M) @ np.abs(x)).max()
        print(f"\n{s.name} {which}: {err:.2e}")
        assert err <= SPMV_TOL
        rest = np.delete(y, s.idx)
        assert (rest.size > 0) == (dpn == 2)
        assert not rest.any()                                          # Dirichlet rows exactly 0


# ---- modes, end to end -------------------------------------------------------------------------------------------------
def check_replacements(s):
    """The factorisation the solve ran on replaced the pivots the emulation replaces: none, on these sections."""
    assert s.ctx.timings()["pivot_perturbations"] == s.emulated_replacements
    return s.emulated_replacements


@pytest.mark.parametrize("driver", ["block", "single"])
@pytest.mark.parametrize("dpn", PENCILS, ids=kind_of)
@pytest.mark.parametrize("name", ["pair", "annulus"])
def test_modes_match_the_dense_reference(sections, monkeypatch, name, dpn, driver):
    """The K pairs nearest sigma: each Ritz value within le.theta_bound, fields within FIELD_TOL with GAP_TOL clustering,
    B-orthonormal, Dirichlet rows 0, the same bits on a repeat (test_gpu_lanczos_drivers.check_converged)."""
    s = sections(name, dpn)
    if name == "pair":
        assert s.dense[2] == 2 and tc.EXPECT[(name, dpn, LEAF)]["root_fs"] == 0
    check_converged(s, monkeypatch, driver, K, NCV, min_restarts=0)
    print(f"pivots replaced: {check_replacements(s)}")


def doublets(s):
    lam = s.dense[0]
    assert s.dense[2] == 2 and lam.size % 2 == 0
    two = np.sort(lam[:K]).reshape(K // 2, 2)
    assert (np.ptp(two, axis=1) <= 1e-9 * np.abs(two[:, 0])).all()      # the K nearest sigma come in pairs
    return two


@pytest.mark.parametrize("dpn", PENCILS, ids=kind_of)
def test_block_driver_returns_both_copies_of_every_doublet(sections, monkeypatch, dpn):
    """twins: every eigenvalue twice (two equal parts), the root of the tree empty.  The rule of
    test_block_driver_returns_every_copy_of_a_triplet."""
    s = sections("twins", dpn)
    assert tc.EXPECT[("twins", dpn, LEAF)]["root_fs"] == 0
    doublets(s)
    check_converged(s, monkeypatch, "block", K, NCV, min_restarts=0)
    check_replacements(s)


@pytest.mark.parametrize("dpn", PENCILS, ids=kind_of)
def test_single_vector_driver_on_doublets_returns_true_pairs(sections, monkeypatch, dpn):
    """The rule of test_single_vector_driver_on_triplets_returns_true_pairs: every returned value is a reference eigenvalue
    within the bound, none more often than its multiplicity, the pairs are B-orthonormal; copies may be missing (the limit
    of a one-vector Krylov space, not asserted away)."""
    s = sections("twins", dpn)
    doublets(s)
    evals, evecs, st = solve(s, monkeypatch, "single", K, NCV, maxiter_of(s))
    assert st["nconv"] == K and st["n_block_solves"] == 0
    assert (np.diff(evals) >= 0).all()
    lam_all = np.sort(s.dense[0])                          # ascending: the two copies of a doublet are neighbours
    th_ref = 1.0 / (lam_all - s.sigma)
    th = 1.0 / (evals - s.sigma)
    bound = le.theta_bound(th_ref, EIG_TOL)
    hit = np.abs(th[:, None] - th_ref[None, :]) <= bound[None, :]
    assert hit.any(axis=1).all(), "a returned value is no eigenvalue of the pencil"
    counts = np.bincount(hit.argmax(axis=1) // 2)
    print(f"\n[doublets] {s.name} single ({K}, {NCV}): copies returned per doublet {counts[counts > 0].tolist()}, "
          f"restarts {st['restarts']}")
    assert counts.max() <= 2
    check_pairs(s, evals, evecs, K)
    check_replacements(s)


# ---- field kernels -----------------------------------------------------------------------------------------------------
KF = 5                              # modes per record set (past-one-chunk counts: test_gpu_field_shapes.py)


class Fields:
    def __init__(self, name, device, seed):
        self.name = name
        self.mesh = tc.trimesh(name)
        self.mf = ModeFields(self.mesh, device=device)
        self.em = IndicatorEmulation(self.mesh.p, self.mesh.t)
        rng = np.random.default_rng(seed)
        self.modes = {"vectorial": records(rng, "vectorial", self.mf.nsolve, KF), "scalar": records(rng, "scalar", self.mf.N, KF)}
        self.lam = {"vectorial": (K0 * rng.uniform(1.2, 1.5, KF)) ** 2, "scalar": -(K0 * rng.uniform(1.2, 1.5, KF)) ** 2}


@pytest.fixture(scope="module")
def fields(gpu_device, built_library):
    out = {name: Fields(name, gpu_device, 40 + i) for i, name in enumerate(tc.FIELD_MESHES + ("full",))}
    yield out
    for f in out.values():
        f.mf.close()
    import torch
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", tc.FIELD_MESHES)
def test_sampling_at_own_doflocs_returns_dof_values(fields, name):
    """Every DOF location of the mesh, the nodes on the hole's rim and the pinch vertex among them: the point goes to an
    element of its DOF -- the one the emulation's tie rule names -- and the DOF value comes back."""
    F = fields[name]
    mf = F.mf
    dl = mf.sym.array("doflocs").reshape(2, mf.N)
    interior = mf.sym.array("interior")
    edof = mf.sym.array("edof").reshape(6, mf.ne)
    e_em, _, _, near = F.em.locate(dl)
    rim = np.unique(edof[:, (F.em.nbr < 0).any(axis=0)])
    out = mf.sample(F.modes["vectorial"], dl)
    e = out["element"]
    assert (e >= 0).all()
    own = (edof[:, e] == np.arange(mf.N)[None]).any(0)
    assert own.all()                                    # (no slivers here: within the locator's tolerance of an element = on it)
    assert ((e == e_em) | (near >= 2)).all()
    on_rim_edge = np.intersect1d(rim, np.nonzero(near == 1)[0])        # midpoints of rim edges: one element, no tie
    assert on_rim_edge.size >= 24 and (e[on_rim_edge] == e_em[on_rim_edge]).all()
    if name == "bowtie":
        v0 = int(np.nonzero((dl[0] == 0.0) & (dl[1] == 0.0))[0][0])
        fan = np.nonzero((edof[:3] == v0).any(axis=0))[0]
        assert fan.size == near[v0] and e_em[v0] == fan.min()
        assert e[v0] == e_em[v0], (e[v0], fan)            # the smallest id of the fan around the pinch, from either part
    worst = 0.0
    for comp, key in (("Hx", "Ex_dofs"), ("Hy", "Ey_dofs")):
        ref = np.zeros((KF, mf.N))
        ref[:, interior] = np.array([m[key] for m in F.modes["vectorial"]])
        err = np.abs(out[comp] - ref).max(0) / np.abs(ref).max()
        worst = max(worst, err.max())
        assert (err[own] <= OWN_DOF_TOL).all() and err.max() <= ANY_DOF_TOL
    u = mf.sample(F.modes["scalar"], dl)["u"]
    ref = np.array([m["field_vector"] for m in F.modes["scalar"]])
    err = np.abs(u - ref).max(0) / np.abs(ref).max()
    worst = max(worst, err.max())
    assert (err[own] <= OWN_DOF_TOL).all() and err.max() <= ANY_DOF_TOL
    print(f"\n{name}: worst error at own DOF locations {worst:.2e} (bound {OWN_DOF_TOL:.0e}); {rim.size} rim nodes")


@pytest.mark.parametrize("name", tc.FIELD_MESHES)
def test_sampling_in_the_void_on_the_rim_and_at_the_pinch(fields, name):
    F = fields[name]
    mf, em = F.mf, F.em
    pts = tc.probe_points(name)
    P = np.hstack(list(pts.values()))
    at = dict(zip(pts, np.split(np.arange(P.shape[1]), np.cumsum([v.shape[1] for v in pts.values()])[:-1])))
    loc = em.locate(P)
    e_em, near = loc[0], loc[3]
    worst = 0.0
    for kind in ("vectorial", "scalar"):
        indexed = kind == "vectorial"
        names = ("Hx", "Hy", "Hz_im") if indexed else ("u",)
        modes = F.modes[kind]
        beta = np.array([m["beta"] for m in modes]) if indexed else None
        ref, _ = em.sample(vals(modes), P, indexed, beta=beta, located=loc)
        out = mf.sample(modes, P)
        e = out["element"]
        same = e == e_em
        assert (same | (near >= 2)).all(), kind
        assert (e[(e_em < 0) & (near == 0)] == -1).all()
        # in the hole, in the gap, outside the bounding box: no element, every value exactly 0
        assert (e[at["void"]] == -1).all()
        # on a rim edge: the one element that has it; at the pinch vertex: the smallest id of its fan
        assert (e[at["rim"]] == e_em[at["rim"]]).all() and (e[at["rim"]] >= 0).all()
        if "pinch" in at:
            assert e[at["pinch"][0]] == e_em[at["pinch"][0]] >= 0
            assert (e[at["pinch"]] >= 0).all()
        for c, nm in enumerate(names):
            scale = np.abs(ref[c]).max()
            cols = same if nm == "Hz_im" else slice(None)          # the gradient jumps across elements
            err = np.abs(out[nm][:, cols] - ref[c][:, cols]).max(initial=0.0) / scale
            worst = max(worst, err)
            assert err <= SAMPLE_TOL, (kind, nm, err)
            assert (out[nm][:, e < 0] == 0).all() and (out[nm][:, at["void"]] == 0).all()
    print(f"\n{name}: worst sampling error {worst:.2e} (bound {SAMPLE_TOL:.0e}); {int((near >= 2).sum())} of {P.shape[1]} "
          f"points near two elements")


@pytest.mark.parametrize("a,b", [("annulus", "full"), ("full", "annulus"), ("islands", "annulus")])
def test_overlap_across_holes_and_gaps(fields, c1_geometry, a, b):
    """B's quadrature points in A's hole or gap contribute 0; A's values come from elements on its rim."""
    FA, FB = fields[a], fields[b]
    qloc = FA.em.locate(FB.em.quadrature()[0])
    missed = int((qloc[0] < 0).sum())
    assert (missed > 100) == (a != "full")            # the holed A leaves points of B without an element
    worst = 0.0
    for kind in ("vectorial", "scalar"):
        for w in (None, c1_geometry):
            ref = em_overlap(FA.em, vals(FA.modes[kind]), FB.em, vals(FB.modes[kind]), kind == "vectorial", weight=w, located=qloc)
            O = mode_overlap(FA.modes[kind], FA.mf, FB.modes[kind], FB.mf, weight=w)
            assert O.shape == ref.shape == (KF, KF)
            err = np.abs(O - ref).max() / np.abs(ref).max()
            worst = max(worst, err)
            assert err <= OVERLAP_TOL, (kind, w is not None, err)
            assert np.array_equal(O, mode_overlap(FA.modes[kind], FA.mf, FB.modes[kind], FB.mf, weight=w))
    print(f"\n{a} on {b}: worst overlap error {worst:.2e} (bound {OVERLAP_TOL:.0e}); {missed} points of B outside A")


HOLE_OVER_MATERIAL = (6.0, -4.0, float(np.cos(0.3)), float(np.sin(0.3)), 0.8)      # A's hole lands on B around (6, -4)


def test_posed_overlap_moves_the_hole_over_material(fields, c1_geometry):
    FA, FB = fields["annulus"], fields["full"]
    poses = (IDENTITY, HOLE_OVER_MATERIAL)
    worst = 0.0
    for kind in ("vectorial", "scalar"):
        for w in (None, c1_geometry):
            O = mode_overlap_poses(FA.modes[kind], FA.mf, FB.modes[kind], FB.mf, np.array(poses), weight=w)
            assert O.shape == (2, KF, KF)
            for ip, pose in enumerate(poses):
                ref, elem = posed_overlap(FA.em, vals(FA.modes[kind]), FB.em, vals(FB.modes[kind]), kind == "vectorial", pose, weight=w)
                # points of B that the pose puts into A's hole: inside A's outline, in no element
                qa = np.vstack([(pose[2] * (FB.em.quadrature()[0][0] - pose[0]) + pose[3] * (FB.em.quadrature()[0][1] - pose[1])) / pose[4],
                                (pose[2] * (FB.em.quadrature()[0][1] - pose[1]) - pose[3] * (FB.em.quadrature()[0][0] - pose[0])) / pose[4]])
                in_hole = np.hypot(qa[0], qa[1]) < 3.0
                assert in_hole.sum() >= 60 and (elem[in_hole] < 0).all()
                err = np.abs(O[ip] - ref).max() / np.abs(ref).max()
                worst = max(worst, err)
                assert err <= POSED_TOL, (kind, w is not None, ip, err)
    print(f"\nannulus posed on full: worst error {worst:.2e} (bound {POSED_TOL:.0e})")


@pytest.mark.parametrize("kind", ["vectorial", "scalar"])
@pytest.mark.parametrize("name", tc.FIELD_MESHES)
def test_indicators_match_emulation(fields, c1_geometry, name, kind):
    """Rim edges (elem_nbr = -1 at an inner boundary) count as outer boundary: weight 1 scalar, 0 vectorial, as the
    emulation has it; the same bits on a repeat."""
    F = fields[name]
    F.mf._ensure_locator()
    v = np.ascontiguousarray(vals(F.modes[kind]))
    staged, _src = F.mf._stage(v)
    got = F.mf._indicators_staged(kind, staged, F.lam[kind], K0, ALPHA, *material_args(c1_geometry))
    want = F.em.eta2(v, kind == "vectorial", F.lam[kind], K0, ALPHA, eps_of(c1_geometry))
    assert got.shape == want.shape == (KF, F.mesh.t.shape[1])
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    err = np.abs(got - want).max() / np.abs(want).max()
    # the rim carries a real share: what weight 1 / 2 (scalar) or 1 (vectorial) on the rim edges would change
    P = F.em.pieces(v, kind == "vectorial", F.lam[kind], K0, ALPHA, eps_of(c1_geometry))
    bnd = F.em.nbr < 0
    assert bnd.sum() == tc.rim_edges(F.mesh.t).shape[1]
    on_rim = bnd.any(axis=0)
    extra = 0.5 * np.einsum("le,ckleg->ke", bnd * 1.0, P["flux"][0] ** 2)
    assert np.all(extra[:, on_rim] > 1e-6 * want[:, on_rim])          # (six orders above the bound: a wrong weight shows)
    print(f"\n{name} {kind}: indicator error {err:.2e} of the largest output (bound {INDICATOR_TOL:.0e}); "
          f"{int(on_rim.sum())} elements on the rim")
    assert err <= INDICATOR_TOL
    staged, _src = F.mf._stage(v)
    assert np.array_equal(F.mf._indicators_staged(kind, staged, F.lam[kind], K0, ALPHA, *material_args(c1_geometry)), got)
