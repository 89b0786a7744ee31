"""Host checks of the meshes with holes, gaps and pinches (topology_cases.py): each analysis has the structural facts it
is in the tests for, its front tree is a valid elimination structure, the NumPy emulation of the factorisation on it
solves both pencils to the accuracy of SuperLU, the sparsity pattern is the union pattern, the neighbour table is the
emulation's, and the sampling points of the GPU tests leave at most 5 % to the rule for points near two elements."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import front_emulation as fe
import operator_cases as oc
import topology_cases as tc
from front_checks import FWD_TOL, backward_error, check_tree_invariants, owned_dofs, right_hand_sides, shallowest_owner
from indicator_emulation import IndicatorEmulation
from pl_fem_vectoriel_amd import _native
from pl_fem_vectoriel_amd.mesh import TriMesh

KEYS = sorted(tc.EXPECT)
IDS = [f"{n}-{'vec' if d == 2 else 'sca'}-l{leaf}" for n, d, leaf in KEYS]


@functools.lru_cache(maxsize=None)
def analysis(name, dpn, leaf):
    p, t = tc.mesh(name)
    return _native.Symbolic(p, t, leaf_elems=leaf, dofs_per_node=dpn, dirichlet=dpn == 2)


def geometry_of(name, c1_geometry):
    return tc.two_core_geometry() if name in ("twins", "pair") else c1_geometry


def test_meshes_are_what_the_cases_say(built_library):
    sizes = {}
    for name in tc.NAMES:
        p, t = tc.mesh(name)
        p2, t2 = tc.mesh(name)
        assert np.array_equal(p, p2) and np.array_equal(t, t2)                    # deterministic
        assert np.array_equal(np.unique(t), np.arange(p.shape[1]))                # every vertex used, ids compact
        assert np.array_equal(TriMesh(p, t).t, t)                                 # columns sorted, as the package keeps them
        sizes[name] = (analysis(name, 1, 24).N, t.shape[1])
    assert sizes["annulus"] == (978, 446) and sizes["islands"][0] == 858 and sizes["comb"][0] == 777
    assert sizes["bowtie"][0] == 337 and sizes["tiny2"] == (9, 2)
    assert sizes["strip1"][1] == 80 and sizes["strip2"][1] == 160
    assert max(n for n, _ in sizes.values()) <= 1000
    # strip1, vectorial: every vertex is on the boundary, the 158 unknowns sit on edge midpoints
    sym = analysis("strip1", 2, 4)
    nv = tc.mesh("strip1")[0].shape[1]
    assert sym.array("bmask")[:nv].all() and 2 * sym.info["nsolve"] == 158
    assert 2 * analysis("tiny2", 2, 0).info["nsolve"] == 2
    # graded: the bisection around one point spreads the element areas over three orders of magnitude
    spread = tc.area_spread(*tc.mesh("graded"))
    print(f"\ngraded: largest / smallest element area = {spread:.4g}")
    assert spread >= 1000.0
    # bowtie: one vertex shared by two parts that share no edge
    p, t = tc.mesh("bowtie")
    v0 = np.nonzero((p[0] == 0.0) & (p[1] == 0.0))[0]
    assert v0.size == 1
    fan = t[:, (t == v0[0]).any(axis=0)]
    cen = p[:, fan].mean(axis=1)
    assert (cen[0] * cen[1] > 0).all() and (cen[0] > 0).any() and (cen[0] < 0).any()


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_features_are_the_expected_ones(built_library, key):
    """A change of the dissection that moves a cut fails here, with the coverage it costs."""
    got = tc.features(analysis(*key))
    assert got == tc.EXPECT[key], {k: (got[k], tc.EXPECT[key][k]) for k in got if got[k] != tc.EXPECT[key][k]}


def test_every_operator_case_has_its_facts(built_library):
    for case in oc.TOPOLOGY_CASES:
        assert (case.mesh[1], case.dpn, case.leaf) in tc.EXPECT, case.name
    want = {("islands", 24), ("islands", 4), ("bowtie", 24), ("comb", 4), ("annulus", 4), ("strip1", 4), ("graded", 24),
            ("tiny2", 0)}
    assert {(c.mesh[1], c.leaf) for c in oc.TOPOLOGY_CASES} == want
    assert all(c.factor for c in oc.TOPOLOGY_CASES)
    # what the matrix did not have before: an empty root under two fronts without boundary, a root of one real node;
    # and trees in which fronts without owned DOFs are a large share
    facts = [tc.EXPECT[(c.mesh[1], c.dpn, c.leaf)] for c in oc.TOPOLOGY_CASES]
    assert any(f["root_fs"] == 0 and f["m0_fronts"] and f["s2_0_levels"] == [0] and f["free_fronts"] == 2 for f in facts)
    assert any(f["empty_inner"] >= 20 for f in facts) and any(f["empty_leaves"] >= 24 for f in facts)
    assert any(f["root_fs"] - f["root_padding"] == 1 for f in facts)


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_front_tree_invariants_hold(built_library, key):
    check_tree_invariants(analysis(*key))


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_emulation_matches_splu(built_library, c1_geometry, key):
    """front_emulation.factor / solve on the case's tree against SuperLU, over the four right-hand sides of the GPU tests:
    forward error below FWD_TOL (measured: at most 3.6e-12, islands vectorial at leaf 4), Dirichlet entries exactly 0, no
    pivot replaced."""
    name, dpn, _leaf = key
    sym = analysis(*key)
    mesh = tc.trimesh(name)
    K, idx, _sigma, _A, _B, Ke = oc.host_pencil(sym, mesh, geometry_of(name, c1_geometry), dpn)
    T = fe.FrontTree(sym)
    logs = {}
    Fs, Ds = fe.factor(T, Ke, logs=logs)
    assert not logs
    lu = spla.splu(K.tocsc())
    worst_f = worst_b = 0.0
    for what, b in right_hand_sides(T, idx, sym.N).items():
        x = fe.solve(T, Fs, Ds, b)
        xs = lu.solve(b[idx])
        rest = np.delete(x, idx)
        assert rest.size == 0 or np.abs(rest).max() == 0.0, what
        worst_f = max(worst_f, np.linalg.norm(x[idx] - xs) / np.linalg.norm(xs))
        worst_b = max(worst_b, backward_error(K, x[idx], b[idx]))
    print(f"\n{IDS[KEYS.index(key)]}: forward error {worst_f:.2e}, backward error {worst_b:.2e}")
    assert worst_f < FWD_TOL


def test_root_right_hand_side_sits_on_the_shallowest_owner(built_library, c1_geometry):
    """The "root" right-hand side is supported on the shallowest front that owns DOFs.  For every case the matrix had
    before the topology cases that front is the root and the four right-hand sides keep their bits (the rule they were
    drawn by is restated here); with an empty root it is front 1."""
    meshes = {}
    for case in oc.CASES:
        if case in oc.TOPOLOGY_CASES:
            continue
        if case.mesh not in meshes:
            meshes[case.mesh] = oc.mesh_of(case, c1_geometry)
        sym = oc.symbolic_of(case, meshes[case.mesh])
        T, N = fe.FrontTree(sym), sym.N
        interior = sym.array("interior").astype(np.int64)
        idx = np.concatenate([interior, interior + N]) if case.dpn == 2 else np.arange(N)
        assert shallowest_owner(T, N) == 0, case.name
        facts = tc.features(sym)           # ... and none of them has what the topology cases are in the matrix for
        assert facts["m0_fronts"] == 0 and facts["free_fronts"] == 0 and facts["s2_0_levels"] == [], case.name
        assert facts["root_fs"] - facts["root_padding"] > 1, case.name
        got = right_hand_sides(T, idx, N)
        rng = np.random.default_rng(7)
        want = {}
        for nm in ("random", "random2"):
            want[nm] = np.zeros(case.dpn * N)
            want[nm][idx] = rng.standard_normal(len(idx))
        for nm, f in (("leaf", max(range(T.leaf0, T.nf), key=lambda f: int(T.fs[f]))), ("root", 0)):
            d = owned_dofs(T, f, N)
            want[nm] = np.zeros(case.dpn * N)
            want[nm][d] = rng.standard_normal(len(d))
        assert list(got) == list(want)
        for nm in want:
            assert np.array_equal(got[nm], want[nm]), (case.name, nm)
        sym.close()
    for case in oc.TOPOLOGY_CASES:
        sym = analysis(case.mesh[1], case.dpn, case.leaf)
        T = fe.FrontTree(sym)
        f = shallowest_owner(T, sym.N)
        assert f == (1 if tc.EXPECT[(case.mesh[1], case.dpn, case.leaf)]["root_fs"] == 0 else 0), case.name
        interior = sym.array("interior").astype(np.int64)
        idx = np.concatenate([interior, interior + sym.N]) if case.dpn == 2 else np.arange(sym.N)
        rhs = right_hand_sides(T, idx, sym.N)
        assert set(np.nonzero(rhs["root"])[0]) <= set(owned_dofs(T, f, sym.N).tolist()) and rhs["root"].any()


class _Recorder:
    """Stands in for a device context: records what FrontTree.device_front asks debug_copy for."""

    def __init__(self, sizes):
        self.sizes, self.calls = sizes, []

    def debug_copy(self, name, offset, count):
        assert count > 0 and 0 <= offset and offset + count <= self.sizes[name], (name, offset, count, self.sizes[name])
        self.calls.append(name)
        return np.zeros(count)


@pytest.mark.parametrize("key", [k for k in KEYS if (k[0], k[2]) in (("islands", 24), ("bowtie", 4), ("comb", 4), ("tiny2", 0))],
                         ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}")
def test_device_front_reads_stay_inside_the_buffers(built_library, key):
    """FrontTree.device_front and the D^-1 read-back of the GPU tests on fronts with m = 0, s2 = 0 or b2 = 0: empty blocks
    come back empty, nothing is requested for them, and no request reaches past the storage of the fronts / an arena."""
    sym = analysis(*key)
    T = fe.FrontTree(sym)
    arena = (int(sym.info["arena_doubles"]) + 31) & ~31
    rec = _Recorder({"front": int(sym.info["front_doubles"]), "schur": 2 * arena, "delta": 2 * 2 * int(T.fptr[T.nf])})
    kinds = set()
    for f in range(T.nf):
        m, s2 = T.m(f), T.s2(f)
        b2 = m - s2
        kinds.add((m == 0, s2 == 0, b2 == 0))
        rec.calls.clear()
        F = T.device_front(rec, f, with_schur=True)
        assert F.shape == (m, m)
        assert F[:s2, :s2].size == s2 * s2 and F[s2:, :s2].size == b2 * s2 and F[s2:, s2:].size == b2 * b2
        assert rec.calls.count("front") == (0 if s2 == 0 else 1 if b2 == 0 else 2)
        assert rec.calls.count("schur") == (1 if b2 else 0)
        assert not np.isnan(F[:, :s2]).any() and not np.isnan(F[s2:, s2:]).any()
        if s2:           # the read-back of D^-1 as test_every_front_matches_the_emulation does it
            rec.debug_copy("delta", 2 * 2 * T.fptr[f], 2 * s2)
    facts = tc.EXPECT[key]
    if facts["m0_fronts"]:
        assert (True, True, True) in kinds
    if facts["free_fronts"]:
        assert (False, False, True) in kinds
    if facts["empty_inner"] > 1 or facts["empty_leaves"]:
        assert (False, True, False) in kinds


@pytest.mark.parametrize("name", tc.NAMES)
def test_pattern_is_the_union_pattern(built_library, name):
    sym = analysis(name, 1, 24)
    ed = sym.array("edof").reshape(6, -1)
    rows = np.broadcast_to(ed.T[:, :, None], (ed.shape[1], 6, 6)).ravel()
    cols = np.broadcast_to(ed.T[:, None, :], (ed.shape[1], 6, 6)).ravel()
    P = sp.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(sym.N, sym.N)).tocsr()
    P.sort_indices()
    np.testing.assert_array_equal(sym.array("rowptr"), P.indptr)
    np.testing.assert_array_equal(sym.array("colind"), P.indices)
    np.testing.assert_array_equal(sym.array("slot_row"), np.repeat(np.arange(sym.N), np.diff(P.indptr)))
    assert sym.info["nnz"] == P.nnz


@pytest.mark.parametrize("name", tc.NAMES)
def test_neighbour_table_is_the_emulations(built_library, name):
    """elem_nbr (what k_mode_indicators reads) against IndicatorEmulation.nbr, as sets per element; a rim edge has -1."""
    p, t = tc.mesh(name)
    sym = analysis(name, 1, 24)
    nbr = sym.array("elem_nbr").reshape(3, -1)
    em = IndicatorEmulation(p, t)
    assert nbr.shape == em.nbr.shape
    assert np.array_equal(np.sort(nbr, axis=0), np.sort(em.nbr, axis=0))
    assert np.array_equal(nbr, em.nbr)                                  # ... and edge by edge, in the local edge order
    assert (nbr < 0).sum() == tc.rim_edges(t).shape[1]
    if name == "bowtie":                                                # no neighbour across the pinch
        left = p[0, t].mean(axis=0) < 0
        ok = nbr >= 0
        assert (left[np.where(ok, nbr, 0)] == left[None])[ok].all()


@pytest.mark.parametrize("name", tc.FIELD_MESHES)
def test_probe_points_leave_little_to_the_near_rule(built_library, name):
    """The sampling points of test_gpu_topology.py under the emulation alone: at most 5 % are within LOOSE of more than
    one element (compared by value only on the GPU), the void points are inside no element and near none, every rim point
    is on exactly one element."""
    p, t = tc.mesh(name)
    em = IndicatorEmulation(p, t)
    pts = tc.probe_points(name)
    allp = np.hstack(list(pts.values()))
    elem, _xi, _eta, near = em.locate(allp)
    share = float((near > 1).mean())
    print(f"\n{name}: {allp.shape[1]} points, {share:.1%} near more than one element")
    assert share <= 0.05
    e, _, _, n = em.locate(pts["void"])
    assert (e == -1).all() and (n == 0).all() and pts["void"].shape[1] >= 50
    e, _, _, n = em.locate(pts["rim"])
    assert (e >= 0).all() and (n == 1).all()
    e, _, _, n = em.locate(pts["random"])
    assert (e < 0).sum() >= 40 and (e >= 0).sum() >= 150
    if name == "bowtie":
        e, _, _, n = em.locate(pts["pinch"])
        v0 = int(np.nonzero((p[0] == 0.0) & (p[1] == 0.0))[0][0])
        fan = np.nonzero((t == v0).any(axis=0))[0]
        assert e[0] == fan.min() and n[0] == fan.size           # the tie rule at the pinch vertex: the smallest id of its fan
        assert (e >= 0).all()
