"""Marked refinement (plfem_mesh_refine_marked, host code): six rounds of seeded random marks on the jittered square and
on C1 at level 0.  Every round must leave a conforming mesh of the same area in which no marked element survives, with
children that tile their parents, untouched old vertices and exact midpoints -- the same bytes on a second run, and a
smallest angle no less than half the input mesh's (the bound of longest-edge bisection)."""
import ctypes

import numpy as np
import pytest

from core_ties import jittered_square_mesh
from pl_fem_vectoriel_amd import TriMesh, _native, generate_mesh, refine_marked

ROUNDS = 6


def areas(mesh):
    p, t = mesh.p, mesh.t
    a, b = p[:, t[1]] - p[:, t[0]], p[:, t[2]] - p[:, t[0]]
    return 0.5 * np.abs(a[0] * b[1] - a[1] * b[0])


def min_angle(mesh):
    p, t = mesh.p, mesh.t
    out = []
    for i in range(3):
        u, w = p[:, t[(i + 1) % 3]] - p[:, t[i]], p[:, t[(i + 2) % 3]] - p[:, t[i]]
        out.append(np.arctan2(np.abs(u[0] * w[1] - u[1] * w[0]), u[0] * w[0] + u[1] * w[1]))
    return float(np.min(out))


def edge_counts(mesh):
    """(counts, lengths) of the unique edges: elements per edge and its length."""
    t = mesh.t.astype(np.int64)
    nv = mesh.p.shape[1]
    pairs = np.hstack([t[[0, 1]], t[[1, 2]], t[[0, 2]]])
    key, counts = np.unique(pairs[0] * nv + pairs[1], return_counts=True)
    d = mesh.p[:, key % nv] - mesh.p[:, key // nv]
    return counts, np.hypot(d[0], d[1])


def one_sided_length(mesh):
    """Total length of the edges with one element: the perimeter of a conforming mesh.  A vertex inside an edge leaves the
    whole edge on one side and its two halves on the other, all three with one element: twice the edge more."""
    counts, length = edge_counts(mesh)
    return float(length[counts == 1].sum())


@pytest.fixture(scope="module", params=["square", "c1"])
def start(request, built_library, c1_geometry):
    if request.param == "square":
        return jittered_square_mesh(8)
    mesh = generate_mesh(c1_geometry, 1.0, 0)
    assert mesh.t.shape[1] == 11313
    return mesh


def test_six_rounds_of_random_marks(start):
    rng = np.random.default_rng(11)
    mesh = start
    area0, angle0 = areas(mesh).sum(), min_angle(mesh)
    perimeter = one_sided_length(mesh)
    for rnd in range(ROUNDS):
        marked = rng.random(mesh.t.shape[1]) < 0.15
        finer, parent = refine_marked(mesh, marked)
        again, parent2 = refine_marked(mesh, marked)
        assert finer.p.tobytes() == again.p.tobytes() and finer.t.tobytes() == again.t.tobytes()
        assert parent.tobytes() == parent2.tobytes()
        nv, ne = mesh.p.shape[1], mesh.t.shape[1]
        # conforming: the analysis accepts it (every edge has at most two elements), no vertex lies inside an edge (the
        # one-element edges are still the perimeter) and the area closes
        sym = _native.Symbolic(finer.p, finer.t)
        counts, _ = edge_counts(finer)
        assert counts.max() == 2 and sym.nedges == counts.size
        assert abs(one_sided_length(finer) - perimeter) <= 1e-12 * perimeter
        a = areas(finer)
        assert abs(a.sum() - area0) <= 1e-13 * area0
        # old vertices untouched, new ones exact midpoints of old edges
        assert np.array_equal(finer.p[:, :nv], mesh.p)
        edges, _ = mesh.edges()
        mids = 0.5 * (mesh.p[:, edges[0]] + mesh.p[:, edges[1]])
        new = finer.p[:, nv:]
        key = {(x, y) for x, y in mids.T}
        assert all((x, y) in key for x, y in new.T)
        # no marked element survives, the children tile their parent
        assert parent.shape == (finer.t.shape[1],) and np.all(np.diff(parent) >= 0) and parent.min() == 0 and parent.max() == ne - 1
        kids = np.bincount(parent, minlength=ne)
        assert np.all(kids[marked] >= 2) and np.all((kids >= 1) & (kids <= 4))
        pa = areas(mesh)
        assert np.abs(np.bincount(parent, weights=a, minlength=ne) - pa).max() <= 1e-13 * pa.max()
        whole = kids == 1
        assert np.array_equal(finer.t[:, np.isin(parent, np.nonzero(whole)[0])], mesh.t[:, whole])
        assert np.all(np.sort(finer.t, axis=0) == finer.t)
        ang = min_angle(finer)
        print(f"round {rnd}: {ne} -> {finer.t.shape[1]} elements, smallest angle {np.degrees(ang):.3f} deg "
              f"(input {np.degrees(angle0):.3f})")
        assert ang >= 0.5 * angle0
        mesh = finer


def test_no_marks_and_all_marks(start):
    mesh = start
    ne = mesh.t.shape[1]
    same, parent = mesh.refined_marked(np.zeros(ne, dtype=bool))
    assert np.array_equal(same.p, mesh.p) and np.array_equal(same.t, mesh.t) and np.array_equal(parent, np.arange(ne))
    every, parent = mesh.refined_marked(np.ones(ne, dtype=np.uint8))
    assert np.all(np.bincount(parent, minlength=ne) >= 2)
    assert abs(areas(every).sum() - areas(mesh).sum()) <= 1e-13 * areas(mesh).sum()
    _native.Symbolic(every.p, every.t)


def test_new_vertex_ids_rank_the_marked_edges(built_library):
    mesh = jittered_square_mesh(8)
    marked = np.zeros(mesh.t.shape[1], dtype=bool)
    marked[[5, 40, 77]] = True
    finer, _ = mesh.refined_marked(marked)
    nv = mesh.p.shape[1]
    edges, _ = mesh.edges()
    mids = 0.5 * (mesh.p[:, edges[0]] + mesh.p[:, edges[1]])
    lookup = {(x, y): i for i, (x, y) in enumerate(mids.T)}
    ids = [lookup[(x, y)] for x, y in finer.p[:, nv:].T]
    assert ids == sorted(ids) and len(set(ids)) == len(ids)          # nv + rank among the marked edges, in edge-id order


def test_bad_arguments_report_through_err(built_library):
    lib = built_library
    mesh = jittered_square_mesh(2)
    p, t = mesh.p, mesh.t
    nv, ne = p.shape[1], t.shape[1]
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    marked = np.ones(ne, dtype=np.uint8)
    err = ctypes.create_string_buffer(256)
    nvo, neo = ctypes.c_int32(0), ctypes.c_int32(0)
    ok = lib.plfem_mesh_refine_marked_count(nv, ne, ptr(p), ptr(t), ptr(marked), ctypes.byref(nvo), ctypes.byref(neo), err, 256)
    assert ok == _native.PLFEM_OK and neo.value > ne and nvo.value > nv
    p2, t2 = np.empty((2, nvo.value)), np.empty((3, neo.value), dtype=np.int32)
    parent = np.empty(neo.value, dtype=np.int32)
    for args in ((None, ptr(t), ptr(marked)), (ptr(p), None, ptr(marked)), (ptr(p), ptr(t), None)):
        err.value = b""
        assert lib.plfem_mesh_refine_marked_count(nv, ne, *args, ctypes.byref(nvo), ctypes.byref(neo), err, 256) == _native.PLFEM_EINVAL
        assert b"null pointer" in err.value
        err.value = b""
        assert lib.plfem_mesh_refine_marked(nv, ne, *args, ptr(p2), ptr(t2), ptr(parent), err, 256) == _native.PLFEM_EINVAL
        assert b"null pointer" in err.value
    err.value = b""
    assert lib.plfem_mesh_refine_marked(nv, ne, ptr(p), ptr(t), ptr(marked), ptr(p2), ptr(t2), None, err, 256) == _native.PLFEM_EINVAL
    assert b"null pointer" in err.value
    bad = t.copy()
    bad[2, 0] = nv + 3                                           # a vertex outside p
    err.value = b""
    assert lib.plfem_mesh_refine_marked(nv, ne, ptr(p), ptr(bad), ptr(marked), ptr(p2), ptr(t2), ptr(parent), err, 256) == _native.PLFEM_EMESH
    assert b"outside" in err.value
    err.value = b""
    assert lib.plfem_mesh_refine_marked_count(2, ne, ptr(p), ptr(t), ptr(marked), ctypes.byref(nvo), ctypes.byref(neo), err, 256) == _native.PLFEM_EMESH
    assert err.value
    with pytest.raises(ValueError):
        mesh.refined_marked(np.ones(ne + 1, dtype=bool))
    with pytest.raises(ValueError):
        mesh.refined_marked(np.ones(ne))                         # floats are no flags
    assert isinstance(mesh.refined_marked(marked)[0], TriMesh)
