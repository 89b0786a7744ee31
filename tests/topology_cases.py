"""Meshes that are no disc, no square and no row of squares: a hole, two parts, a notch, teeth, strips one and two
elements wide, two squares that meet in one vertex, sizes graded by marked bisection, two triangles, and two-part
sections with and without a forced degeneracy.  Shared by the host tests (test_topology_cases_host.py), the operator
matrix (operator_cases.py) and the GPU tests (test_gpu_topology.py).  NumPy and the package's own mesh helpers only."""
from __future__ import annotations

import functools

import numpy as np

HALF = 12.0                 # the base mesh is unit_square_mesh(16) mapped to [-HALF, HALF]^2: the C1 core discs cut it
NAMES = ("annulus", "islands", "notch", "comb", "strip1", "strip2", "bowtie", "graded", "tiny2", "twins", "pair")
GRADED_CENTRE = (1.4, 0.3)
GRADED_ROUNDS = 10
GRADED_RADIUS = 0.6         # a round marks the elements whose centroid is within this of GRADED_CENTRE


def compact(p, t):
    """Unused vertices dropped, ids compacted (order kept)."""
    used = np.unique(t)
    remap = -np.ones(p.shape[1], dtype=np.int32)
    remap[used] = np.arange(len(used), dtype=np.int32)
    return np.ascontiguousarray(p[:, used], dtype=np.float64), np.ascontiguousarray(remap[t], dtype=np.int32)


def _square(n, half):
    """unit_square_mesh(n) mapped to [-half, half]^2."""
    from pl_fem_vectoriel_amd.mesh import unit_square_mesh
    m = unit_square_mesh(n)
    return (m.p - 0.5) * (2.0 * half), m.t


def _cut(keep):
    """The base mesh without the elements whose centroid (x, y) fails keep."""
    p, t = _square(16, HALF)
    c = p[:, t].mean(axis=1)
    return compact(p, t[:, keep(c[0], c[1])])


def _strip(w):
    """40 x w cells of two triangles, x from -12 to 12, height 0.6 w about y = 0."""
    gx, gy = np.linspace(-HALF, HALF, 41), np.linspace(-0.3 * w, 0.3 * w, w + 1)
    X, Y = np.meshgrid(gx, gy)
    idx = np.arange(41 * (w + 1)).reshape(w + 1, 41)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    return np.vstack([X.ravel(), Y.ravel()]), np.hstack([np.vstack([a, b, d]), np.vstack([a, d, c])]).astype(np.int32)


def _join(parts):
    """Disjoint union of (p, t) parts."""
    ps, ts, off = [], [], 0
    for p, t in parts:
        ps.append(p)
        ts.append(t + off)
        off += p.shape[1]
    return np.hstack(ps), np.hstack(ts).astype(np.int32)


def _bowtie():
    """Two 6-squares of side 10, on [-10, 0]^2 and [0, 10]^2; the two vertices at the origin are one."""
    pa, ta = _square(6, 5.0)
    p, t = _join([(pa - 5.0, ta), (pa + 5.0, ta)])
    at0 = np.nonzero((p[0] == 0.0) & (p[1] == 0.0))[0]
    assert at0.size == 2
    t = np.where(t == at0[1], at0[0], t)
    return compact(p, t)


def _two_squares(n_left, n_right):
    """Squares of side 10 centred at (-8, 0) and (8, 0)."""
    pl, tl = _square(n_left, 5.0)
    pr, tr = _square(n_right, 5.0)
    return _join([(pl + np.array([[-8.0], [0.0]]), tl), (pr + np.array([[8.0], [0.0]]), tr)])


def _graded():
    """Marked bisection of the elements around one point, GRADED_ROUNDS times: a fixed small neighbourhood, so that the
    sizes at the point halve every round while the far elements stay (area_spread: the ratio reached)."""
    from pl_fem_vectoriel_amd.mesh import TriMesh
    p, t = _square(6, HALF)
    m = TriMesh(p, t)
    for _ in range(GRADED_ROUNDS):
        c = m.p[:, m.t].mean(axis=1)
        marked = np.hypot(c[0] - GRADED_CENTRE[0], c[1] - GRADED_CENTRE[1]) <= GRADED_RADIUS
        if not marked.any():
            marked[np.argmin(np.hypot(c[0] - GRADED_CENTRE[0], c[1] - GRADED_CENTRE[1]))] = True
        m, _parent = m.refined_marked(marked)
    return m.p, m.t


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "annulus":
        p, t = _cut(lambda x, y: np.hypot(x, y) > 5.0)
    elif name == "islands":
        p, t = _cut(lambda x, y: np.abs(x) > 3.0)
    elif name == "notch":
        p, t = _cut(lambda x, y: (x < 0.0) | (y < 0.0))
    elif name == "comb":
        p, t = _cut(lambda x, y: (y < -6.0) | (np.floor((x + HALF) / 3.0) % 2 == 0))
    elif name in ("strip1", "strip2"):
        p, t = _strip(int(name[-1]))
    elif name == "bowtie":
        p, t = _bowtie()
    elif name == "graded":
        p, t = _graded()
    elif name == "tiny2":
        p = np.array([[-1.5, 1.5, -1.5, 1.5], [-1.5, -1.5, 1.5, 1.5]])
        t = np.array([[0, 0], [1, 3], [3, 2]], dtype=np.int32)
    elif name == "twins":
        p, t = _two_squares(10, 10)
    elif name == "pair":
        p, t = _two_squares(10, 8)
    elif name == "full":                    # (the uncut base mesh: the partner of the holed meshes in the overlap tests)
        p, t = _square(16, HALF)
    else:
        raise KeyError(name)
    p, t = compact(np.asarray(p, dtype=np.float64), np.sort(np.asarray(t), axis=0))
    p.setflags(write=False)
    t.setflags(write=False)
    return p, t


def mesh(name):
    """(p, t) of the named mesh: p (2, nv) float64, t (3, ne) int32, every vertex used.  Deterministic."""
    p, t = _mesh(name)
    return p.copy(), t.copy()


def trimesh(name):
    from pl_fem_vectoriel_amd.mesh import TriMesh
    return TriMesh(*mesh(name))


def area_spread(p, t):
    """Largest element area over the smallest."""
    a, b, c = p[:, t[0]], p[:, t[1]], p[:, t[2]]
    area = 0.5 * np.abs((b[0] - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (b[1] - a[1]))
    return float(area.max() / area.min())


def two_core_geometry():
    """The geometry of ``twins`` / ``pair``: one core of radius 1.5 in the middle of each part (built as discs() of
    test_gpu_field_shapes.py: no PML, only the real permittivity is read)."""
    from pl_fem_vectoriel_amd import MCFGeometry
    g = MCFGeometry(7, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55, use_complex_pml=False)
    g.positions = g.core_positions = np.array([[-8.0, 0.0], [8.0, 0.0]])
    g.core_radii = np.array([1.5, 1.5])
    g.n_cores = 2
    return g


def rim_edges(t):
    """(2, n) vertex pairs of the edges that belong to one element only: the outer boundary and the rims of holes."""
    pairs = np.sort(np.hstack([t[[0, 1]], t[[1, 2]], t[[0, 2]]]), axis=0)
    uniq, count = np.unique(pairs, axis=1, return_counts=True)
    return uniq[:, count == 1]


FIELD_MESHES = ("annulus", "islands", "bowtie")
VOID = {"annulus": lambda x, y: np.hypot(x, y) < 3.0,                     # well inside the hole (its rim is a staircase)
        "islands": lambda x, y: np.abs(x) < 2.9,                            # the gap between the two parts
        "bowtie": lambda x, y: ((x < -0.1) & (y > 0.1)) | ((x > 0.1) & (y < -0.1))}   # the two quadrants without material


def probe_points(name, seed=0):
    """Sampling points of a FIELD_MESHES mesh by kind: "random" over the bounding box and a tenth beyond it, "void"
    (in the hole / gap and outside the box: inside no element), "rim" (the midpoints of all rim edges and points a
    third along them: on one element's edge, no neighbour across), "pinch" (bowtie: the shared vertex, and points on the
    four rim edges that leave it)."""
    p, t = _mesh(name)
    rng = np.random.default_rng([seed, FIELD_MESHES.index(name)])
    x0, x1, y0, y1 = p[0].min(), p[0].max(), p[1].min(), p[1].max()
    dx, dy = 0.1 * (x1 - x0), 0.1 * (y1 - y0)
    rnd = np.vstack([rng.uniform(x0 - dx, x1 + dx, 400), rng.uniform(y0 - dy, y1 + dy, 400)])
    cand = np.vstack([rng.uniform(x0, x1, 2000), rng.uniform(y0, y1, 2000)])
    void = cand[:, VOID[name](cand[0], cand[1])][:, :100]
    outside = np.array([[x0 - dx, x1 + dx, 0.5 * (x0 + x1), 0.3 * x0, x0 - 1e-3, x1 + 1e-3],
                        [0.2 * y0, 0.7 * y1, y1 + dy, y0 - dy, y0 - 1e-3, y1 + 1e-3]])
    e = rim_edges(t)
    a, b = p[:, e[0]], p[:, e[1]]
    out = {"random": rnd, "void": np.hstack([void, outside]), "rim": np.hstack([0.5 * (a + b), a + (b - a) / 3.0])}
    if name == "bowtie":
        v0 = int(np.nonzero((p[0] == 0.0) & (p[1] == 0.0))[0][0])
        spokes = e[:, (e == v0).any(axis=0)]
        other = np.where(spokes[0] == v0, spokes[1], spokes[0])
        assert other.size == 4
        out["pinch"] = np.hstack([p[:, [v0]], 0.25 * p[:, other], 1e-9 * p[:, other]])
    return out


def features(sym):
    """The structural facts of an analysis that the cases are chosen for, from fs, fb and the level count."""
    fs, fb = sym.array("fs").astype(np.int64), sym.array("fb").astype(np.int64)
    L, nf = int(sym.info["levels"]), int(sym.info["nfronts"])
    leaf0 = (1 << L) - 1
    assert nf == (1 << (L + 1)) - 1 == fs.size == fb.size
    fn, fptr = sym.array("fnodes"), sym.array("fnode_ptr")
    root = fn[fptr[0]:fptr[0] + fs[0]]
    inner, leaves = np.arange(nf) < leaf0, np.arange(nf) >= leaf0
    return {"levels": L,
            "root_fs": int(fs[0]),
            "root_padding": int((root < 0).sum()),
            "m0_fronts": int(((fs + fb) == 0).sum()),
            "empty_inner": int(((fs == 0) & inner).sum()),
            "empty_leaves": int(((fs == 0) & leaves).sum()),
            "free_fronts": int(((fs > 0) & (fb == 0))[1:].sum()),           # not the root: owned DOFs, no boundary
            "s2_0_levels": [lev for lev in range(L + 1) if fs[(1 << lev) - 1:(1 << (lev + 1)) - 1].max() == 0]}


def _facts(levels, root_fs, root_padding, m0_fronts, empty_inner, empty_leaves, free_fronts, s2_0_levels=()):
    return {"levels": levels, "root_fs": root_fs, "root_padding": root_padding, "m0_fronts": m0_fronts,
            "empty_inner": empty_inner, "empty_leaves": empty_leaves, "free_fronts": free_fronts,
            "s2_0_levels": list(s2_0_levels)}


# (mesh, unknowns per node, leaf_elems) -> features of its analysis: what each case is in the tests for.  A change of the
# dissection that moves a cut shows here as the coverage it costs (test_topology_cases_host.py).
EXPECT = {
    # two parts: the root cut runs through the gap and owns nothing (m = 0, level 0 with max_s2 = 0); the two fronts below
    # it own DOFs and have no boundary (b2 = 0: no Z, no Schur complement)
    ("islands", 2, 24): _facts(4, 0, 0, 1, 1, 0, 2, (0,)),
    ("islands", 1, 24): _facts(4, 0, 0, 1, 1, 0, 2, (0,)),
    ("islands", 2, 4): _facts(7, 0, 0, 1, 1, 0, 2, (0,)),
    ("islands", 1, 4): _facts(7, 0, 0, 1, 1, 0, 2, (0,)),
    ("twins", 2, 24): _facts(5, 0, 0, 1, 1, 0, 2, (0,)),
    ("twins", 1, 24): _facts(5, 0, 0, 1, 1, 0, 2, (0,)),
    ("pair", 2, 24): _facts(4, 0, 0, 1, 1, 0, 2, (0,)),
    ("pair", 1, 24): _facts(4, 0, 0, 1, 1, 0, 2, (0,)),
    # the same through a pinch (the shared vertex is Dirichlet); scalar: the root owns the pinch vertex and 15 padding nodes
    ("bowtie", 2, 24): _facts(3, 0, 0, 1, 1, 0, 2, (0,)),
    ("bowtie", 2, 4): _facts(6, 0, 0, 1, 1, 24, 2, (0,)),
    ("bowtie", 1, 24): _facts(3, 16, 15, 0, 0, 0, 0),
    ("bowtie", 1, 4): _facts(6, 16, 15, 0, 0, 16, 0),
    # teeth: 20 inner fronts own nothing and only hand their boundary on to their children
    ("comb", 2, 4): _facts(7, 8, 1, 0, 20, 24, 0),
    ("comb", 1, 4): _facts(7, 16, 7, 0, 20, 7, 0),
    # a hole: separators cut by it
    ("annulus", 2, 4): _facts(7, 24, 6, 0, 3, 6, 0),
    ("annulus", 2, 24): _facts(5, 24, 6, 0, 0, 0, 0),
    ("annulus", 1, 24): _facts(5, 32, 10, 0, 0, 0, 0),
    ("notch", 2, 4): _facts(7, 16, 1, 0, 0, 0, 0),
    ("notch", 1, 4): _facts(7, 32, 15, 0, 0, 0, 0),
    # strips: separators of one real node (vectorial, one element wide: every vertex is Dirichlet)
    ("strip1", 2, 4): _facts(5, 8, 7, 0, 0, 0, 0),
    ("strip2", 2, 4): _facts(6, 8, 5, 0, 8, 8, 0),
    ("graded", 2, 24): _facts(5, 56, 7, 0, 0, 0, 0),
    ("graded", 2, 4): _facts(7, 56, 7, 0, 4, 35, 0),
    # two triangles: one front; vectorial 2 unknowns (the midpoint of the diagonal) in 16 rows
    ("tiny2", 2, 0): _facts(0, 8, 7, 0, 0, 0, 0),
    ("tiny2", 1, 0): _facts(0, 16, 7, 0, 0, 0, 0),
}
