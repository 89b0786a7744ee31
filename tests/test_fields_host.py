"""Mode fields, host side (no GPU): the locator grid of the analysis, the NumPy emulation of the sampling kernel
against a direct per-element evaluation, argument checking before any device call, and the solve's workspace
untouched by a locator."""
import ctypes

import numpy as np
import pytest

from fields_emulation import Emulation
from oracle.p2 import p2_basis
from pl_fem_vectoriel_amd import ModeFields, _native, generate_mesh, mode_overlap
from pl_fem_vectoriel_amd.mesh import unit_square_mesh


@pytest.fixture(scope="module")
def small_mesh(c1_geometry, built_library):
    return generate_mesh(c1_geometry, 0.5, 0)


def test_locator_cells_list_exactly_the_bounding_box_cells(small_mesh):
    sym = _native.Symbolic(small_mesh.p, small_mesh.t)
    g = sym.array("loc_grid")
    ptr, elems = sym.array("loc_cell_ptr"), sym.array("loc_cell_elems")
    x0, y0, ihx, ihy, nx, ny = g[0], g[1], g[2], g[3], int(g[4]), int(g[5])
    ne = sym.ne
    assert nx * ny <= 2 * ne and ptr.size == nx * ny + 1 and ptr[-1] == elems.size
    p, t = small_mesh.p, small_mesh.t
    assert x0 == p[0].min() and y0 == p[1].min()

    def cell(v, v0, ih, n):
        return np.clip(np.floor((v - v0) * ih), 0, n - 1).astype(np.int64)

    X, Y = p[0][t], p[1][t]                                   # (3, ne)
    ix0, ix1 = cell(X.min(0), x0, ihx, nx), cell(X.max(0), x0, ihx, nx)
    iy0, iy1 = cell(Y.min(0), y0, ihy, ny), cell(Y.max(0), y0, ihy, ny)
    expect = [[] for _ in range(nx * ny)]
    for e in range(ne):
        for iy in range(iy0[e], iy1[e] + 1):
            for ix in range(ix0[e], ix1[e] + 1):
                expect[iy * nx + ix].append(e)
    for c in range(nx * ny):
        got = elems[ptr[c]:ptr[c + 1]]
        assert got.tolist() == expect[c], c                   # every bbox cell, no other, ascending
    st = sym.array("loc_stats")
    assert st[0] == nx * ny and st[1] == pytest.approx(elems.size / (nx * ny)) and st[2] == np.diff(ptr).max()


def test_emulation_matches_direct_per_element_evaluation(small_mesh):
    em = Emulation(small_mesh.p, small_mesh.t)
    rng = np.random.default_rng(3)
    ne = small_mesh.t.shape[1]
    e = rng.integers(0, ne, 400)
    a = rng.uniform(0.05, 0.9, e.size)
    b = rng.uniform(0.0, 1.0, e.size) * (0.95 - a)
    J = em.basis.J[:, :, e]
    p0 = small_mesh.p[:, small_mesh.t[0, e]]
    pts = p0 + J[:, 0] * a + J[:, 1] * b
    k = 3
    vals = rng.standard_normal((2, k, em.interior.size))
    beta = np.array([5.0, 6.0, 7.0])
    out, elem = em.sample(vals, pts, indexed=True, beta=beta)
    assert (elem == e).all()
    phi, dphi = p2_basis(a, b)
    dofs = em.basis.element_dofs[:, e]
    full = np.zeros((2, k, em.N))
    full[:, :, em.interior] = vals
    direct = np.einsum("an,ckan->ckn", phi, full[:, :, dofs])
    # (the points went through x = p0 + J xi and back: on sliver elements that costs digits)
    assert np.abs(out[:2] - direct).max() <= 1e-10 * np.abs(direct).max()
    inv = em.basis.invJ[:, :, e]
    grad = [np.einsum("an,kan->kn", dphi[:, 0] * inv[0, c] + dphi[:, 1] * inv[1, c], full[c][:, dofs]) for c in (0, 1)]
    hz = -(grad[0] + grad[1]) / beta[:, None]
    assert np.abs(out[2] - hz).max() <= 1e-10 * np.abs(hz).max()
    # scalar layout on all N DOFs, and a point far outside
    u = rng.standard_normal((1, k, em.N))
    pts2 = np.hstack([pts, [[1e3], [1e3]]])
    out, elem = em.sample(u, pts2, indexed=False)
    assert elem[-1] == -1 and (out[:, :, -1] == 0).all()
    direct = np.einsum("an,kan->kn", phi, u[0][:, dofs])
    assert np.abs(out[0][:, :-1] - direct).max() <= 1e-10 * np.abs(direct).max()


def test_argument_errors_raise_before_any_device_call(small_mesh):
    mf = ModeFields(small_mesh)
    vec = {"Ex_dofs": np.zeros(mf.nsolve), "Ey_dofs": np.zeros(mf.nsolve), "beta": 6.0}
    sca = {"field_vector": np.zeros(mf.N)}
    pts = np.zeros((2, 4))
    with pytest.raises(ValueError):
        mf.sample([vec, sca], pts)                            # mixed kinds
    with pytest.raises(ValueError):
        mf.sample([{"Ex_dofs": np.zeros(mf.N), "Ey_dofs": np.zeros(mf.N)}], pts)   # vectorial vector of length N
    with pytest.raises(ValueError):
        mf.sample([{"field_vector": np.zeros(mf.nsolve)}], pts)                   # scalar vector of length nsolve
    with pytest.raises(ValueError):
        mf.sample([vec], np.zeros((3, 4)))                    # points not (2, npts)
    with pytest.raises(ValueError):
        mf.sample([{"Ex_dofs": np.zeros(mf.nsolve), "Ey_dofs": np.zeros(mf.nsolve)}], pts)   # Hz_im without beta
    with pytest.raises(ValueError):
        mf.sample([{"n_eff": 1.5}], pts)                      # not a mode record
    with pytest.raises(ValueError):
        mf.sample_grid([vec], 0, 4)
    with pytest.raises(ValueError):
        mode_overlap([vec], small_mesh, [sca], small_mesh)    # mixed kinds across the two sets
    with pytest.raises(ValueError):
        mode_overlap([vec], small_mesh, [vec], small_mesh, weight="not a geometry")
    other = unit_square_mesh(4)
    with pytest.raises(ValueError):
        mode_overlap([vec], small_mesh, [vec], other)         # B's vectors do not fit mesh B
    with pytest.raises(NotImplementedError):
        mf.sample([{"field_vector": np.zeros(mf.N, dtype=complex)}], pts)
    assert mf._loc is None                                    # nothing reached the device
    assert mode_overlap([], small_mesh, [vec], small_mesh).shape == (0, 1)


def test_workspace_bytes_unchanged_by_the_locator(small_mesh):
    sym = _native.Symbolic(small_mesh.p, small_mesh.t)
    lib = _native.load_library()

    def ws():
        b = ctypes.c_int64(0)
        assert lib.plfem_workspace_bytes(sym._h, 65, ctypes.byref(b)) == 0
        return b.value

    before = ws()
    nb = ctypes.c_int64(0)
    assert lib.plfem_locator_bytes(sym._h, ctypes.byref(nb)) == 0 and nb.value > 0
    sym.array("loc_grid")
    assert ws() == before


def test_locator_stats_on_the_c1_mesh(c1_geometry, built_library):
    mesh = generate_mesh(c1_geometry, 1.0, 0)
    mf = ModeFields(mesh)
    st = mf.stats
    assert st["cells"] <= 2 * mesh.t.shape[1]
    assert 1.0 <= st["mean_candidates"] <= st["max_candidates"] < 500
