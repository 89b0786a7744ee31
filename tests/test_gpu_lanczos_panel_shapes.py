"""The block driver's panel dot (launch_panel_dot at P = BLOCK_P) and the first Gram-Schmidt pass (k_permute_dot_first,
its wave sums by multi_reduce), through the same hooks and against the same extended-precision reference, bound and
mutants as test_gpu_lanczos_kernels.py (lanczos_emulation.panel_dot / assert_margins), at small shapes chosen for the
tails of 16-row tiles, of a quarter chunk (one wave's share when four waves split a chunk) and of the 1024-row chunk --
where a dot kernel of either form, on the vector units or on the matrix cores, goes wrong:

* dot: n2 = 882 (55 tiles of 16 rows and 2 rows: not a multiple of 16), 1008 (one tile short of the chunk) and 1026 (one
  row PAIR past the chunk boundary: n2 = 2 N is even on every vectorial mesh; a second chunk of two rows); column counts
  around 16 (4, 12, 16, 20), around 64 (64, 68) and max_ncv rounded down to a multiple of 4; W 16-byte aligned and not;
  with and without the CGS2 accumulation; the context's memory, d_partial included, NaN before the first call and
  d_partial NaN again before every repeat;
* first pass: one partly filled segment (n2 = 882), 1024 - 1 and 1024 + 1 rows (the last segment one row, Dirichlet or
  live), three segments with Dirichlet rows (npos = -1) in the last; 4 and 8 columns;
* determinism: the same call twice with the partial sums poisoned in between, H and W bit for bit.

Meshes: structured rectangles (P2 nodes (2 nx + 1)(2 ny + 1), always odd), one of them with a corner triangle cut off
(three nodes fewer), so that n2 = 2 N = 1008 is reached."""
import functools

import numpy as np
import pytest

import lanczos_emulation as le
from pl_fem_vectoriel_amd import _native

pytestmark = pytest.mark.gpu
P = le.BLOCK_P
CHUNK = le.PANEL_CHUNK
MAX_NCV = 75
NCOLS = (4, 12, 16, 20, 64, 68, MAX_NCV // 4 * 4)
# name: (nx, ny, corner cut, unknowns per node, Dirichlet boundary)
MESHES = {"v882": (10, 10, False, 2, True), "v1008": (6, 19, True, 2, True), "v1026": (13, 9, False, 2, True),
          "v2178": (16, 16, False, 2, True), "s1023": (16, 15, False, 1, True), "s1025": (12, 20, False, 1, True),
          "s1025live": (12, 20, False, 1, False)}
DOT_MESHES = ("v882", "v1008", "v1026")
FIRST_MESHES = ("v882", "s1023", "s1025", "s1025live", "v2178")


def rectangle(nx, ny, cut):
    X, Y = np.meshgrid(np.linspace(0.0, 1.0, nx + 1), np.linspace(0.0, ny / nx, ny + 1))
    p = np.vstack([X.ravel(), Y.ravel()])
    idx = np.arange((nx + 1) * (ny + 1)).reshape(ny + 1, nx + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    t = np.hstack([np.vstack([a, b, d]), np.vstack([a, d, c])])
    if cut:                                                 # without the one triangle that owns the corner (0, ny / nx)
        keep = ~(t == idx[-1, 0]).any(axis=0)
        assert keep.sum() == t.shape[1] - 1
        t = t[:, keep]
        used = np.unique(t)
        renumber = np.full(p.shape[1], -1)
        renumber[used] = np.arange(used.size)
        p, t = p[:, used], renumber[t]
    return p, t


class Shape:
    """A context on one of the meshes, created with its device memory NaN, and the data the tests of the mesh share."""

    def __init__(self, name, device):
        import torch
        self.torch, self.name = torch, name
        nx, ny, cut, dpn, dirichlet = MESHES[name]
        p, t = rectangle(nx, ny, cut)
        self.sym = _native.Symbolic(p, t, dofs_per_node=dpn, dirichlet=dirichlet)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(_native, "SCRATCH_FILL", float("nan"))
            self.ctx = _native.Context(self.sym, device, max_ncv=MAX_NCV)
        self.N, self.dpn, self.n2 = self.sym.N, dpn, self.ctx.n2
        assert self.n2 == int(name[1:5]), self.n2
        self.front = le.FrontOrder(self.sym)
        self.live = ~np.tile(self.sym.array("bmask").astype(bool), dpn)
        self.rng = np.random.default_rng(sorted(MESHES).index(name) + 101)
        self.chol_T, self.chol_R = self.dev(np.zeros(P * P)), self.dev(np.zeros(P * P))

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).cuda(self.ctx.device)

    @staticmethod
    def host(t):
        return t.cpu().numpy().astype(np.float64)

    def block(self, X, ld):
        n, q = X.shape
        buf = np.full((q, ld), np.nan)
        buf[:, :n] = X.T
        return self.dev(buf)

    def unblock(self, t, q, ld):
        buf = self.host(t).reshape(q, ld)
        assert np.isnan(buf[:, self.n2:]).all(), "a gap between the columns was written"
        return buf[:, :self.n2].T.copy()

    def random(self, *shape, live=False):
        X = self.rng.uniform(0.5, 1.5, shape) * self.rng.choice((-1.0, 1.0), shape)
        if live:
            X[~self.live] = 0.0
        return X

    def poison_partials(self, count):
        """The first ``count`` doubles of d_partial NaN: the CholQR hook copies the partials it is handed there (its own
        result, the factor of a NaN matrix, is dropped)."""
        nch = -(-count // (P * P))
        self.ctx.debug_chol(self.dev(np.full(P * P * nch, np.nan)), 0, True, nch, self.chol_T, P, self.chol_R)

    # -- shared, never modified
    @functools.cached_property
    def dot_data(self):
        Pm_h, W_h = self.random(self.n2, max(NCOLS)), self.random(self.n2, P)
        href, hbnd = le.panel_dot(Pm_h, W_h)
        return Pm_h, W_h, self.dev(Pm_h.T), href, hbnd

    @functools.cached_property
    def first_data(self):
        X = self.random(self.n2, P)
        xl_h = self.front.permute_in(X, fill=np.nan)
        Wglob = self.front.permute_out(xl_h)
        assert np.isfinite(Wglob).all() and np.array_equal(Wglob[~self.live], np.zeros(((~self.live).sum(), P)))
        BVm_h, Vm_h = self.random(self.n2, 8, live=True), self.random(self.n2, 8, live=True)
        href, hbnd = le.panel_dot(BVm_h, Wglob)
        return Wglob, BVm_h, Vm_h, self.dev(xl_h), self.dev(BVm_h.T), self.dev(Vm_h.T), href, hbnd


@pytest.fixture(scope="module")
def shapes(gpu_device, built_library):
    @functools.lru_cache(maxsize=None)
    def get(name):
        return Shape(name, gpu_device)
    return get


def ok(gpu, ref, bound, what):
    assert np.isfinite(gpu).all(), f"{what}: non-finite result"
    r = le.within(gpu, ref, bound)
    assert r <= 1.0, f"{what}: {r:.3g} times the bound"


def test_the_meshes_reach_their_shapes(shapes):
    """What the shapes are chosen for: the tails of the dot's tiles, waves and chunks, and where the Dirichlet rows fall."""
    assert shapes("v882").n2 % 16 == 2 and shapes("v882").n2 < CHUNK
    assert shapes("v1008").n2 == CHUNK - 16
    assert shapes("v1026").n2 == CHUNK + 2
    assert all(shapes(m).n2 % 2 == 0 for m in DOT_MESHES)
    assert 64 in NCOLS and 68 in NCOLS and max(NCOLS) == 72 and max(NCOLS) <= MAX_NCV + P
    for name, in_last in (("v882", 160), ("s1023", 124), ("s1025", 1), ("s1025live", 0), ("v2178", 21)):
        s = shapes(name)
        last = (s.n2 - 1) // CHUNK * CHUNK
        assert (~s.live[last:]).sum() == in_last, name
    assert shapes("s1023").n2 == CHUNK - 1 and shapes("s1025").n2 == CHUNK + 1 and shapes("v2178").n2 > 2 * CHUNK


@pytest.mark.parametrize("ncols", NCOLS)
@pytest.mark.parametrize("name", DOT_MESHES)
def test_block_panel_dot_shapes(shapes, name, ncols):
    c = shapes(name)
    n2 = c.n2
    Pm_h, W_h, Pm, href, hbnd = c.dot_data
    href, hbnd = href[:ncols], hbnd[:ncols]
    le.assert_margins(href, hbnd, le.panel_dot_mutants(Pm_h[:, :ncols], W_h, href))
    nchunks = -(-n2 // CHUNK)
    assert nchunks == (2 if name == "v1026" else 1) and n2 % 2 == 0
    ldh = ncols + 3
    for ldw in (n2 + 37, n2 + 38):                          # W columns 8-byte and 16-byte aligned
        Wd = c.block(W_h, ldw)
        c.poison_partials(nchunks * ncols * P)
        H = c.dev(np.full((P, ldh), np.nan))
        c.ctx.debug_panel("dot_block", ncols, Pm, Wd, ldw, H, ldh)
        Hh = c.host(H).reshape(P, ldh)
        assert np.isnan(Hh[:, ncols:]).all()
        h = Hh[:, :ncols].T
        ok(h, href, hbnd, f"dot_block {name} ncols={ncols} ldw={ldw}")
        assert np.array_equal(c.unblock(Wd, P, ldw), W_h), "the dot wrote W"
        # the same call after the partial sums were poisoned: the same bits
        c.poison_partials(nchunks * ncols * P)
        H2 = c.dev(np.full((P, ldh), np.nan))
        c.ctx.debug_panel("dot_block", ncols, Pm, Wd, ldw, H2, ldh)
        assert np.array_equal(c.host(H2), c.host(H), equal_nan=True), "panel dot not deterministic"
        # CGS2: hacc += h, the same h bits into both outputs
        acc0 = c.random(ncols, P)
        ldacc = ncols + 1
        acc = c.dev(np.vstack([acc0, np.full((1, P), np.nan)]).T)
        c.poison_partials(nchunks * ncols * P)
        c.ctx.debug_panel("dot_block", ncols, Pm, Wd, ldw, H2, ldh, hacc=acc, ldacc=ldacc)
        Ah = c.host(acc).reshape(P, ldacc)
        assert np.isnan(Ah[:, ncols]).all()
        assert np.array_equal(Ah[:, :ncols].T, acc0 + h), "hacc != old hacc + h"
        assert np.array_equal(c.host(H2), c.host(H), equal_nan=True)


@pytest.mark.parametrize("ncols", (4, 8))
@pytest.mark.parametrize("name", FIRST_MESHES)
def test_first_pass_shapes(shapes, name, ncols):
    c = shapes(name)
    n2, ldw = c.n2, c.n2 + 37
    Wglob, BVm_h, Vm_h, xl, BVm, Vm, href, hbnd = c.first_data
    href, hbnd = href[:ncols], hbnd[:ncols]
    mutants = le.panel_dot_mutants(BVm_h[:, :ncols], Wglob, href)
    if name == "s1025":                                     # (its last chunk is one Dirichlet row: counted twice it changes nothing)
        assert not c.live[CHUNK:].any()
        del mutants["last_chunk_twice"]
    le.assert_margins(href, hbnd, mutants)
    nseg = -(-n2 // CHUNK)
    ldh = ncols + 2
    runs = []
    for _ in range(2):
        c.poison_partials(8 * P * nseg)
        Wd = c.block(np.full((n2, P), 7.0), ldw)
        Ho = c.dev(np.full((P, ldh), np.nan))
        c.ctx.debug_first_pass(xl, BVm, Vm, ncols, Wd, ldw, Ho, ldh)
        runs.append((c.host(Ho), c.unblock(Wd, P, ldw)))
    Hh = runs[0][0].reshape(P, ldh)
    assert np.isnan(Hh[:, ncols:]).all()
    h = Hh[:, :ncols].T
    ok(h, href, hbnd, f"first pass Hout {name} ncols={ncols}")
    Wn = runs[0][1]
    wref, wbnd = le.panel_axpy(Wglob, Vm_h[:, :ncols], h)
    ok(Wn, wref, wbnd, f"first pass update {name} ncols={ncols}")
    le.assert_margins(wref, wbnd, le.panel_axpy_mutants(Wglob, Vm_h[:, :ncols], h))
    assert np.array_equal(Wn[~c.live], np.zeros(((~c.live).sum(), P)))
    assert np.array_equal(runs[1][0], runs[0][0], equal_nan=True), "first pass H not deterministic"
    assert np.array_equal(runs[1][1], runs[0][1]), "first pass W not deterministic"
    # the pass alone (Vm = 0) leaves exactly the permuted block
    Wd = c.block(np.full((n2, P), 7.0), ldw)
    c.ctx.debug_first_pass(xl, BVm, c.dev(np.zeros((8, n2))), ncols, Wd, ldw, c.dev(np.full((P, ldh), np.nan)), ldh)
    assert np.array_equal(c.unblock(Wd, P, ldw), Wglob), "W != permuted d_xl"
