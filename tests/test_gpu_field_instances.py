"""Every compiled instance and every launch group of the projection calls, and the small-mesh regime of the quartic overlap
(DESIGN.md section 33).  ``test_gpu_projection.py`` and ``test_gpu_sampled_projection.py`` cover the mode and factor / frame
counts around one tile; this file aims the same NumPy emulations and their rounding-bound tolerances at what the host
code chooses between:

* the 12 instances of ``k_mode_project<MAXT>`` and the 6 of ``k_mode_project_sampled<NFT>``, each at the smallest and the
  largest field count ``nf = ncomp k`` that reaches it (``INSTANCE_PAIRS``, derived from the two rules restated below), and
  the bits of a mode across instances: a mode's result does not depend on how many modes share its call;
* the frame groups of ``plfem_mode_project_sampled`` (16 tiles of 32 frames per launch): one group exactly, one frame
  and one tile into the second, a ragged last tile, all 8 groups; the bits of a frame whatever it is batched with; and
  that no group reads the partial tiles of the group before;
* the tile regimes of ``plfem_mode_project``: one slice (more than 512 tiles), ``1024 / tiles == 0``, thin tile grids;
* meshes with fewer elements than element slices in ``project``, ``project_sampled`` and ``quartic``, on a fresh work
  buffer and on one pre-filled with 0xFF bytes.

Every bound is the one of the existing test of the same kernel (imported), or bit equality."""
import ctypes
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np
import pytest

import power_cases
from projection_emulation import ProjectionEmulation
from quartic_emulation import square_mesh
from sampled_projection_emulation import SampledProjectionEmulation
from test_gpu_nonlinear import QUARTIC_TOL
from test_gpu_projection import TX, TY, _excess, _family, _records
from test_gpu_sampled_projection import T, _axes, _complex, _extents
from pl_fem_vectoriel_amd import ModeFields, _native
from pl_fem_vectoriel_amd.fields import PROJECT_SAMPLED_MAX_FRAMES
from pl_fem_vectoriel_amd.mesh import unit_square_mesh

pytestmark = pytest.mark.gpu

# ---- the host's rules, restated (csrc/kernels_fields.hip: project_plan, sampled_plan, quartic_slices) -----------------
MAXT_COMPILED = (2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32)     # k_mode_project<MAXT>: ncomp k <= 4 MAXT
NFT_COMPILED = (1, 2, 3, 4, 6, 8)                                # k_mode_project_sampled<NFT>: ncomp k <= 16 NFT
KMAX = 64                                                        # PJ_KMAX, QKMAX
PJ_SLICES, PJ_WG = 256, 1024
PS_SLICES, PS_GROUP = 128, 16
QP, QB_MAX, QWG = 64, 128, 2048


def maxt_of(nf):
    """The instance of k_mode_project: ceil(nf / 4), rounded to even up to 16 and to a multiple of 4 above."""
    m = (nf + 3) // 4
    return m + (m % 2 if m <= 16 else (4 - m % 4) % 4)


def nft_of(nf):
    """The instance of k_mode_project_sampled: ceil(nf / 16), 5 rounded to 6 and 7 to 8."""
    n = (nf + 15) // 16
    return {5: 6, 7: 8}.get(n, n)


def project_slices(la, lb):
    tiles = ((la + TX - 1) // TX) * ((lb + TY - 1) // TY)
    return max(1, min(PJ_SLICES, PJ_WG // tiles))


def quartic_slices(k):
    tiles = (k * (k + 1) // 2 + QP - 1) // QP
    return max(1, min(QB_MAX, QWG // (tiles * (tiles + 1) // 2)))


def _pairs_of(nf):
    """Every (k, ncomp) with ncomp k = nf: a scalar call when nf <= 64, a vectorial one when nf is even."""
    return [(nf // c, c) for c in (1, 2) if nf % c == 0 and nf // c <= KMAX]


REACHABLE = sorted({c * k for c in (1, 2) for k in range(1, KMAX + 1)})
# the smallest and the largest reachable nf of every instance of either kernel, and every call that has that nf
EDGES = sorted({f(nf for nf in REACHABLE if rule(nf) == v) for rule, values in ((maxt_of, MAXT_COMPILED), (nft_of, NFT_COMPILED))
                for v in values for f in (min, max)})
ALREADY = ((1, 1), (1, 2), (33, 1), (33, 2), (64, 1), (64, 2))    # the pairs of the two projection test files
INSTANCE_PAIRS = sorted({p for nf in EDGES for p in _pairs_of(nf)} | set(ALREADY), key=lambda p: (p[0] * p[1], p[1]))
# mode counts, by ncomp, whose calls run different instances: between them all 12 of MAXT and all 6 of NFT
BITS_K = {1: (8, 9, 17, 25, 33, 41, 49, 57, 64), 2: (4, 8, 12, 20, 28, 40, 48, 56, 64)}

GROUP_FRAMES = PS_GROUP * T                                      # 512: the frames of one launch
GROUP_COUNTS = (GROUP_FRAMES, GROUP_FRAMES + 1, GROUP_FRAMES + T, GROUP_FRAMES + T + 3)
GROUP_K = {1: 3, 2: 9}                                           # modes of the group tests, by ncomp
REGIMES = ((184, 184), (264, 250), (3, 320), (320, 3))           # (la, lb) of the tile regimes
REGIME_K = {1: 2, 2: 3}
SMALL_N = (1, 2, 5)                                              # unit_square_mesh(n): 2, 8 and 50 elements
SMALL_COUNTS = ((5, 3), (TX + 1, TY - 1))
# quartic overlaps on the small meshes: every (n, k) of k = 1, 12, 64 with fewer elements than the call's slices
QUARTIC_CASES = tuple((n, k) for n in SMALL_N for k in (1, 12, 64) if 2 * n * n < quartic_slices(k))
QUARTIC_WEIGHTS = (2.5, 0.25)


# ---- fixtures and helpers ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def square(gpu_device, built_library):
    """The jittered 16 x 16 square of the projection tests (512 elements, Q = 8 192) and its two emulations."""
    p, t = square_mesh(16, seed=2)
    mf = ModeFields(SimpleNamespace(p=p, t=t), device=gpu_device)
    yield SimpleNamespace(mf=mf, pj=ProjectionEmulation(p, t), ps=SampledProjectionEmulation(p, t))
    mf.close()


@pytest.fixture(scope="module")
def small(gpu_device, built_library):
    """{n: unit_square_mesh(n)} with 2 n^2 elements, each with its ModeFields and emulations."""
    out = {}
    for n in SMALL_N:
        m = unit_square_mesh(n)
        out[n] = SimpleNamespace(mf=ModeFields(m, device=gpu_device), pj=ProjectionEmulation(m.p, m.t),
                                 ps=SampledProjectionEmulation(m.p, m.t), ne=m.t.shape[1])
        assert out[n].ne == 2 * n * n
    yield out
    for s in out.values():
        s.mf.close()


def _random(em, ncomp, k, rng):
    """Seeded random DOF values (ncomp, k, rows) and their records: interior-indexed rows for ncomp = 2."""
    indexed = ncomp == 2
    vals = rng.standard_normal((ncomp, k, em.interior.size if indexed else em.N))
    return vals, _records(vals, indexed), indexed


@contextmanager
def _scratch_filled(monkeypatch, fill, sizes):
    """Every device buffer the package hands to the library holds ``fill`` in every byte; ``sizes`` collects the sizes."""
    import torch

    def filled(nbytes, tdev):
        sizes.append(int(nbytes))
        buf = torch.full((int(nbytes),), fill, dtype=torch.uint8, device=tdev)
        torch.cuda.current_stream(tdev).synchronize()             # the calls run on the locator's own stream
        return buf

    with monkeypatch.context() as mp:
        mp.setattr(_native, "device_scratch", filled)
        yield


def _work_bytes(mf, sizer, *sizes):
    need = ctypes.c_int64(0)
    assert getattr(mf._lib, sizer)(*sizes, ctypes.byref(need)) == _native.PLFEM_OK
    return int(need.value)


def _same_on_filled_work(monkeypatch, mf, sizer, sizes, fills, call):
    """``call()`` on a fresh work buffer and on buffers pre-filled with each of ``fills``: the same bits.  The work buffer
    of the call (``sizer(*sizes) + 256`` bytes) is among the filled ones."""
    plain = call()
    mf._ensure_locator()
    need = _work_bytes(mf, sizer, *sizes)
    for fill in fills:
        seen = []
        with _scratch_filled(monkeypatch, fill, seen):
            again = call()
        assert need + 256 in seen, (sizer, sizes, seen)
        assert np.array_equal(plain, again), (sizer, sizes, fill)
    return plain


@contextmanager
def _spy(monkeypatch, mf, fn, pick):
    """The calls of the C entry ``fn`` made meanwhile, each as ``pick(args)``."""
    calls = []
    mf._ensure_locator()                                           # (the library is loaded with the locator)
    real = getattr(mf._lib, fn)
    with monkeypatch.context() as mp:
        mp.setattr(mf._lib, fn, lambda *a: (calls.append(pick(a)), real(*a))[1])
        yield calls


# ---- A. every instance of the two projection kernels, at both ends of its range ----------------------------------------
@pytest.mark.parametrize("k,ncomp", INSTANCE_PAIRS)
def test_project_in_every_instance(square, k, ncomp):
    mf, em = square.mf, square.pj
    rng = np.random.default_rng(3000 * k + ncomp)
    vals, recs, indexed = _random(em, ncomp, k, rng)
    xf, yf = _family(TX + 1, rng), _family(TY - 1, rng)
    P = mf.project(recs, xf, yf)
    assert P.shape == (ncomp, k, TY - 1, TX + 1)
    ex = _excess(P, em.project(vals, indexed, xf, yf), em.tolerance(vals, indexed, xf, yf))
    print(f"project k = {k} ncomp = {ncomp} (nf = {ncomp * k}, MAXT = {maxt_of(ncomp * k)}): {ex:.2e} of the tolerance")
    assert ex <= 1.0


@pytest.mark.parametrize("k,ncomp", INSTANCE_PAIRS)
def test_project_sampled_in_every_instance(square, k, ncomp):
    mf, em = square.mf, square.ps
    rng = np.random.default_rng(4000 * k + ncomp)
    vals, recs, indexed = _random(em, ncomp, k, rng)
    nx, ny = 64, 48
    x, y = _axes(em, dict(_extents(em))["cutting"], nx, ny, True)
    frames = _complex(rng, (T + 1, ny, nx))
    P = mf.project_sampled(recs, frames, x, y)
    assert P.shape == (ncomp, k, T + 1)
    ex = _excess(P, em.project_sampled(vals, indexed, frames, x, y), em.tolerance(vals, indexed, frames))
    print(f"project_sampled k = {k} ncomp = {ncomp} (nf = {ncomp * k}, NFT = {nft_of(ncomp * k)}): {ex:.2e} of the tolerance")
    assert ex <= 1.0


@pytest.mark.parametrize("ncomp", [1, 2])
def test_a_mode_has_the_same_bits_in_every_instance(square, ncomp):
    """A field's row of the MFMA tile is formed from its own column of s_u and from operands shared by all fields, so the
    result of mode m depends neither on the modes that share its call nor on the instance that ran."""
    mf, em = square.mf, square.ps
    ks = BITS_K[ncomp]
    assert len({maxt_of(ncomp * k) for k in ks}) >= 8 and len({nft_of(ncomp * k) for k in ks}) >= 4
    rng = np.random.default_rng(17 + ncomp)
    vals, recs, indexed = _random(em, ncomp, KMAX, rng)
    xf, yf = _family(TX + 1, rng), _family(TY - 1, rng)
    nx, ny = 64, 48
    x, y = _axes(em, dict(_extents(em))["cutting"], nx, ny, True)
    frames = _complex(rng, (T + 1, ny, nx))
    whole, whole_s = mf.project(recs, xf, yf), mf.project_sampled(recs, frames, x, y)
    assert np.abs(whole).max(axis=(2, 3)).min() > 0 and np.abs(whole_s).min() > 0
    for k in ks[:-1]:
        P, S = mf.project(recs[:k], xf, yf), mf.project_sampled(recs[:k], frames, x, y)
        same, same_s = np.array_equal(P, whole[:, :k]), np.array_equal(S, whole_s[:, :k])
        print(f"ncomp = {ncomp}: k = {k} (MAXT = {maxt_of(ncomp * k)}, NFT = {nft_of(ncomp * k)}) against k = {KMAX}: project "
              f"{'same bits' if same else 'DIFFERENT'}, project_sampled {'same bits' if same_s else 'DIFFERENT'}")
        assert same and same_s, (ncomp, k)


# ---- B. the frame groups of the sampled projection ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def grouped(square):
    """By ncomp: GROUP_K modes, the 547 frames of the largest count on a 3 x 5 image larger than the mesh, the emulation
    and its tolerance for all of them (computed once; a frame's reference does not depend on the others), and the GPU
    result of the one call with all 547."""
    em, out = square.ps, {}
    nx, ny, nf = 3, 5, GROUP_COUNTS[-1]
    x, y = _axes(em, dict(_extents(em))["larger"], nx, ny, False)
    for ncomp, k in GROUP_K.items():
        rng = np.random.default_rng(23 + ncomp)
        vals, recs, indexed = _random(em, ncomp, k, rng)
        frames = _complex(rng, (nf, ny, nx))
        out[ncomp] = SimpleNamespace(recs=recs, frames=frames, x=x, y=y, ref=em.project_sampled(vals, indexed, frames, x, y),
                                     tol=em.tolerance(vals, indexed, frames), whole=square.mf.project_sampled(recs, frames, x, y))
    return out


def _nf_of(args):
    return args[11]                                                # plfem_mode_project_sampled(..., dy, nf, frames, ...)


@pytest.mark.parametrize("nf", GROUP_COUNTS)
@pytest.mark.parametrize("ncomp", [1, 2])
def test_frame_counts_past_one_group(square, grouped, monkeypatch, ncomp, nf):
    """One group exactly, one frame into the second, exactly 17 tiles, a ragged last tile in the second group."""
    g = grouped[ncomp]
    with _spy(monkeypatch, square.mf, "plfem_mode_project_sampled", _nf_of) as calls:
        P = square.mf.project_sampled(g.recs, g.frames[:nf], g.x, g.y)
    assert calls == [nf]                                           # one C call: the groups are the library's own loop
    ex = _excess(P, g.ref[:, :, :nf], g.tol[:, :, :nf])
    print(f"ncomp = {ncomp} k = {GROUP_K[ncomp]}: {nf} frames in {-(-nf // GROUP_FRAMES)} groups: {ex:.2e} of the tolerance")
    assert ex <= 1.0


@pytest.mark.parametrize("ncomp", [1, 2])
def test_a_frame_has_the_same_bits_in_any_group(square, grouped, ncomp):
    mf, g = square.mf, grouped[ncomp]
    n = GROUP_FRAMES
    assert np.array_equal(mf.project_sampled(g.recs, g.frames[:n], g.x, g.y), g.whole[:, :, :n])
    assert np.array_equal(mf.project_sampled(g.recs, g.frames[n:], g.x, g.y), g.whole[:, :, n:])
    pick = np.random.default_rng(29).permutation(g.frames.shape[0])[:40]
    pick[:2] = (n + 3, n - 1)                                      # frames of both groups, out of order
    assert len(set(pick)) == 40
    assert np.array_equal(mf.project_sampled(g.recs, g.frames[pick], g.x, g.y), g.whole[:, :, pick])


@pytest.mark.parametrize("ncomp", [1, 2])
def test_no_group_reads_the_partial_tiles_of_the_group_before(square, grouped, ncomp):
    """The second group's partial tiles overwrite the first group's in the work buffer.  Zero frames in one group and
    random ones in the other, both ways: a reduce that read the other group's tiles would fail one of the two."""
    mf, g = square.mf, grouped[ncomp]
    n = GROUP_FRAMES
    frames = g.frames.copy()
    frames[:n] = 0.0
    P = mf.project_sampled(g.recs, frames, g.x, g.y)
    assert np.all(P[:, :, :n] == 0.0)
    assert np.abs(P[:, :, n:]).min() > 0 and np.array_equal(P[:, :, n:], mf.project_sampled(g.recs, frames[n:], g.x, g.y))
    frames = g.frames.copy()
    frames[n:] = 0.0
    P = mf.project_sampled(g.recs, frames, g.x, g.y)
    assert np.all(P[:, :, n:] == 0.0)
    assert np.abs(P[:, :, :n]).min() > 0 and np.array_equal(P[:, :, :n], g.whole[:, :, :n])


@pytest.mark.parametrize("ncomp", [1, 2])
def test_the_most_frames_of_one_call(small, monkeypatch, ncomp):
    """4096 frames, 8 groups, on the 8-element mesh with a 2 x 2 image, whatever the work buffer held."""
    s = small[2]
    mf, em, nf, k = s.mf, s.ps, PROJECT_SAMPLED_MAX_FRAMES, GROUP_K[ncomp]
    assert nf == 8 * GROUP_FRAMES
    rng = np.random.default_rng(31 + ncomp)
    vals, recs, indexed = _random(em, ncomp, k, rng)
    x, y = _axes(em, dict(_extents(em))["larger"], 2, 2, False)
    frames = _complex(rng, (nf, 2, 2))
    with _spy(monkeypatch, mf, "plfem_mode_project_sampled", _nf_of) as calls:
        P = _same_on_filled_work(monkeypatch, mf, "plfem_project_sampled_work_bytes", (ncomp, k, nf), (0xFF, 0),
                                 lambda: mf.project_sampled(recs, frames, x, y))
    assert calls == [nf] * 3
    ex = _excess(P, em.project_sampled(vals, indexed, frames, x, y), em.tolerance(vals, indexed, frames))
    print(f"ncomp = {ncomp} k = {k}: {nf} frames in 8 groups on {s.ne} elements: {ex:.2e} of the tolerance")
    assert ex <= 1.0


# ---- C. tile regimes of plfem_mode_project -----------------------------------------------------------------------------
def _lb_of(args):
    return args[7]                                                 # plfem_mode_project(..., la, xfac, lb, yfac, ...)


@pytest.fixture(scope="module")
def regime_modes(square):
    out = {}
    for ncomp, k in REGIME_K.items():
        out[ncomp] = _random(square.pj, ncomp, k, np.random.default_rng(37 + ncomp))
    return out


@pytest.mark.parametrize("la,lb", REGIMES)
@pytest.mark.parametrize("ncomp", [1, 2])
def test_project_tile_regimes(square, regime_modes, monkeypatch, ncomp, la, lb):
    """529 tiles (one slice), 1056 tiles (1024 / tiles == 0), and 1 x 40 and 40 x 1 tile grids."""
    mf, em = square.mf, square.pj
    ntx, nty = -(-la // TX), -(-lb // TY)
    assert {(184, 184): ntx * nty == 529 and project_slices(la, lb) == 1, (264, 250): ntx * nty == 1056 and PJ_WG // 1056 == 0,
            (3, 320): (ntx, nty) == (1, 40), (320, 3): (ntx, nty) == (40, 1)}[la, lb]
    vals, recs, indexed = regime_modes[ncomp]
    rng = np.random.default_rng(41 * la + lb)
    xf, yf = _family(la, rng), _family(lb, rng)
    with _spy(monkeypatch, mf, "plfem_mode_project", _lb_of) as calls:
        P = mf.project(recs, xf, yf)
    assert calls == [lb] and P.shape == (ncomp, REGIME_K[ncomp], lb, la)
    ex = _excess(P, em.project(vals, indexed, xf, yf), em.tolerance(vals, indexed, xf, yf))
    print(f"ncomp = {ncomp} k = {REGIME_K[ncomp]}: {la} x {lb} factors, {ntx} x {nty} tiles, {project_slices(la, lb)} slices: "
          f"{ex:.2e} of the tolerance")
    assert ex <= 1.0


@pytest.mark.parametrize("ncomp", [1, 2])
def test_one_slice_gives_the_same_bits_with_fewer_y_factors(square, regime_modes, ncomp):
    """(184, 184) and (184, 177): the same slice count (1) and the same ntx, one live column in the last y tile."""
    la, lb, fewer = 184, 184, 177
    assert project_slices(la, lb) == project_slices(la, fewer) == 1 and -(-lb // TY) == -(-fewer // TY) and fewer % TY == 1
    _, recs, _ = regime_modes[ncomp]
    rng = np.random.default_rng(43)
    xf, yf = _family(la, rng), _family(lb, rng)
    assert np.array_equal(square.mf.project(recs, xf, yf)[:, :, :fewer], square.mf.project(recs, xf, yf[:fewer]))


# ---- D. meshes with fewer elements than slices -------------------------------------------------------------------------
@pytest.mark.parametrize("la,lb", SMALL_COUNTS)
@pytest.mark.parametrize("ncomp", [1, 2])
@pytest.mark.parametrize("n", SMALL_N)
def test_project_on_fewer_elements_than_slices(small, monkeypatch, n, ncomp, la, lb):
    s = small[n]
    assert s.ne < project_slices(la, lb)
    rng = np.random.default_rng(100 * n + 10 * ncomp + la)
    k = 3
    vals, recs, indexed = _random(s.pj, ncomp, k, rng)
    xf, yf = _family(la, rng), _family(lb, rng)
    P = _same_on_filled_work(monkeypatch, s.mf, "plfem_project_work_bytes", (ncomp, k, la, lb), (0xFF,),
                             lambda: s.mf.project(recs, xf, yf))
    ex = _excess(P, s.pj.project(vals, indexed, xf, yf), s.pj.tolerance(vals, indexed, xf, yf))
    print(f"project on {s.ne} elements, {project_slices(la, lb)} slices planned, ncomp = {ncomp}, {la} x {lb}: {ex:.2e} of the "
          f"tolerance")
    assert ex <= 1.0


@pytest.mark.parametrize("ncomp", [1, 2])
@pytest.mark.parametrize("n", SMALL_N)
def test_project_sampled_on_fewer_elements_than_slices(small, monkeypatch, n, ncomp):
    s = small[n]
    assert s.ne < PS_SLICES
    rng = np.random.default_rng(200 * n + ncomp)
    k, nx, ny, nf = 3, 3, 5, T + 1
    vals, recs, indexed = _random(s.ps, ncomp, k, rng)
    x, y = _axes(s.ps, dict(_extents(s.ps))["larger"], nx, ny, False)
    frames = _complex(rng, (nf, ny, nx))
    P = _same_on_filled_work(monkeypatch, s.mf, "plfem_project_sampled_work_bytes", (ncomp, k, nf), (0xFF,),
                             lambda: s.mf.project_sampled(recs, frames, x, y))
    ex = _excess(P, s.ps.project_sampled(vals, indexed, frames, x, y), s.ps.tolerance(vals, indexed, frames))
    print(f"project_sampled on {s.ne} elements, {PS_SLICES} slices planned, ncomp = {ncomp}: {ex:.2e} of the tolerance")
    assert ex <= 1.0


@pytest.mark.parametrize("ncomp", [1, 2])
@pytest.mark.parametrize("n,k", QUARTIC_CASES)
def test_quartic_on_fewer_elements_than_slices(small, monkeypatch, n, k, ncomp):
    s = small[n]
    assert s.ne < quartic_slices(k)
    rng = np.random.default_rng(300 * n + 3 * k + ncomp)
    vals, recs, indexed = _random(s.pj, ncomp, k, rng)
    disc = power_cases.discs([[0.5, 0.5]], [0.3])
    for geom, w in ((None, (1.0, 1.0)), (disc, QUARTIC_WEIGHTS)):
        Q = _same_on_filled_work(monkeypatch, s.mf, "plfem_quartic_work_bytes", (ncomp, k), (0xFF,),
                                 lambda: s.mf.quartic(recs, geom, w))
        ref = s.pj.quartic(vals, indexed, geom, w)
        err = np.abs(Q - ref).max() / np.abs(ref).max()
        print(f"quartic on {s.ne} elements, {quartic_slices(k)} slices planned, ncomp = {ncomp} k = {k} weights "
              f"{geom is not None}: {err / QUARTIC_TOL:.2e} of the tolerance")
        assert np.array_equal(Q, Q.T) and err <= QUARTIC_TOL
