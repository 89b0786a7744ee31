"""Projection of modes on sampled fields on the GPU (k_mode_project_sampled + k_project_sampled_reduce) against the NumPy
emulation (tests/sampled_projection_emulation.py), every entry within ``tol = 1.2e-16 (Q + 64) S_m Fmax_f``: random P2
fields on a 512-element mesh and its shifted copy at k = 1, 33, 64 over frame counts on both sides of the kernel's frame
tile, three image sizes and three extents; bit-identical repeats and chunks; the all-ones frame against ``project``;
``field_coupling`` of sampled Gaussian spots against ``gaussian_coupling`` on solver output at C1 L = 0; and the argument
errors of the C ABI.  These mode counts run 5 of the 6 instances of ``k_mode_project_sampled``, and at most 67 frames are
one launch of the entry's loop over groups of 16 frame tiles: every instance at both ends of its range, the bits of a mode
across instances, 512 to 4096 frames in one call (two to eight groups) and meshes with fewer elements than slices are in
tests/test_gpu_field_instances.py."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from quartic_emulation import square_mesh
from sampled_projection_emulation import SampledProjectionEmulation
from pl_fem_vectoriel_amd import ModeFields, _native, field_coupling, gaussian_coupling, generate_mesh, mode_overlap
from pl_fem_vectoriel_amd.fields import PROJECT_SAMPLED_TILE
from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver

pytestmark = pytest.mark.gpu

T = PROJECT_SAMPLED_TILE
COUNTS = (1, T - 1, T, T + 1, 2 * T + 3)                 # frames: one, and both sides of one and two tiles
IMAGES = ((2, 2), (3, 5), (64, 48))                      # (nx, ny): one cell; small and odd; not square (a swapped stride shows)


@pytest.fixture(scope="module")
def squares(gpu_device, built_library):
    """The jittered 16 x 16 square on [-1, 1]^2 (512 elements, Q = 8 192) and its copy shifted by (1.0, 0.5)."""
    p, t = square_mesh(16, seed=2)
    out = {}
    for name, d in (("centred", (0.0, 0.0)), ("shifted", (1.0, 0.5))):
        q = p + np.array(d)[:, None]
        out[name] = (ModeFields(SimpleNamespace(p=q, t=t), device=gpu_device), SampledProjectionEmulation(q, t))
    yield out
    for mf, _ in out.values():
        mf.close()


def _extents(em):
    """(name, (xmin, xmax, ymin, ymax)): larger than the mesh, exactly its bounding box, cutting through it."""
    p = em.mesh.p
    x0, x1, y0, y1 = p[0].min(), p[0].max(), p[1].min(), p[1].max()
    return (("larger", (x0 - 0.3, x1 + 0.45, y0 - 0.2, y1 + 0.35)), ("bounding box", (x0, x1, y0, y1)),
            ("cutting", (x0 + 0.45, x1 + 0.2, y0 - 0.1, y0 + 1.27)))


def _axes(em, ext, nx, ny, cutting):
    x, y = np.linspace(ext[0], ext[1], nx), np.linspace(ext[2], ext[3], ny)
    if cutting:                                          # no quadrature point where rounding could decide in or out
        for _ in range(8):
            if em.edge_distance(x, y) > 1e-9:
                break
            x, y = x + 1e-3, y + 1e-3
        assert em.edge_distance(x, y) > 1e-9
        inside = em.inside(x, y)
        assert 0.25 * inside.size < inside.sum() < 0.75 * inside.size
    return x, y


def _complex(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _records(vals, indexed):
    k = vals.shape[1]
    if indexed:
        return [{"Ex_dofs": vals[0, i], "Ey_dofs": vals[1, i]} for i in range(k)]
    return [{"field_vector": vals[0, i]} for i in range(k)]


def _vals(modes):
    if "Ex_dofs" in modes[0]:
        return np.stack([np.array([m["Ex_dofs"] for m in modes]), np.array([m["Ey_dofs"] for m in modes])])
    return np.array([m["field_vector"] for m in modes])[None]


def _excess(got, ref, tol):
    assert got.shape == ref.shape and np.all(np.isfinite(got.real)) and np.all(np.isfinite(got.imag))
    return float((np.abs(got - ref) / tol).max())


@pytest.mark.parametrize("where", ["centred", "shifted"])
@pytest.mark.parametrize("k,ncomp", [(1, 1), (1, 2), (33, 1), (33, 2), (64, 1), (64, 2)])
def test_kernel_matches_emulation_on_random_fields(squares, where, k, ncomp):
    mf, em = squares[where]
    indexed = ncomp == 2                                           # interior-indexed rows: boundary DOFs drop out
    rng = np.random.default_rng(2000 * k + ncomp)
    vals = rng.standard_normal((ncomp, k, em.interior.size if indexed else em.N))
    recs = _records(vals, indexed)
    worst = 0.0
    for nx, ny in IMAGES:
        for name, ext in _extents(em):
            x, y = _axes(em, ext, nx, ny, name == "cutting")
            for nf in COUNTS:
                frames = _complex(rng, (nf, ny, nx))
                P = mf.project_sampled(recs, frames, x, y)
                assert P.shape == (ncomp, k, nf)
                ex = _excess(P, em.project_sampled(vals, indexed, frames, x, y), em.tolerance(vals, indexed, frames))
                worst = max(worst, ex)
                assert ex <= 1.0, (nx, ny, name, nf, ex)
    print(f"{where} k = {k} ncomp = {ncomp}: at most {worst:.2e} of the tolerance")


def test_same_bits_twice_and_a_real_frame(squares):
    mf, em = squares["centred"]
    rng = np.random.default_rng(7)
    vals = rng.standard_normal((2, 33, em.interior.size))
    recs = _records(vals, True)
    x, y = _axes(em, _extents(em)[2][1], 64, 48, True)
    frames = _complex(rng, (T + 1, 48, 64))
    frames[3] = frames[3].real
    P = mf.project_sampled(recs, frames, x, y)
    assert np.array_equal(P, mf.project_sampled(recs, frames, x, y))
    assert np.all(P[:, :, 3].imag == 0.0) and np.all(P[:, :, 3].real != 0.0) and np.all(P[:, :, 4].imag != 0.0)
    real = mf.project_sampled(recs, frames.real, x, y)             # a real array: as the same frames with zero imaginary parts
    assert np.all(real.imag == 0.0) and np.array_equal(real[:, :, 3], P[:, :, 3])
    assert np.array_equal(mf.project_sampled(recs, frames[3], x, y)[:, :, 0], P[:, :, 3])     # one image (ny, nx)


def test_chunks_give_the_same_bits(squares, monkeypatch):
    mf, em = squares["shifted"]
    rng = np.random.default_rng(9)
    vals = rng.standard_normal((1, 33, em.N))
    recs = _records(vals, False)
    nx, ny, nf = 64, 48, 2 * T + 3
    x, y = _axes(em, _extents(em)[0][1], nx, ny, False)
    frames = _complex(rng, (nf, ny, nx))
    whole = mf.project_sampled(recs, frames, x, y)
    per_chunk = T - 7                                              # not a multiple of the tile: the frames change columns
    assert (nf + per_chunk - 1) // per_chunk >= 3
    monkeypatch.setattr(mf, "CHUNK_BYTES", 16 * ny * nx * per_chunk)
    calls = []
    real = mf._lib.plfem_mode_project_sampled
    monkeypatch.setattr(mf._lib, "plfem_mode_project_sampled", lambda *a: (calls.append(a[11]), real(*a))[1])   # a[11] = nf
    chunked = mf.project_sampled(recs, frames, x, y)
    assert calls == [per_chunk, per_chunk, nf - 2 * per_chunk]
    assert np.array_equal(chunked, whole)


def test_all_ones_frame_against_project(squares):
    one = np.array([[0.0, 0.0, 0.0]])
    for where in ("centred", "shifted"):
        mf, em = squares[where]
        rng = np.random.default_rng(13)
        for indexed in (False, True):
            vals = rng.standard_normal((2 if indexed else 1, 33, em.interior.size if indexed else em.N))
            recs = _records(vals, indexed)
            x, y = _axes(em, _extents(em)[0][1], 5, 3, False)
            ones = np.ones((1, 3, 5))
            P = mf.project_sampled(recs, ones, x, y)
            ex = _excess(P, mf.project(recs, one, one)[:, :, :, 0], 2 * em.tolerance(vals, indexed, ones))
            print(f"{where} indexed {indexed}: all-ones frame against project, {ex:.2e} of twice the tolerance")
            assert ex <= 1.0


@pytest.fixture(scope="module")
def c1(c1_geometry, gpu_device, built_library):
    mesh = generate_mesh(c1_geometry, 1.0, 0)
    vsol = TrueVectorialMaxwellSolver(c1_geometry, device=gpu_device, eig_tol=1e-10)
    ssol = ScalarHelmholtzSolver(c1_geometry, device=gpu_device)
    vec = vsol.solve_vectorial_modes(mesh, 22)[:22]
    scal = ssol.solve(mesh, 10)[:10]
    mf = ModeFields(mesh, device=gpu_device, solver=vsol)
    yield {"mesh": mesh, "vec": vec, "scal": scal, "mf": mf, "em": SampledProjectionEmulation(mesh.p, mesh.t)}
    mf.close()
    vsol.clear_cache()
    ssol.clear_cache()
    import torch
    torch.cuda.empty_cache()


def test_sampled_gaussians_against_gaussian_coupling(c1):
    mf, em, w, h = c1["mf"], c1["em"], 1.5, 0.05
    spots = ((0.0, 0.0), (8.0, 0.0), (-4.0, 6.9))                   # on the central core, on an outer core, beside one
    x0, x1, y0, y1 = mf.bbox
    x = x0 + h * np.arange(int(np.ceil((x1 - x0) / h)) + 1)
    y = y0 + h * np.arange(int(np.ceil((y1 - y0) / h)) + 1)
    assert x[-1] >= x1 and y[-1] >= y1
    frames = np.stack([np.exp(-((x[None, :] - cx) ** 2 + (y[:, None] - cy) ** 2) / w ** 2) for cx, cy in spots])
    # bilinear interpolation: (h^2 / 8) max |f''| per axis, max |f_xx| = 2 / w^2
    delta = (h * h + h * h) / (4 * w * w)
    beam = np.pi * w * w / 2
    pol = (0.6, -0.8)
    for modes, indexed in ((c1["vec"], True), (c1["scal"], False)):
        kind = "vectorial" if indexed else "scalar"
        before = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in m.items()} for m in modes]
        vals = _vals(modes)
        S = em.scale(vals, indexed)                                  # (ncomp, k)
        tol = delta * S[:, :, None] + em.tolerance(vals, indexed, frames)
        res = field_coupling(modes, mf, frames, x, y, polarization=pol)
        given = field_coupling(modes, mf, frames, x, y, polarization=pol, power=np.full(3, beam))
        A = res["amplitude"]
        assert A.shape == (vals.shape[0], len(modes), 3) and np.array_equal(given["amplitude"], A)
        assert res["efficiency"].shape == (len(modes), 3) and res["captured"].shape == (3,) and res["power"].shape == (3,)
        norm = np.diag(mode_overlap(modes, mf, modes, mf))
        a = pol[0] * A[0] + pol[1] * A[1] if indexed else A[0]
        atol = abs(pol[0]) * tol[0] + abs(pol[1]) * tol[1] if indexed else tol[0]
        assert np.allclose(res["efficiency"], np.abs(a) ** 2 / (norm[:, None] * res["power"][None, :]), rtol=1e-12, atol=0)
        # the interpolant is within delta of the beam everywhere: in L2 over the grid within delta sqrt(area)
        area = (x[-1] - x[0]) * (y[-1] - y[0])
        assert np.all(np.abs(np.sqrt(res["power"]) - np.sqrt(beam)) <= delta * np.sqrt(area) + 1e-12), res["power"]
        assert np.array_equal(given["power"], np.full(3, beam))
        for f, (cx, cy) in enumerate(spots):
            gc = gaussian_coupling(modes, mf, w, [cx], [cy], polarization=pol)
            G = gc["amplitude"][:, :, 0, 0]
            ex = _excess(A[:, :, f], G, tol[:, :, f])
            g = pol[0] * G[0] + pol[1] * G[1] if indexed else G[0]
            # | |a|^2 - |g|^2 | <= (|a| + |g|) |a - g|, both efficiencies over the same N_m pi w^2 / 2
            etol = (np.abs(a[:, f]) + np.abs(g)) * atol[:, f] / (norm * beam)
            ee = float((np.abs(given["efficiency"][:, f] - gc["efficiency"][:, 0, 0]) / etol).max())
            print(f"{kind} spot ({cx}, {cy}): amplitude {ex:.2e}, efficiency {ee:.2e} of the tolerance; captured "
                  f"{res['captured'][f]:.6f}, power {res['power'][f]:.6f} (pi w^2 / 2 = {beam:.6f})")
            assert ex <= 1.0 and ee <= 1.0
        assert np.all(res["captured"] >= 0) and np.all(res["captured"] <= 1 + 1e-9)
        for m, b in zip(modes, before):                             # the records are untouched
            assert set(m) == set(b)
            for key in m:
                assert np.array_equal(m[key], b[key]) if isinstance(b[key], np.ndarray) else m[key] == b[key]


def test_argument_errors_through_the_c_abi(squares):
    import torch
    mf, em = squares["centred"]
    mf._ensure_locator()
    lib, loc = mf._lib, mf._loc
    k, nx, ny, nf = 3, 5, 3, 4
    rng = np.random.default_rng(11)
    vals = rng.standard_normal((1, k, em.N))
    staged, _src = mf._stage(vals)
    x, y = _axes(em, _extents(em)[0][1], nx, ny, False)
    dx, dy = (x[-1] - x[0]) / (nx - 1), (y[-1] - y[0]) / (ny - 1)
    frames = _complex(rng, (nf, ny, nx))
    dev = torch.view_as_real(torch.from_numpy(frames).to(mf.tdev)).permute(1, 2, 0, 3).contiguous()
    need = ctypes.c_int64(0)
    assert lib.plfem_project_sampled_work_bytes(1, 65, nf, ctypes.byref(need)) == _native.PLFEM_EINVAL
    assert lib.plfem_project_sampled_work_bytes(1, k, 4097, ctypes.byref(need)) == _native.PLFEM_EINVAL
    assert lib.plfem_project_sampled_work_bytes(1, k, nf, ctypes.byref(need)) == _native.PLFEM_OK
    work = torch.empty(need.value + 256, dtype=torch.uint8, device=mf.tdev)
    aligned = (work.data_ptr() + 255) & ~255
    out = np.full((1, k, nf), np.nan + 0j)

    def call(k=k, nx=nx, dx=dx, nf=nf, nbytes=need.value, frames=dev.data_ptr()):
        return lib.plfem_mode_project_sampled(loc, 1, k, ctypes.c_void_p(staged.data_ptr()), 0, nx, ny, float(x[0]), float(y[0]), dx,
                                              dy, nf, ctypes.c_void_p(frames), ctypes.c_void_p(aligned), ctypes.c_int64(nbytes),
                                              out.ctypes.data_as(ctypes.c_void_p))

    ref, tol = em.project_sampled(vals, False, frames, x, y), em.tolerance(vals, False, frames)
    for name, kw in (("k = 65", dict(k=65)), ("nx = 1", dict(nx=1)), ("dx = 0", dict(dx=0.0)), ("dx = NaN", dict(dx=np.nan)),
                     ("dx < 0", dict(dx=-dx)), ("dx = inf", dict(dx=np.inf)), ("1 / dx = inf", dict(dx=1e-310)),
                     ("nf = 4097", dict(nf=4097)), ("nf = 0", dict(nf=0)), ("null frames", dict(frames=0)),
                     ("work one short", dict(nbytes=need.value - 1))):
        assert call(**kw) == _native.PLFEM_EINVAL, name
        msg = lib.plfem_locator_last_error(loc).decode()
        assert msg.startswith("plfem_mode_project_sampled: "), (name, msg)
        assert np.all(np.isnan(out.real))                          # nothing was written
        assert call() == _native.PLFEM_OK, name                    # the locator is still usable
        assert _excess(out, ref, tol) <= 1.0, name
        out[...] = np.nan
