"""Projection of modes on plane waves and Gaussian beams on the GPU (k_mode_project + k_project_reduce) against the NumPy
emulation (tests/projection_emulation.py), every entry within ``tol_m = 1.2e-16 (Q + 64 + 8 Phi) S_m``: random P2 fields
on a 512-element mesh and its shifted copy at k = 1, 33, 64 over factor counts on both sides of the kernel's tile;
bit-identical repeats; ``far_field`` and ``gaussian_coupling`` on solver output at C1 L = 0 with the Hermitian and shift
identities; the norm of a projection against the beam's norm; and the argument errors of the C ABI.  These mode counts run
5 of the 12 instances of ``k_mode_project`` and at most 9 tiles on a mesh with more elements than slices: every instance at
both ends of its range, the bits of a mode across instances, the tile regimes (one slice, more than 1024 tiles, thin tile
grids) and meshes with fewer elements than slices are in tests/test_gpu_field_instances.py."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from projection_emulation import ProjectionEmulation
from quartic_emulation import square_mesh
from pl_fem_vectoriel_amd import ModeFields, _native, far_field, gaussian_coupling, generate_mesh, mode_overlap
from pl_fem_vectoriel_amd.fields import PROJECT_TILE
from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver

pytestmark = pytest.mark.gpu

TX, TY = PROJECT_TILE
# x- and y-factor counts: 1 x 1, 5 x 3, one below / at / one above the kernel's tile on each axis, and a pair of which
# neither is a multiple of 16 (3 x 3 tiles)
COUNTS = ((1, 1), (5, 3), (TX - 1, TY + 1), (TX, TY), (TX + 1, TY - 1), (21, 19))


@pytest.fixture(scope="module")
def squares(gpu_device, built_library):
    """The jittered 16 x 16 square on [-1, 1]^2 (512 elements, Q = 8 192) and its copy shifted to x in [0, 2]."""
    p, t = square_mesh(16, seed=2)
    out = {}
    for name, d in (("centred", (0.0, 0.0)), ("shifted", (1.0, 0.5))):
        q = p + np.array(d)[:, None]
        out[name] = (ModeFields(SimpleNamespace(p=q, t=t), device=gpu_device), ProjectionEmulation(q, t))
    yield out
    for mf, _ in out.values():
        mf.close()


def _family(n, rng):
    """n factors (c, s, kappa): plane waves with kappa = 0 and +-kappa pairs up to 250 (500 rad on the shifted mesh),
    Gaussians of w = 0.05 .. 10 centred inside the mesh and far outside it (exp underflows to 0), then random ones."""
    pool = [(0.0, 0.0, 0.0), (0.0, 0.0, 250.0), (0.0, 0.0, -250.0), (0.3, 1 / 0.05 ** 2, 10.0), (-0.5, 1 / 10.0 ** 2, -40.0),
            (50.0, 1 / 0.5 ** 2, 1.0), (0.0, 0.0, 3.7), (0.0, 0.0, -3.7), (0.9, 1.0, 250.0), (-300.0, 1 / 0.05 ** 2, -7.0),
            (1.7, 1 / 0.2 ** 2, 0.0)]
    rows = [pool[i] for i in rng.permutation(len(pool))[:n]]
    while len(rows) < n:
        w = 10 ** rng.uniform(np.log10(0.05), 1.0)
        rows.append((rng.uniform(-1.5, 2.5), 0.0 if rng.random() < 0.3 else 1 / w ** 2, rng.uniform(-250.0, 250.0)))
    return np.array(rows)


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
    rng = np.random.default_rng(1000 * k + ncomp)
    vals = rng.standard_normal((ncomp, k, em.interior.size if indexed else em.N))
    recs = _records(vals, indexed)
    for la, lb in COUNTS:
        xf, yf = _family(la, rng), _family(lb, rng)
        P = mf.project(recs, xf, yf)
        ref = em.project(vals, indexed, xf, yf)
        assert P.shape == (ncomp, k, lb, la)
        ex = _excess(P, ref, em.tolerance(vals, indexed, xf, yf))
        print(f"{where} k = {k} ncomp = {ncomp} {la} x {lb}: {ex:.2e} of the tolerance")
        assert ex <= 1.0


def test_same_bits_twice_and_a_real_zero_wavenumber(squares):
    mf, em = squares["centred"]
    rng = np.random.default_rng(7)
    vals = rng.standard_normal((2, 33, em.interior.size))
    recs = _records(vals, True)
    xf, yf = _family(21, rng), _family(19, rng)
    xf[4], yf[7] = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
    P = mf.project(recs, xf, yf)
    assert np.array_equal(P, mf.project(recs, xf, yf))
    assert np.all(P[:, :, 7, 4].imag == 0.0) and np.all(P[:, :, 7, 4].real != 0.0)


@pytest.fixture(scope="module")
def c1(c1_geometry, gpu_device, built_library):
    mesh = generate_mesh(c1_geometry, 1.0, 0)
    vsol = TrueVectorialMaxwellSolver(c1_geometry, device=gpu_device, eig_tol=1e-10)
    ssol = ScalarHelmholtzSolver(c1_geometry, device=gpu_device)
    vec = vsol.solve_vectorial_modes(mesh, 22)[:22]
    scal = ssol.solve(mesh, 10)[:10]
    mf = ModeFields(mesh, device=gpu_device, solver=vsol)
    d = np.array([0.5, -0.25])
    moved = ModeFields(SimpleNamespace(p=mesh.p + d[:, None], t=mesh.t), device=gpu_device)
    yield {"mesh": mesh, "vec": vec, "scal": scal, "mf": mf, "em": ProjectionEmulation(mesh.p, mesh.t), "d": d, "moved": moved,
           "em_moved": ProjectionEmulation(mesh.p + d[:, None], mesh.t)}
    mf.close()
    moved.close()
    vsol.clear_cache()
    ssol.clear_cache()
    import torch
    torch.cuda.empty_cache()


def _symmetric(kmax, n):
    half = np.linspace(0.0, kmax, n // 2 + 1)
    return np.concatenate([-half[:0:-1], half])                    # exactly symmetric about 0


def _plane(kap):
    return np.stack([np.zeros_like(kap), np.zeros_like(kap), kap], 1)


def test_far_field_and_launch_map_of_solver_modes(c1, c1_geometry):
    mf, em, k0 = c1["mf"], c1["em"], c1_geometry.k0
    kx, ky = _symmetric(k0, 17), _symmetric(k0, 9)
    w, cx, cy, tilt = 1.5, np.linspace(-10.0, 10.0, 11), np.linspace(-9.0, 9.0, 5), (0.4, -0.25)
    s = 1.0 / (w * w)
    bx = np.stack([cx, np.full_like(cx, s), np.full_like(cx, tilt[0])], 1)
    by = np.stack([cy, np.full_like(cy, s), np.full_like(cy, tilt[1])], 1)
    for modes, indexed in ((c1["vec"], True), (c1["scal"], False)):
        before = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in m.items()} for m in modes]
        vals = _vals(modes)
        kind = "vectorial" if indexed else "scalar"
        ff = far_field(modes, mf, kx, ky)
        F = ff["amplitude"]
        assert F.shape == (vals.shape[0], len(modes), 9, 17) and ff["intensity"].shape == (len(modes), 9, 17)
        tol = em.tolerance(vals, indexed, _plane(kx), _plane(ky))
        ex = _excess(F, em.project(vals, indexed, _plane(kx), _plane(ky)), tol)
        print(f"{kind} far field 17 x 9, k = {len(modes)}: {ex:.2e} of the tolerance")
        assert ex <= 1.0
        assert np.allclose(ff["intensity"], (np.abs(F) ** 2).sum(0), rtol=1e-14, atol=0)
        # P(-kappa) = conj P(kappa): the axes are symmetric, so reversing both is negating kappa
        ex = _excess(F[:, :, ::-1, ::-1], np.conj(F), 2 * tol)
        print(f"{kind} Hermitian identity: {ex:.2e} of twice the tolerance")
        assert ex <= 1.0
        # the mesh translated by d: P exp(-i kappa . d)
        Fm = far_field(modes, c1["moved"], kx, ky)["amplitude"]
        d = c1["d"]
        shift = np.exp(-1j * (kx[None, :] * d[0] + ky[:, None] * d[1]))[None, None]
        ex = _excess(Fm, F * shift, 2 * c1["em_moved"].tolerance(vals, indexed, _plane(kx), _plane(ky)))
        print(f"{kind} shift identity: {ex:.2e} of twice the tolerance")
        assert ex <= 1.0

        gc = gaussian_coupling(modes, mf, w, cx, cy, tilt=tilt, polarization=(0.6, -0.8))
        A = gc["amplitude"]
        assert A.shape == (vals.shape[0], len(modes), 5, 11) and gc["efficiency"].shape == (len(modes), 5, 11)
        ex = _excess(A, em.project(vals, indexed, bx, by), em.tolerance(vals, indexed, bx, by))
        print(f"{kind} launch map 11 x 5, w = {w}, tilt {tilt}: {ex:.2e} of the tolerance")
        assert ex <= 1.0
        norm = np.diag(mode_overlap(modes, mf, modes, mf))
        a = 0.6 * A[0] - 0.8 * A[1] if indexed else A[0]
        assert np.allclose(gc["efficiency"], np.abs(a) ** 2 / (norm[:, None, None] * np.pi * w * w / 2), rtol=1e-12, atol=0)
        assert np.all(gc["efficiency"] >= 0)
        for m, b in zip(modes, before):                             # the records are untouched
            assert set(m) == set(b)
            for key in m:
                assert np.array_equal(m[key], b[key]) if isinstance(b[key], np.ndarray) else m[key] == b[key]


def test_projection_norm_is_bounded_by_the_beam_norm(c1, c1_geometry):
    mf, em, w = c1["mf"], c1["em"], 1.5
    s = 1.0 / (w * w)
    for modes, indexed, spot, tilt in ((c1["scal"], False, (0.0, 0.0), (0.0, 0.0)), (c1["scal"], False, (7.3, 1.1), (0.5, -0.3)),
                                       (c1["vec"], True, (0.0, 0.0), (0.0, 0.0)), (c1["vec"], True, (-4.2, 6.5), (-0.2, 0.7))):
        G = mf.grams(modes, c1_geometry)
        G = G["M_core"] + G["M_clad"]
        gc = gaussian_coupling(modes, mf, w, [spot[0]], [spot[1]], tilt=tilt, polarization=(0.6, -0.8))
        A = gc["amplitude"][:, :, 0, 0]
        c = 0.6 * A[0] - 0.8 * A[1] if indexed else A[0]
        captured = float(np.real(np.conj(c) @ np.linalg.solve(G, c)))
        beam = em.beam_norm([(spot[0], s, tilt[0])], [(spot[1], s, tilt[1])])
        print(f"{'vectorial' if indexed else 'scalar'} spot {spot}: c^H G^-1 c = {captured:.6f}, beam norm on the mesh "
              f"{beam:.6f}, pi w^2 / 2 = {np.pi * w * w / 2:.6f}")
        assert 0 <= captured <= (1 + 1e-9) * beam
    eff = gaussian_coupling(c1["scal"], mf, w, [0.0], [0.0])["efficiency"][:, 0, 0]
    print(f"w = {w} spot on the central core: efficiency {eff.max():.4f} into scalar mode {int(eff.argmax())}, "
          f"{eff.sum():.4f} into all {eff.size}")
    assert eff.max() > 0


def test_argument_errors_through_the_c_abi(squares):
    import torch
    mf, em = squares["centred"]
    mf._ensure_locator()
    lib, loc = mf._lib, mf._loc
    k, la, lb = 3, 5, 3
    rng = np.random.default_rng(11)
    vals = rng.standard_normal((1, k, em.N))
    staged, _src = mf._stage(vals)
    xf, yf = np.ascontiguousarray(_family(la, rng)), np.ascontiguousarray(_family(lb, rng))
    need = ctypes.c_int64(0)
    assert lib.plfem_project_work_bytes(1, 65, la, lb, ctypes.byref(need)) == _native.PLFEM_EINVAL
    assert lib.plfem_project_work_bytes(1, k, la, lb, ctypes.byref(need)) == _native.PLFEM_OK
    work = torch.empty(need.value + 256, dtype=torch.uint8, device=mf.tdev)
    aligned = (work.data_ptr() + 255) & ~255
    out = np.full((1, k, lb, la), np.nan + 0j)

    def call(k=k, la=la, lb=lb, xf=xf, yf=yf, nbytes=need.value):
        return lib.plfem_mode_project(loc, 1, k, ctypes.c_void_p(staged.data_ptr()), 0, la, xf.ctypes.data_as(ctypes.c_void_p), lb,
                                      yf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(aligned), ctypes.c_int64(nbytes),
                                      out.ctypes.data_as(ctypes.c_void_p))

    negative, nan = xf.copy(), yf.copy()
    negative[2, 1] = -1e-300
    nan[1, 0] = np.nan
    for name, kw in (("k = 65", dict(k=65)), ("la = 0", dict(la=0)), ("s < 0", dict(xf=negative)), ("NaN", dict(yf=nan)),
                     ("work one short", dict(nbytes=need.value - 1))):
        assert call(**kw) == _native.PLFEM_EINVAL, name
        msg = lib.plfem_locator_last_error(loc).decode()
        assert msg.startswith("plfem_mode_project: "), (name, msg)
        assert np.all(np.isnan(out.real))                          # nothing was written
        assert call() == _native.PLFEM_OK, name                    # the locator is still usable
        ex = _excess(out, em.project(vals, False, xf, yf), em.tolerance(vals, False, xf, yf))
        assert ex <= 1.0, name
        out[...] = np.nan
