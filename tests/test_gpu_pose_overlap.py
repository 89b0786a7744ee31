"""Posed overlaps on the GPU (k_field_overlap_posed through mode_overlap_poses, splice_map and taper_transfer): seeded
random DOF records on two small meshes against the NumPy emulation (tests/pose_overlap_emulation.py), against the merged
kernel on a mesh moved by the pose on the host, against a closed form; bit-identical results wherever a pose stands in
its table; the argument errors of the C ABI; and a scalar C1 solve spliced onto itself and run through a taper."""
import ctypes

import numpy as np
import pytest

from fields_emulation import Emulation
from pose_overlap_emulation import (COVERING, HALF_OUT, IDENTITY, closed_form, moved_mesh, moved_records, posed_overlap,
                                    quadratic_records, records, small_meshes, vals)
from pl_fem_vectoriel_amd import (MCFGeometry, ModeFields, _native, generate_mesh, mode_overlap, mode_overlap_poses, pose_table,
                                  splice_map, splice_quantities_from_overlaps, taper_transfer)
from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver

pytestmark = pytest.mark.gpu

PAIRS = ((1, 65), (33, 70), (32, 33))
KMAX = 70
POSES = (IDENTITY, COVERING, HALF_OUT)
QUARTER = (0.05, 0.1, 0.0, 1.0, 0.9)                     # an exact quarter turn


POSED_TOL = 1e-12       # posed overlaps against the emulation, of the largest reference entry


def discs_in_b():
    """Core discs inside mesh B ([-0.5, 0.5]^2) (no PML: only the real permittivity is read)."""
    g = MCFGeometry(7, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55, use_complex_pml=False)
    g.positions = g.core_positions = np.array([[-0.2, -0.15], [0.22, 0.1], [0.0, 0.3]])
    g.core_radii = np.array([0.17, 0.12, 0.1])
    g.n_cores = 3
    return g


def rel(a, ref):
    return np.abs(a - ref).max() / np.abs(ref).max()


@pytest.fixture(scope="module")
def pair(gpu_device, built_library):
    mesh_a, mesh_b = small_meshes()
    S = type("Pair", (), {})()
    S.mesh_a, S.mesh_b = mesh_a, mesh_b
    S.em_a, S.em_b = Emulation(mesh_a.p, mesh_a.t), Emulation(mesh_b.p, mesh_b.t)
    S.fa, S.fb = ModeFields(mesh_a, device=gpu_device), ModeFields(mesh_b, device=gpu_device)
    # several 64-point tiles and a partial last one, on both meshes
    assert 6 * S.fa.ne == 300 and 6 * S.fb.ne == 192 and S.em_b.quadrature()[0].shape[1] == 192
    assert 300 % 64 != 0 and 300 > 64 and 192 > 64
    rng = np.random.default_rng(31)
    S.modes = {kind: (records(rng, kind, S.fa.nsolve if kind == "vectorial" else S.fa.N, KMAX),
                      records(rng, kind, S.fb.nsolve if kind == "vectorial" else S.fb.N, KMAX))
               for kind in ("vectorial", "scalar")}
    S.weights = {"none": None, "discs": discs_in_b()}
    S.table = np.array(POSES)
    # the references, computed once: the emulation per (kind, weight, pose) on all KMAX x KMAX modes
    S.ref, S.outside = {}, {}
    for kind, (ra, rb) in S.modes.items():
        for wname, w in S.weights.items():
            for ip, pose in enumerate(POSES):
                O, elem = posed_overlap(S.em_a, vals(ra), S.em_b, vals(rb), kind == "vectorial", pose, weight=w)
                S.ref[kind, wname, ip] = O
                S.outside[ip] = float(np.mean(elem < 0))
    S.moved = {pose: ModeFields(moved_mesh(mesh_a, pose), device=gpu_device) for pose in POSES[1:] + (QUARTER,)}
    yield S
    for mf in [S.fa, S.fb] + list(S.moved.values()):
        mf.close()
    import torch
    torch.cuda.empty_cache()


def test_the_poses_exercise_the_outside_rule(pair):
    assert pair.outside[0] == 0.0 and pair.outside[1] == 0.0          # identity and covering pose: A covers B
    assert 0.25 <= pair.outside[2] <= 0.75, pair.outside[2]
    core = pair.em_b.quadrature(pair.weights["discs"])[1] != pair.em_b.quadrature()[1]
    assert 0.1 <= core.mean() <= 0.9                                    # the discs hold a real share of B's points


@pytest.mark.parametrize("wname", ["none", "discs"])
@pytest.mark.parametrize("kind", ["vectorial", "scalar"])
def test_posed_overlap_matches_emulation(pair, kind, wname):
    ra, rb = pair.modes[kind]
    w = pair.weights[wname]
    for ka, kb in PAIRS:
        O = mode_overlap_poses(ra[:ka], pair.fa, rb[KMAX - kb:], pair.fb, pair.table, weight=w)
        assert O.shape == (3, ka, kb)
        for ip in range(3):
            ref = pair.ref[kind, wname, ip][:ka, KMAX - kb:]
            err = rel(O[ip], ref)
            print(kind, wname, ka, kb, ip, f"{err:.2e}")
            assert err <= POSED_TOL, (kind, wname, ka, kb, ip, err)


@pytest.mark.parametrize("wname", ["none", "discs"])
@pytest.mark.parametrize("kind", ["vectorial", "scalar"])
def test_posed_overlap_matches_the_merged_kernel_on_a_moved_mesh(pair, kind, wname):
    ra, rb = pair.modes[kind]
    w = pair.weights[wname]
    for ka, kb in PAIRS:
        A, B = ra[:ka], rb[KMAX - kb:]
        O = mode_overlap_poses(A, pair.fa, B, pair.fb, pair.table, weight=w)
        for ip, pose in enumerate(POSES):
            if ip == 0:
                err = rel(O[0], mode_overlap(A, pair.fa, B, pair.fb, weight=w))
                assert err <= 1e-13, (kind, wname, ka, kb, err)
            else:
                err = rel(O[ip], mode_overlap(moved_records(A, pose), pair.moved[pose], B, pair.fb, weight=w))
                assert err <= 1e-12, (kind, wname, ka, kb, ip, err)
            print(kind, wname, ka, kb, ip, f"{err:.2e}")


def test_exact_quarter_turn_of_a_vectorial_record(pair):
    ra, rb = pair.modes["vectorial"]
    A, B = ra[:33], rb[:5]
    O = mode_overlap_poses(A, pair.fa, B, pair.fb, [QUARTER])
    ref = mode_overlap(moved_records(A, QUARTER), pair.moved[QUARTER], B, pair.fb)
    err = rel(O[0], ref)
    print(f"quarter turn {err:.2e}")
    assert err <= 1e-12, err
    # the turn matters: without it the result is another matrix
    assert rel(mode_overlap(A, pair.moved[QUARTER], B, pair.fb), ref) > 1e-3


def test_closed_form_of_quadratics(pair):
    rng = np.random.default_rng(32)
    Ca, Cb = rng.standard_normal((KMAX, 6)), rng.standard_normal((33, 6))
    O = mode_overlap_poses(quadratic_records(pair.em_a, Ca), pair.fa, quadratic_records(pair.em_b, Cb), pair.fb, [COVERING, IDENTITY])
    for ip, pose in enumerate((COVERING, IDENTITY)):
        ref = closed_form(Ca, Cb, pose)
        err = rel(O[ip], ref)
        print(f"closed form {pose}: {err:.2e}")
        assert err <= 1e-12, (pose, err)


def test_normalize(pair):
    ra, rb = pair.modes["scalar"]
    A, B = ra[:3], rb[:4]
    O = mode_overlap_poses(A, pair.fa, B, pair.fb, pair.table[:2])
    daa, dbb = np.diag(mode_overlap(A, pair.fa, A, pair.fa)), np.diag(mode_overlap(B, pair.fb, B, pair.fb))
    ref = O * O / (pair.table[:2, 4, None, None] ** 2 * daa[None, :, None] * dbb[None, None, :])
    assert np.array_equal(mode_overlap_poses(A, pair.fa, B, pair.fb, pair.table[:2], normalize=True), ref)


def batch_of_the_header(ka, kb, nposes, tiles_b):
    """The batch formula of include/plfem.h (plfem_field_overlap_posed)."""
    pairs = ((ka + 31) // 32) * ((kb + 31) // 32)
    slices = min(128, tiles_b)
    return max(1, min(nposes, 4096, ((512 << 20) - 768) // (8 * (ka * kb + 1024 * pairs * slices + 5))))


@pytest.mark.parametrize("kind", ["vectorial", "scalar"])
def test_a_pose_has_the_same_bits_wherever_it_stands(pair, kind):
    ra, rb = pair.modes[kind]
    w = pair.weights["discs"]
    A, B = ra[:33], rb[:35]
    pose = np.array([COVERING])
    alone = mode_overlap_poses(A, pair.fa, B, pair.fb, pose, weight=w)
    assert np.array_equal(alone, mode_overlap_poses(A, pair.fa, B, pair.fb, pose, weight=w))          # a repeat
    other = np.array([HALF_OUT, (0.3, 0.1, np.cos(1.0), np.sin(1.0), 0.7)])
    first = mode_overlap_poses(A, pair.fa, B, pair.fb, np.vstack([pose, other]), weight=w)
    last = mode_overlap_poses(A, pair.fa, B, pair.fb, np.vstack([other, pose]), weight=w)
    assert np.array_equal(first[0], alone[0]) and np.array_equal(last[2], alone[0])
    assert np.array_equal(first[1:], last[:2])
    # a table longer than one internal batch: small k, the pose on both sides of the batch boundary
    A, B = ra[:2], rb[:3]
    tiles_b = (6 * pair.fb.ne + 63) // 64
    T = 4096 + 2
    batch = batch_of_the_header(2, 3, T, tiles_b)
    assert batch + 2 == T                                              # the boundary is crossed
    alone = mode_overlap_poses(A, pair.fa, B, pair.fb, pose, weight=w)
    rng = np.random.default_rng(33)
    ang = rng.uniform(0, 2 * np.pi, T)
    table = pose_table(rng.uniform(-1, 1, T), rng.uniform(-1, 1, T), ang, rng.uniform(0.5, 1.5, T))
    at = (0, 1000, batch - 1, batch, T - 1)
    table[list(at)] = pose[0]
    long = mode_overlap_poses(A, pair.fa, B, pair.fb, table, weight=w)
    for i in at:
        assert np.array_equal(long[i], alone[0]), i
    for i in (7, batch - 2, T - 2):                                     # and the others are their own poses' results
        assert np.array_equal(long[i], mode_overlap_poses(A, pair.fa, B, pair.fb, table[i:i + 1], weight=w)[0]), i


def _abi_call(pair, work_fill=None, **kw):
    """plfem_field_overlap_posed on three scalar modes per side and two poses, arguments overridden by ``kw``."""
    import torch
    fa, fb = pair.fa, pair.fb
    fa._ensure_locator()
    fb._ensure_locator()
    lib = fa._lib
    ra, rb = pair.modes["scalar"]
    sa, _ = fa._stage(vals(ra[:3]))
    sb, _ = fb._stage(vals(rb[:3]))
    cores = np.zeros((65, 3))
    cores[:, 2] = 0.01
    poses = kw.pop("poses", np.array([IDENTITY, COVERING]))
    poses_ptr = None if poses is None else poses.ctypes.data_as(ctypes.c_void_p)
    need = ctypes.c_int64(0)
    assert lib.plfem_overlap_posed_work_bytes(fb._loc, 3, 3, 2, ctypes.byref(need)) == _native.PLFEM_OK
    work = torch.empty(int(need.value) + 256, dtype=torch.uint8, device=fa.tdev)
    if work_fill is not None:
        work.fill_(work_fill)
    aligned = (work.data_ptr() + 255) & ~255
    out = np.zeros((2, 3, 3))
    a = dict(loc_a=fa._loc, ma=ctypes.c_void_p(sa.data_ptr()), ka=3, loc_b=fb._loc, mb=ctypes.c_void_p(sb.data_ptr()), kb=3, ncomp=1,
             cores=cores.ctypes.data_as(ctypes.c_void_p), ncore=3, nposes=2, poses=poses_ptr,
             work=ctypes.c_void_p(aligned), work_bytes=int(need.value), out=out.ctypes.data_as(ctypes.c_void_p))
    a.update(kw)
    torch.cuda.synchronize()
    rc = lib.plfem_field_overlap_posed(a["loc_a"], a["ma"], a["ka"], 0, a["loc_b"], a["mb"], a["kb"], 0, a["ncomp"], a["cores"],
                                       a["ncore"], 2.0, 1.0, a["nposes"], a["poses"], a["work"], ctypes.c_int64(a["work_bytes"]),
                                       a["out"])
    torch.cuda.synchronize()
    return rc, out, lib.plfem_locator_last_error(fa._loc).decode()


def test_work_buffer_contents_change_nothing(pair):
    rc, ref, _ = _abi_call(pair, work_fill=0)
    assert rc == _native.PLFEM_OK and np.abs(ref).max() > 0
    rc, out, _ = _abi_call(pair, work_fill=0xFF)                       # NaN bytes
    assert rc == _native.PLFEM_OK and np.array_equal(out, ref)


def test_argument_errors_of_the_c_abi(pair):
    def pose(**kw):
        p = np.array([IDENTITY, COVERING])
        for j, v in kw.items():
            p[1, int(j[1:])] = v
        return p

    bad = {"nposes 0": dict(nposes=0), "nposes -1": dict(nposes=-1), "ka 0": dict(ka=0), "kb 0": dict(kb=0), "ncomp 0": dict(ncomp=0),
           "ncomp 3": dict(ncomp=3), "65 cores": dict(ncore=65), "null modes a": dict(ma=None), "null modes b": dict(mb=None),
           "null poses": dict(poses=None), "null work": dict(work=None), "null out": dict(out=None),
           "null cores": dict(cores=None), "null loc b": dict(loc_b=None), "short work": dict(short=True),
           "nan tx": dict(poses=pose(c0=np.nan)), "inf ty": dict(poses=pose(c1=np.inf)), "nan c": dict(poses=pose(c2=np.nan)),
           "nan m": dict(poses=pose(c4=np.nan)), "m 0": dict(poses=pose(c4=0.0)), "m < 0": dict(poses=pose(c4=-1.0)),
           "no rotation": dict(poses=pose(c2=1.0, c3=1e-5))}
    for name, kw in bad.items():
        if kw.pop("short", False):
            need = ctypes.c_int64(0)
            pair.fa._lib.plfem_overlap_posed_work_bytes(pair.fb._loc, 3, 3, 2, ctypes.byref(need))
            rc, out, msg = _abi_call(pair, work_bytes=int(need.value) - 1)
        else:
            rc, out, msg = _abi_call(pair, **kw)
        assert rc == _native.PLFEM_EINVAL, (name, rc)
        assert msg and "plfem_field_overlap_posed" in msg, (name, msg)
        assert (out == 0).all(), name
    need = ctypes.c_int64(0)
    lib = pair.fa._lib
    for args in ((None, 3, 3, 2), (pair.fb._loc, 0, 3, 2), (pair.fb._loc, 3, 0, 2), (pair.fb._loc, 3, 3, 0), (pair.fb._loc, 520, 520, 1)):
        assert lib.plfem_overlap_posed_work_bytes(*args, ctypes.byref(need)) == _native.PLFEM_EINVAL, args
    assert lib.plfem_overlap_posed_work_bytes(pair.fb._loc, 3, 3, 2, None) == _native.PLFEM_EINVAL
    for ka, kb, n in ((1, 1, 1), (70, 70, 1681), (512, 512, 100000), (512, 1, 2 ** 31 - 1)):
        assert lib.plfem_overlap_posed_work_bytes(pair.fb._loc, ka, kb, n, ctypes.byref(need)) == _native.PLFEM_OK
        assert 0 < need.value <= 512 << 20, (ka, kb, n, need.value)


# -- physics: one scalar C1 solve ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1(c1_geometry, gpu_device, built_library):
    mesh = generate_mesh(c1_geometry, 0.5, 0)
    sol = ScalarHelmholtzSolver(c1_geometry, device=gpu_device, eig_tol=1e-10)
    modes = sol.solve(mesh, n_modes_target=7)
    narrow = MCFGeometry(7, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55 / 0.9)       # the section scaled by 0.9
    sol2 = ScalarHelmholtzSolver(narrow, device=gpu_device, eig_tol=1e-10)
    modes2 = sol2.solve(mesh, n_modes_target=7)
    mf = ModeFields(mesh, device=gpu_device)
    yield {"mesh": mesh, "modes": modes, "modes2": modes2, "mf": mf, "k0": c1_geometry.k0}
    mf.close()
    sol.clear_cache()
    sol2.clear_cache()


def test_splice_of_a_set_onto_itself(c1):
    modes, mf = c1["modes"], c1["mf"]
    k = len(modes)
    assert k >= 2
    far = 3.0 * max(mf.bbox[1] - mf.bbox[0], mf.bbox[3] - mf.bbox[2])
    r = splice_map(modes, mf, modes, mf, [0.0, far], [0.0])
    assert r["transfer"].shape == (1, 2, k, k) and r["IL_dB"].shape == (1, 2)
    assert np.abs(r["transfer"][0, 0] - np.eye(k)).max() <= 1e-10
    assert abs(r["IL_dB"][0, 0]) <= 1e-10 and abs(r["MDL_dB"][0, 0]) <= 1e-10
    assert (r["overlap"][0, 1] == 0).all() and (r["transfer"][0, 1] == 0).all() and np.isinf(r["IL_dB"][0, 1])
    # a small offset loses power
    r = splice_map(modes, mf, modes, mf, [0.5], [0.25])
    assert 0 < r["IL_dB"][0, 0] < 3 and r["singular_values"].max() <= 1.01


def test_taper_of_equal_sections_is_the_diagonal_of_phases(c1):
    modes, mf, k0 = c1["modes"], c1["mf"], c1["k0"]
    L = (100.0, 250.0, 50.0)
    r = taper_transfer([modes] * 3, mf, (1.0, 1.0, 1.0), L, k0)
    beta = k0 * np.array([m["n_eff"] for m in modes])
    assert np.abs(r["transfer"] - np.diag(np.exp(-1j * beta * sum(L)))).max() <= 1e-10
    assert abs(r["IL_dB"]) <= 1e-10 and np.abs(r["transmitted"] - 1).max() <= 1e-10


def test_taper_interface_is_the_normalised_posed_overlap(c1):
    modes, modes2, mf, k0 = c1["modes"], c1["modes2"], c1["mf"], c1["k0"]
    assert len(modes2) >= 1
    r = taper_transfer([modes, modes2], mf, (1.0, 0.9), (100.0, 100.0), k0)
    m = 1.0 / 0.9
    O = mode_overlap_poses(modes, mf, modes2, mf, pose_table(scale=m))[0]
    q = splice_quantities_from_overlaps(O, mode_overlap(modes, mf, modes, mf), mode_overlap(modes2, mf, modes2, mf), m)
    T = r["interfaces"][0]
    assert T.shape == (len(modes2), len(modes))
    assert np.abs(T - q["transfer"]).max() <= 1e-12 * np.abs(q["transfer"]).max()
    sv = np.linalg.svd(T, compute_uv=False)
    assert 0.5 < sv.max() <= 1.01                                       # a projection, and most of the light gets through
    print("interface singular values", sv, "IL", r["IL_dB"], "MDL", r["MDL_dB"])
