"""Posed flux overlaps on the GPU (k_flux_overlap_posed through flux_overlap_poses, splice_power_map and
taper_transfer_vectorial): seeded random interior DOF records on the two small meshes of section 22 against the NumPy
emulation (tests/flux_overlap_emulation.py), against ``flux_grams`` at the identity pose of a set on itself, against
``sample_e`` contracted on the host, against the closed forms of quadratic fields through the C ABI; bit-identical results
wherever a pose stands in its table, whatever the work buffer held and however the modes are ordered; every argument error
of the C entry with the text recorded in tests/golden/flux_overlap_call_errors.json; and one small vectorial solve.
``PYTHONPATH=. python tests/test_gpu_flux_overlap.py [file]`` writes the record anew from the built library (on a GPU)."""
import ctypes
import json
import os

import numpy as np
import pytest

import power_cases
import topology_cases as tc
from flux_overlap_emulation import (NAMES, OUTSIDE, centred_profile, ka_closed_form, posed_flux, profiled, rim_disc_geometry,
                                    uniform_geometry, wide_profile)
from pose_overlap_emulation import COVERING, IDENTITY, rotate, small_meshes, to_a_frame
from power_emulation import PowerEmulation

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flux_overlap_call_errors.json")
PAIRS = ((1, 65), (33, 70), (32, 33))
KMAX = 70
POSES = (IDENTITY, COVERING, OUTSIDE)
MATERIALS = ("discs/discs", "profile/profile", "discs/profile", "profile/discs")      # all four kernel instances
EMU_TOL = 1e-12          # of each output's largest entry
SENTINEL = -7.0
NAN, INF = float("nan"), float("inf")
LAYER = [0.1, 0.1, 0.0, 0.2, 2.2, 2.1, 1.0, 0.0]        # (x, y, r_in, r_out, eps_in, eps_out, g, -)

SIDE = "loc{0} modes{0} k{0} indexed{0} cores{0} ncore{0} eps_core{0} eps_clad{0} layers{0} nlayer{0} eps_bg{0} use_profile{0}"
ORDER = (SIDE.format("_a") + " " + SIDE.format("_b") + " nposes poses work nbytes out").split()


def rel(a, ref):
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def raw(v):
    return v.ctypes.data_as(ctypes.c_void_p) if isinstance(v, np.ndarray) else v


def geometries(em_b):
    """{material: (geometry of A, geometry of B)}; the first disc of B has its rim through a quadrature point of B."""
    discs_b, rim_point = rim_disc_geometry(em_b)
    discs_a = power_cases.discs([[0.3, -0.2], [-0.6, 0.5], [0.1, 0.1]], [0.45, 0.3, 0.12], n_core=1.535, n_clad=1.0)
    prof_a, prof_b = profiled(wide_profile(), discs_a), profiled(centred_profile(), discs_b)
    return {"discs/discs": (discs_a, discs_b), "profile/profile": (prof_a, prof_b), "discs/profile": (discs_a, prof_b),
            "profile/discs": (prof_a, discs_b)}, rim_point


@pytest.fixture(scope="module")
def pair(gpu_device, built_library):
    from pl_fem_vectoriel_amd import ModeFields
    mesh_a, mesh_b = small_meshes()
    S = type("Pair", (), {})()
    S.mesh_a, S.mesh_b = mesh_a, mesh_b
    S.em_a, S.em_b = PowerEmulation(mesh_a.p, mesh_a.t), PowerEmulation(mesh_b.p, mesh_b.t)
    S.fa, S.fb = ModeFields(mesh_a, device=gpu_device), ModeFields(mesh_b, device=gpu_device)
    # several 32-point tiles on B; a partial last tile is what the 300 points of A give when A stands on B's side
    assert 6 * S.fa.ne == 300 and 6 * S.fb.ne == 192 and 300 % 32 != 0
    rng = np.random.default_rng(51)
    S.ra, S.rb = power_cases.records(rng, S.fa.nsolve, KMAX), power_cases.records(rng, S.fb.nsolve, KMAX)
    S.va, S.vb = power_cases.vals_of(S.ra), power_cases.vals_of(S.rb)
    S.geoms, S.rim_point = geometries(S.em_b)
    S.table = np.array(POSES)
    # the references, computed once: the emulation per (material, pose) on all KMAX x KMAX modes
    S.ref, S.elem = {}, {}
    for mname, (ga, gb) in S.geoms.items():
        for ip, pose in enumerate(POSES):
            S.ref[mname, ip], S.elem[ip] = posed_flux(S.em_a, S.va, ga, S.em_b, S.vb, gb, True, pose)
    yield S
    S.fa.close()
    S.fb.close()
    import torch
    torch.cuda.empty_cache()


def test_the_poses_and_materials_exercise_every_rule(pair):
    assert (pair.elem[0] >= 0).all() and (pair.elem[1] >= 0).all()          # identity and covering pose: A covers B
    outside = float(np.mean(pair.elem[2] < 0))
    assert outside >= 1 / 3 and 1 - outside >= 1 / 3, outside
    ga, gb = pair.geoms["discs/discs"]
    qx = pair.em_b.basis.qx.reshape(2, -1)
    core = pair.em_b.region_mask(gb).reshape(-1)
    assert 0.1 <= core.mean() <= 0.9 and core[pair.rim_point]                 # the rim point counts as core
    X, Y = qx[:, pair.rim_point]
    cx, cy = gb.positions[0]
    assert (X - cx) ** 2 + (Y - cy) ** 2 == gb.core_radii[0] ** 2             # and stands exactly on the rim


@pytest.mark.parametrize("mname", MATERIALS)
def test_posed_flux_matches_emulation(pair, mname):
    from pl_fem_vectoriel_amd import flux_overlap_poses
    ga, gb = pair.geoms[mname]
    for ka, kb in PAIRS:
        G = flux_overlap_poses(pair.ra[:ka], pair.fa, ga, pair.rb[KMAX - kb:], pair.fb, gb, pair.table)
        for ip in range(3):
            for nm in NAMES:
                assert G[nm].shape == (3, ka, kb)
                ref = pair.ref[mname, ip][nm][:ka, KMAX - kb:]
                err = rel(G[nm][ip], ref)
                print(mname, ka, kb, ip, nm, f"{err:.2e}")
                assert err <= EMU_TOL, (mname, ka, kb, ip, nm, err)


@pytest.mark.parametrize("mname", ["discs/discs", "profile/profile"])
def test_identity_pose_of_a_set_on_itself_is_flux_grams(pair, mname):
    """The same locator twice: MA = MB = M_w, GA = G_w, GB = G_w^T, core + rest."""
    from pl_fem_vectoriel_amd import flux_overlap_poses
    g = pair.geoms[mname][1]
    for k in (1, 33, 70):
        modes = pair.rb[:k]
        G = flux_overlap_poses(modes, pair.fb, g, modes, pair.fb, g, [IDENTITY])
        F = pair.fb.flux_grams(modes, g)
        M, Gw = F["M_w_core"] + F["M_w_rest"], F["G_w_core"] + F["G_w_rest"]
        errs = {"MA": rel(G["MA"][0], M), "MB": rel(G["MB"][0], M), "GA": rel(G["GA"][0], Gw), "GB": rel(G["GB"][0], Gw.T)}
        print(mname, k, {nm: f"{e:.2e}" for nm, e in errs.items()})
        assert max(errs.values()) <= 1e-13, (mname, k, errs)


def test_a_profile_reaches_the_side_it_is_given_to(pair):
    """The same locator and modes on both sides at the identity pose, a profile on one side and discs on the other: with
    the profile on A, MA and GA carry 1 / eps of the profile and MB and GB that of the discs; with the sides exchanged the
    outputs exchange their roles, MA <-> MB^T and GA <-> GB^T.  A kernel instance that took the other side's material, or
    evaluated it at the other side's point, differs from that by what the profile differs from the discs."""
    from pl_fem_vectoriel_amd import flux_overlap_poses
    discs, prof = pair.geoms["discs/discs"][1], pair.geoms["profile/profile"][1]
    for k in (1, 33, 70):
        modes = pair.rb[:k]
        call = lambda ga, gb: {nm: v[0] for nm, v in flux_overlap_poses(modes, pair.fb, ga, modes, pair.fb, gb, [IDENTITY]).items()}
        PD, DP, DD = call(prof, discs), call(discs, prof), call(discs, discs)
        errs = {"MA": rel(PD["MA"], DP["MB"].T), "MB": rel(PD["MB"], DP["MA"].T), "GA": rel(PD["GA"], DP["GB"].T),
                "GB": rel(PD["GB"], DP["GA"].T)}
        moved = {"MA of profile/discs": rel(PD["MA"], DD["MA"]), "GA of profile/discs": rel(PD["GA"], DD["GA"]),
                 "MB of discs/profile": rel(DP["MB"], DD["MB"]), "GB of discs/profile": rel(DP["GB"], DD["GB"])}
        kept = {"MB of profile/discs": rel(PD["MB"], DD["MB"]), "GB of profile/discs": rel(PD["GB"], DD["GB"]),
                "MA of discs/profile": rel(DP["MA"], DD["MA"]), "GA of discs/profile": rel(DP["GA"], DD["GA"])}
        print(k, {nm: f"{e:.2e}" for nm, e in errs.items()}, {nm: f"{e:.2e}" for nm, e in moved.items()},
              {nm: f"{e:.2e}" for nm, e in kept.items()})
        assert max(errs.values()) <= 1e-13, (k, errs)
        assert min(moved.values()) > 1e-3, (k, moved)                  # the profile changes its own side's outputs
        assert max(kept.values()) <= 1e-13, (k, kept)                  # and leaves the discs' side as discs / discs has it


@pytest.mark.parametrize("mname", MATERIALS)
def test_x_ab_against_sampled_e(pair, mname):
    """A's E sampled at B's posed quadrature points (sample_e, in A's frame, with A's own beta and k0), turned, and
    contracted on the host with B's own H: X_ab = int (E_a' x H_b) . z = (beta_a MA + GA / beta_a) / k0_a."""
    from pl_fem_vectoriel_amd import flux_overlap_poses
    ga, gb = pair.geoms[mname]
    ka, kb = 33, 35
    A, B = pair.ra[:ka], pair.rb[:kb]
    beta, k0 = power_cases.betas_of(A), float(ga.k0)
    G = flux_overlap_poses(A, pair.fa, ga, B, pair.fb, gb, pair.table)
    qx = pair.em_b.basis.qx.reshape(2, -1)
    w = pair.em_b.basis.dx.reshape(-1)
    hB = pair.em_b.own_values(pair.vb[:, :kb], True)
    for ip, pose in enumerate(POSES):
        E = pair.fa.sample_e(A, to_a_frame(qx, pose), ga)
        assert np.array_equal(E["element"] >= 0, pair.elem[ip] >= 0)
        Et = rotate(np.stack([E["Ex"], E["Ey"]]), pose)
        ref = Et[0] @ (hB[1] * w[None]).T - Et[1] @ (hB[0] * w[None]).T
        X_ab = (beta[:, None] * G["MA"][ip] + G["GA"][ip] / beta[:, None]) / k0
        err = rel(X_ab, ref)
        print(mname, ip, f"{err:.2e}")
        assert err <= 1e-11, (mname, ip, err)


# -- the C ABI ---------------------------------------------------------------------------------------------------------
def abi_arguments(pair, va, vb, indexed, poses, ga, gb, work_fill=None):
    """(arguments by name in ORDER, out (T, 4, ka, kb), work tensor) of a plfem_flux_overlap_posed call on host values
    va / vb (2, k, n) with disc geometries ga / gb; everything the pointers refer to stays alive in the dict."""
    import torch
    from pl_fem_vectoriel_amd import _native
    fa, fb = pair.fa, pair.fb
    fa._ensure_locator()
    fb._ensure_locator()
    sa, sb = fa._stage(np.ascontiguousarray(va))[0], fb._stage(np.ascontiguousarray(vb))[0]
    ka, kb, T = va.shape[1], vb.shape[1], len(poses)
    need = ctypes.c_int64(0)
    assert fa._lib.plfem_flux_overlap_posed_work_bytes(fb._loc, ka, kb, T, ctypes.byref(need)) == _native.PLFEM_OK
    work = torch.empty(int(need.value) + 256, dtype=torch.uint8, device=fa.tdev)
    if work_fill is not None:
        work.fill_(work_fill)
    out = np.full((T, 4, ka, kb), SENTINEL)
    a = dict(nposes=T, poses=np.ascontiguousarray(np.asarray(poses, dtype=np.float64)), work=(work.data_ptr() + 255) & ~255,
             nbytes=int(need.value), out=out, _keep=(sa, sb, work))
    for s, f, st, k, g in (("_a", fa, sa, ka, ga), ("_b", fb, sb, kb, gb)):
        cores = np.ascontiguousarray(np.column_stack([np.asarray(g.positions, dtype=np.float64).reshape(-1, 2),
                                                      np.asarray(g.core_radii, dtype=np.float64).reshape(-1)]))
        a.update({"loc" + s: f._loc, "modes" + s: st.data_ptr(), "k" + s: k, "indexed" + s: indexed, "cores" + s: cores,
                  "ncore" + s: cores.shape[0], "eps_core" + s: float(g.n_core) ** 2, "eps_clad" + s: float(g.n_clad) ** 2,
                  "layers" + s: np.array([LAYER]), "nlayer" + s: 1, "eps_bg" + s: 2.1, "use_profile" + s: 0})
    return a, out, work


def invoke(pair, a):
    import torch
    torch.cuda.synchronize()
    rc = pair.fa._lib.plfem_flux_overlap_posed(*[raw(a[nm]) for nm in ORDER])
    torch.cuda.synchronize()
    return rc


def test_closed_form_of_quadratic_fields_through_the_c_abi(pair):
    from pl_fem_vectoriel_amd import _native
    g = uniform_geometry()
    va = power_cases.ka_all_dof_vectors(pair.em_a.basis.doflocs)
    vb = power_cases.ka_all_dof_vectors(pair.em_b.basis.doflocs)
    a, out, _ = abi_arguments(pair, va, vb, 0, [COVERING, IDENTITY], g, g)
    assert invoke(pair, a) == _native.PLFEM_OK
    for ip, pose in enumerate((COVERING, IDENTITY)):
        ref = ka_closed_form(pose)
        for i, nm in enumerate(NAMES):
            err = rel(out[ip, i], ref[nm])
            print(f"closed form {nm} pose {ip}: {err:.2e}")
            assert err <= 1e-12, (nm, pose, err)


def test_work_buffer_contents_change_nothing(pair):
    from pl_fem_vectoriel_amd import _native
    ga, gb = pair.geoms["discs/discs"]
    outs = []
    for fill in (0, 0xFF):                                              # zeros, then NaN bytes
        a, out, _ = abi_arguments(pair, pair.va[:, :33], pair.vb[:, :35], 1, POSES, ga, gb, work_fill=fill)
        assert invoke(pair, a) == _native.PLFEM_OK
        outs.append(out)
    assert np.abs(outs[0]).max() > 0 and np.all(np.isfinite(outs[0])) and np.array_equal(outs[0], outs[1])
    for ip in range(3):
        for i, nm in enumerate(NAMES):
            assert rel(outs[0][ip, i], pair.ref["discs/discs", ip][nm][:33, :35]) <= EMU_TOL


def batch_of_the_header(ka, kb, nposes, tiles_b):
    """The batch formula of include/plfem.h (plfem_flux_overlap_posed)."""
    pairs = ((ka + 31) // 32) * ((kb + 31) // 32)
    slices = min(128, tiles_b)
    return max(1, min(nposes, 4096, ((512 << 20) - 768) // (8 * (4 * ka * kb + 4096 * pairs * slices + 5))))


def test_the_sizer_against_the_layout_of_the_header(pair):
    from pl_fem_vectoriel_amd import _native
    pair.fb._ensure_locator()
    lib, loc = pair.fb._lib, pair.fb._loc
    tiles_b = (6 * pair.fb.ne + 31) // 32
    up = lambda n: (n + 255) & ~255
    need = ctypes.c_int64(0)
    for ka, kb, n in ((1, 1, 1), (3, 3, 2), (70, 70, 1681), (33, 65, 5000), (256, 256, 100000), (2048, 1, 2 ** 31 - 1)):
        assert lib.plfem_flux_overlap_posed_work_bytes(loc, ka, kb, n, ctypes.byref(need)) == _native.PLFEM_OK
        pairs, slices = ((ka + 31) // 32) * ((kb + 31) // 32), min(128, tiles_b)
        batch = batch_of_the_header(ka, kb, n, tiles_b)
        assert need.value == up(8 * batch * 4 * ka * kb) + up(8 * batch * 4 * pairs * slices * 1024) + up(8 * batch * 5), (ka, kb, n)
        assert 0 < need.value <= 512 << 20, (ka, kb, n, need.value)
    for args in ((None, 3, 3, 2), (loc, 0, 3, 2), (loc, 3, 0, 2), (loc, 3, 3, 0), (loc, 264, 264, 1)):
        assert lib.plfem_flux_overlap_posed_work_bytes(*args, ctypes.byref(need)) == _native.PLFEM_EINVAL, args
    assert lib.plfem_flux_overlap_posed_work_bytes(loc, 3, 3, 2, None) == _native.PLFEM_EINVAL


@pytest.mark.parametrize("mname", ["discs/discs", "discs/profile"])
def test_a_pose_has_the_same_bits_wherever_it_stands(pair, mname):
    from pl_fem_vectoriel_amd import flux_overlap_poses, pose_table
    ga, gb = pair.geoms[mname]
    A, B = pair.ra[:33], pair.rb[:35]
    pose = np.array([COVERING])

    def call(a, b, table):
        G = flux_overlap_poses(a, pair.fa, ga, b, pair.fb, gb, table)
        return np.stack([G[nm] for nm in NAMES], axis=1)                # (T, 4, ka, kb)

    alone = call(A, B, pose)
    assert np.array_equal(alone, call(A, B, pose))                      # a repeat
    other = np.array([OUTSIDE, (0.3, 0.1, np.cos(1.0), np.sin(1.0), 0.7)])
    first, last = call(A, B, np.vstack([pose, other])), call(A, B, np.vstack([other, pose]))
    assert np.array_equal(first[0], alone[0]) and np.array_equal(last[2], alone[0])
    assert np.array_equal(first[1:], last[:2])
    # a permutation of the modes of each side, across the chunk boundary
    rng = np.random.default_rng(52)
    pa, pb = rng.permutation(33), rng.permutation(35)
    perm = call([A[i] for i in pa], [B[j] for j in pb], pose)
    assert np.array_equal(perm[0], alone[0][:, pa][:, :, pb])
    if mname != "discs/discs":
        return
    # a table longer than one internal batch: small k, the pose on both sides of the batch boundary
    A, B = pair.ra[:2], pair.rb[:3]
    tiles_b = (6 * pair.fb.ne + 31) // 32
    batch = batch_of_the_header(2, 3, 4096, tiles_b)
    assert batch < 4096
    T = batch + 2                                                       # the boundary is crossed
    assert batch_of_the_header(2, 3, T, tiles_b) == batch
    alone = call(A, B, pose)
    ang = rng.uniform(0, 2 * np.pi, T)
    table = pose_table(rng.uniform(-1, 1, T), rng.uniform(-1, 1, T), ang, rng.uniform(0.5, 1.5, T))
    at = (0, 1000, batch - 1, batch, T - 1)
    table[list(at)] = pose[0]
    long = call(A, B, table)
    for i in at:
        assert np.array_equal(long[i], alone[0]), i
    for i in (7, batch - 2, T - 2):                                     # and the others are their own poses' results
        assert np.array_equal(long[i], call(A, B, table[i:i + 1])[0]), i


def error_cases(good):
    """[(label, {argument: value})] of the rejected calls in the documented check order; the last have two faults."""
    c = []
    add = lambda label, **kw: c.append((label, kw))

    def pose(**kw):
        p = np.array([IDENTITY, COVERING])
        for j, v in kw.items():
            p[1, int(j[1:])] = v
        return p

    def bad_layer(j, v):
        row = list(LAYER)
        row[j] = v
        return np.array([row])

    add("loc_b=null", loc_b=None)
    add("ka=0", k_a=0)
    add("kb=-1", k_b=-1)
    add("nposes=0", nposes=0)
    add("nposes=-1", nposes=-1)
    add("65 chunk pairs", k_a=2049, k_b=33)
    for s in ("_a", "_b"):
        add(f"ncore{s}=65", **{"ncore" + s: 65})
        add(f"ncore{s}=-1", **{"ncore" + s: -1})
    for p in ("modes_a", "modes_b", "poses", "work", "out", "cores_a", "cores_b"):
        add(f"{p}=null", **{p: None})
    for s in ("_a", "_b"):
        prof = {"use_profile" + s: 1}
        add(f"profile{s}: nlayer=-1", **prof, **{"nlayer" + s: -1})
        add(f"profile{s}: nlayer=65", **prof, **{"nlayer" + s: 65})
        add(f"profile{s}: layers=null", **prof, **{"layers" + s: None})
        add(f"profile{s}: eps_bg=nan", **prof, **{"eps_bg" + s: NAN})
        add(f"profile{s}: eps_bg=0", **prof, **{"eps_bg" + s: 0.0})
        add(f"profile{s}: layer inf entry", **prof, **{"layers" + s: bad_layer(0, INF)})
        add(f"profile{s}: layer r_in<0", **prof, **{"layers" + s: bad_layer(2, -0.1)})
        add(f"profile{s}: layer r_out<=r_in", **prof, **{"layers" + s: bad_layer(3, 0.0)})
        add(f"profile{s}: layer eps<=0", **prof, **{"layers" + s: bad_layer(5, 0.0)})
        add(f"profile{s}: layer g<0", **prof, **{"layers" + s: bad_layer(6, -1.0)})
        add(f"discs{s}: eps_core=nan", **{"eps_core" + s: NAN})
        add(f"discs{s}: eps_core=-1", **{"eps_core" + s: -1.0})
        add(f"discs{s}: eps_clad=0", **{"eps_clad" + s: 0.0})
        add(f"discs{s}: eps_clad=inf", **{"eps_clad" + s: INF})
        add(f"discs{s}: a map on the locator", _map=s)
        add(f"profile{s}: a map on the locator", _map=s, **prof)
    add("one locator, two tables", _same=True, use_profile_a=1, use_profile_b=1, layers_b=bad_layer(4, 2.3))
    add("one locator, two table lengths", _same=True, use_profile_a=1, use_profile_b=1, nlayer_b=0)
    add("nan tx", poses=pose(c0=NAN))
    add("inf ty", poses=pose(c1=INF))
    add("nan c", poses=pose(c2=NAN))
    add("nan m", poses=pose(c4=NAN))
    add("m=0", poses=pose(c4=0.0))
    add("m<0", poses=pose(c4=-1.0))
    add("no rotation", poses=pose(c2=1.0, c3=1e-5))
    add("work one byte short", nbytes=good["nbytes"] - 1)
    add("work misaligned by 8", work=good["work"] + 8)
    # two faults: the earlier check speaks
    add("ka=0, ncore_a=65", k_a=0, ncore_a=65)
    add("ncore_b=65, modes_a=null", ncore_b=65, modes_a=None)
    add("out=null, discs_a: eps_core=nan", out=None, eps_core_a=NAN)
    add("discs_a: eps_clad=0, profile_b: eps_bg=nan", eps_clad_a=0.0, use_profile_b=1, eps_bg_b=NAN)
    add("profile_a: eps_bg=nan with bad discs", use_profile_a=1, eps_bg_a=NAN, eps_core_a=NAN)
    add("discs_b: eps_clad=0, nan m", eps_clad_b=0.0, poses=pose(c4=NAN))
    add("nan m, work one byte short", poses=pose(c4=NAN), nbytes=good["nbytes"] - 1)
    add("work one byte short and misaligned", nbytes=good["nbytes"] - 1, work=good["work"] + 8)
    return c


def observe(pair):
    """{case: text} of the library.  Asserts on the way that every case is rejected with PLFEM_EINVAL, and at the end that
    neither the host output nor the work buffer was written."""
    import torch
    from pl_fem_vectoriel_amd import _native
    ga, gb = pair.geoms["discs/discs"]
    good, out, work = abi_arguments(pair, pair.va[:, :3], pair.vb[:, :3], 1, [IDENTITY, COVERING], ga, gb)
    work.fill_(0x5A)
    lib = pair.fa._lib
    EINVAL, OK = _native.PLFEM_EINVAL, _native.PLFEM_OK
    a_map = np.full((2, 2), 2.0)
    # a second set of modes on B's mesh, for the calls with B's locator on both sides
    same = {"loc_a": good["loc_b"], "modes_a": good["modes_b"]}

    def set_map(loc, on):
        rc = (lib.plfem_locator_set_index_map(loc, raw(a_map), 2, 2, 0.0, 0.0, 1.0, 1.0) if on else
              lib.plfem_locator_set_index_map(loc, None, 0, 0, 0.0, 0.0, 0.0, 0.0))
        assert rc == OK

    errors = {}
    for label, kw in error_cases(good):
        kw = dict(kw)
        side, one = kw.pop("_map", None), kw.pop("_same", False)
        args = {**good, **(same if one else {}), **kw}
        err_loc = args["loc_a"]
        # a rejection with another text in between: the text read below is this call's, not the previous case's
        assert invoke(pair, {**good, **(same if one else {}), "nposes": 0 if label != "nposes=0" else -1}) == EINVAL
        if side:
            set_map(good["loc" + side], True)
        try:
            assert invoke(pair, args) == EINVAL, label
            text = lib.plfem_locator_last_error(err_loc).decode()
        finally:
            if side:
                set_map(good["loc" + side], False)
        assert label not in errors
        errors[label] = text
        assert text.startswith("plfem_flux_overlap_posed: ") and len(text) > len("plfem_flux_overlap_posed: "), (label, text)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert bool((work == 0x5A).all())
    # and the accepted call still runs
    assert invoke(pair, good) == OK and np.all(np.isfinite(out)) and np.abs(out).max() > 0
    return errors


def test_rejections_are_the_recorded_ones(pair):
    with open(GOLDEN) as f:
        recorded = json.load(f)
    got = observe(pair)
    assert got == recorded
    # the documented check order: a call with two faults speaks of the earlier one
    assert got["ka=0, ncore_a=65"] == got["ka=0"]
    assert got["ncore_b=65, modes_a=null"] == got["ncore_b=65"]
    assert got["out=null, discs_a: eps_core=nan"] == got["out=null"]
    assert got["discs_a: eps_clad=0, profile_b: eps_bg=nan"] == got["discs_a: eps_clad=0"]
    assert got["profile_a: eps_bg=nan with bad discs"] == got["profile_a: eps_bg=nan"]             # eps_core is not read
    assert got["discs_b: eps_clad=0, nan m"] == got["discs_b: eps_clad=0"]
    assert got["nan m, work one byte short"] == got["nan m"]
    assert got["work one byte short and misaligned"] == got["work one byte short"] != got["work misaligned by 8"]
    assert got["discs_a: a map on the locator"] != got["discs_b: a map on the locator"]            # each names its side
    print(len(got), "cases,", len(set(got.values())), "texts")


# -- physics: one small vectorial solve --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solved(gpu_device, built_library):
    from pl_fem_vectoriel_amd import MCFGeometry, ModeFields, generate_mesh
    from pl_fem_vectoriel_amd.solver_fem import TrueVectorialMaxwellSolver
    g = tc.two_core_geometry()
    mesh = generate_mesh(g, 0.5, 0)
    solver = TrueVectorialMaxwellSolver(g, device=gpu_device)
    modes = solver.solve_vectorial_modes(mesh, n_modes_target=4)
    assert len(modes) >= 2
    # the section scaled by 0.9: the same mesh at the wavelength divided by 0.9
    narrow = MCFGeometry(7, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55 / 0.9, use_complex_pml=False)
    narrow.positions = narrow.core_positions = g.positions
    narrow.core_radii, narrow.n_cores = g.core_radii, g.n_cores
    solver2 = TrueVectorialMaxwellSolver(narrow, device=gpu_device)
    modes2 = solver2.solve_vectorial_modes(mesh, n_modes_target=4)
    assert len(modes2) >= 1
    mf = ModeFields(mesh, device=gpu_device, solver=solver)
    yield {"g": g, "mesh": mesh, "modes": modes, "modes2": modes2, "mf": mf}
    mf.close()
    solver.clear_cache()
    solver2.clear_cache()


def test_power_splice_of_a_set_onto_itself_is_the_identity(solved):
    """|T| = I inside 1e-10 at zero offset.  The records of this solve are power-orthogonal to 5.4e-2 only (DESIGN.md section
    28), so the identity is that of the map's own normalisation: each set Loewdin-orthonormalised under its symmetrised
    cross powers.  With the modes taken as they are (``orthonormalize=False``) the diagonal is still 1 -- the self flux of a
    mode is twice its power -- and the off-diagonal entries are the records' power orthogonality, printed."""
    from pl_fem_vectoriel_amd import mode_power, splice_power_map
    g, modes, mf = solved["g"], solved["modes"], solved["mf"]
    k = len(modes)
    r = splice_power_map(modes, mf, g, modes, mf, g, [0.0], [0.0])
    T = r["transfer"][0, 0]
    assert T.shape == (k, k)
    print(f"|T| - I: {np.abs(np.abs(T) - np.eye(k)).max():.2e}, IL {r['IL_dB'][0, 0]:.2e} dB, MDL {r['MDL_dB'][0, 0]:.2e} dB")
    assert np.abs(np.abs(T) - np.eye(k)).max() <= 1e-10
    assert abs(r["IL_dB"][0, 0]) <= 1e-9 and abs(r["MDL_dB"][0, 0]) <= 1e-9
    raw = splice_power_map(modes, mf, g, modes, mf, g, [0.0], [0.0], orthonormalize=False)["transfer"][0, 0]
    q = mode_power(modes, mf, g)
    off = np.abs(raw - np.diag(np.diag(raw)))
    print(f"modes as they are: diagonal - 1 {np.abs(np.diag(raw) - 1).max():.2e}, largest off-diagonal entry {off.max():.2e}, "
          f"orthogonality.max() {q['orthogonality'].max():.2e}")
    assert np.abs(np.diag(raw) - 1).max() <= 1e-10
    assert np.abs(off - q["orthogonality"]).max() <= 1e-10               # the raw map of a set onto itself is that matrix
    assert np.array_equal(r["power_a"], q["power"]) and np.array_equal(r["cross_a"], q["cross_sym"])


def test_power_splice_with_an_offset_and_against_the_h_h_map(solved):
    from pl_fem_vectoriel_amd import splice_map, splice_power_map
    g, modes, mf = solved["g"], solved["modes"], solved["mf"]
    k = len(modes)
    r = splice_power_map(modes, mf, g, modes, mf, g, [0.0, 0.2], [0.0])
    assert r["transfer"].shape == (1, 2, k, k) and r["IL_dB"].shape == (1, 2)
    for nm in ("transfer", "power", "singular_values", "IL_dB", "MDL_dB"):
        assert np.all(np.isfinite(r[nm])), nm
    assert np.abs(r["transfer"][0, 0] - np.eye(k)).max() <= 1e-10
    assert 0 < r["IL_dB"][0, 1] < 6 and r["singular_values"][0, 1].max() <= 1.05      # a small offset loses power
    hh = splice_map(modes, mf, modes, mf, [0.0, 0.2], [0.0])
    print("IL_dB, E x H:", r["IL_dB"][0], " H.H:", hh["IL_dB"][0])       # printed, not asserted
    print("MDL_dB, E x H:", r["MDL_dB"][0], " H.H:", hh["MDL_dB"][0])


def test_vectorial_taper_over_two_scales(solved):
    from pl_fem_vectoriel_amd import taper_transfer_vectorial
    g, modes, modes2, mf = solved["g"], solved["modes"], solved["modes2"], solved["mf"]
    r = taper_transfer_vectorial([modes, modes2], mf, g, (1.0, 0.9), (100.0, 100.0), float(g.k0))
    assert r["transfer"].shape == (len(modes2), len(modes)) and r["interfaces"][0].shape == (len(modes2), len(modes))
    for nm in ("transfer", "power", "transmitted", "singular_values"):
        assert np.all(np.isfinite(r[nm])), nm
    assert np.isfinite(r["IL_dB"]) and np.all(np.isfinite(r["interface_IL_dB"]))
    # equal sections: every interface is the normalised cross flux of the set with itself, diagonal 1
    same = taper_transfer_vectorial([modes, modes], mf, g, (1.0, 1.0), (10.0, 10.0), float(g.k0))
    assert np.abs(np.diag(same["interfaces"][0]) - 1).max() <= 1e-10
    print("interface singular values", np.linalg.svd(r["interfaces"][0], compute_uv=False), "IL", r["IL_dB"], "MDL", r["MDL_dB"])


if __name__ == "__main__":
    import sys
    from pl_fem_vectoriel_amd import ModeFields
    ma, mb = small_meshes()
    P = type("Pair", (), {})()
    P.em_b = PowerEmulation(mb.p, mb.t)
    P.fa, P.fb = ModeFields(ma, device=0), ModeFields(mb, device=0)
    gen = np.random.default_rng(51)
    P.va = power_cases.vals_of(power_cases.records(gen, P.fa.nsolve, 3))
    P.vb = power_cases.vals_of(power_cases.records(gen, P.fb.nsolve, 3))
    P.geoms, _ = geometries(P.em_b)
    with open(GOLDEN if len(sys.argv) < 2 else sys.argv[1], "w") as f:
        json.dump(observe(P), f, indent=1, sort_keys=True)
        f.write("\n")
    P.fa.close()
    P.fb.close()
