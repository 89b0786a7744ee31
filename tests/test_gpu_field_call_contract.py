"""What the field entry points of the C ABI reject, and with which words: every rejection branch of the ten work-buffer
calls, of plfem_stage_modes and of plfem_sample_fields is driven once on a 72-element mesh, plus one call per entry point
with two faults at once (which check comes first), and the three sizers that need a locator return their recorded
bytes.  Every rejected call returns PLFEM_EINVAL, leaves the full text recorded in tests/golden/field_call_errors.json in
plfem_locator_last_error and writes none of its outputs.  Host validation rejects every call here before any launch.
``python tests/test_gpu_field_call_contract.py`` writes the record anew from the built library (on a GPU)."""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "field_call_errors.json")
K = 3
SENTINEL = -7.0
NAN, INF = float("nan"), float("inf")
LAYER = [0.5, 0.5, 0.0, 0.2, 2.2, 2.1, 1.0, 0.0]        # (x, y, r_in, r_out, eps_in, eps_out, g, -)

# argument order of each entry point (include/plfem.h)
HEAD = "L ncomp k modes indexed"
TAIL = "work nbytes out"
PAIR = "L modes_a ka indexed_a Lb modes_b kb indexed_b ncomp cores ncore eps_core eps_clad"
ORDER = {
    "plfem_stage_modes": "L ncomp k nrows src dst",
    "plfem_sample_fields": f"{HEAD} beta npts points out_dev elem",
    "plfem_field_overlap": f"{PAIR} {TAIL}",
    "plfem_field_overlap_posed": f"{PAIR} nposes poses {TAIL}",
    "plfem_mode_grams": f"{HEAD} cores ncore {TAIL}",
    "plfem_profile_grams": f"{HEAD} layers nlayer eps_bg {TAIL}",
    "plfem_mode_indicators": f"{HEAD} lam k0 alpha_p cores ncore eps_core eps_clad layers nlayer eps_bg {TAIL}",
    "plfem_core_grams": f"{HEAD} cores ncore {TAIL} count",
    "plfem_moment_grams": f"{HEAD} cores ncore origin {TAIL}",
    "plfem_mode_quartic": f"{HEAD} cores ncore w_core w_clad {TAIL}",
    "plfem_mode_project": f"{HEAD} la xfac lb yfac {TAIL}",
    "plfem_mode_project_sampled": f"{HEAD} nx ny x0 y0 dx dy nf frames {TAIL}",
}
# sizer and its arguments, as names of the call's arguments, of the entry points that take a work buffer
SIZER = {
    "plfem_field_overlap": ("plfem_overlap_work_bytes", "ka kb"),
    "plfem_field_overlap_posed": ("plfem_overlap_posed_work_bytes", "Lb ka kb nposes"),
    "plfem_mode_grams": ("plfem_gram_work_bytes", "ncomp k"),
    "plfem_profile_grams": ("plfem_profile_gram_work_bytes", "ncomp k"),
    "plfem_mode_indicators": ("plfem_indicator_work_bytes", "L ncomp k"),
    "plfem_core_grams": ("plfem_core_gram_work_bytes", "L ncomp k ncore"),
    "plfem_moment_grams": ("plfem_moment_gram_work_bytes", "ncomp k"),
    "plfem_mode_quartic": ("plfem_quartic_work_bytes", "ncomp k"),
    "plfem_mode_project": ("plfem_project_work_bytes", "ncomp k la lb"),
    "plfem_mode_project_sampled": ("plfem_project_sampled_work_bytes", "ncomp k nf"),
}
# the locator-bound sizers at a few shapes
LOCATOR_SIZES = {
    "plfem_overlap_posed_work_bytes": [(3, 3, 3), (33, 3, 1), (3, 64, 5000)],
    "plfem_core_gram_work_bytes": [(1, 3, 2), (2, 3, 2), (2, 33, 64)],
    "plfem_indicator_work_bytes": [(1, 3), (2, 3), (2, 33)],
}
# pointer arguments whose null is a rejection branch of its own (`beta` and an unused `cores` may be null)
POINTERS = {
    "plfem_stage_modes": "src dst",
    "plfem_sample_fields": "points elem modes out_dev",
    "plfem_field_overlap": "modes_a modes_b work out cores",
    "plfem_field_overlap_posed": "modes_a modes_b poses work out cores",
    "plfem_mode_grams": "modes work out cores",
    "plfem_profile_grams": "modes work out layers",
    "plfem_mode_indicators": "modes lam work out",
    "plfem_core_grams": "modes cores work out count",
    "plfem_moment_grams": "modes work out origin cores",
    "plfem_mode_quartic": "modes work out cores",
    "plfem_mode_project": "modes xfac yfac work out",
    "plfem_mode_project_sampled": "modes frames work out",
}


def _bad_layer(j, v):
    row = list(LAYER)
    row[j] = v
    return np.array([row])


def _bad_row(good, i, j, v):
    a = np.array(good, dtype=np.float64, copy=True)
    a[i, j] = v
    return a


def cases(name, good):
    """[(label, {argument: value})] of the rejected calls of one entry point; ``good`` is its accepted argument set.  The
    last case of each list has two faults."""
    c = []
    add = lambda label, **kw: c.append((label, kw))
    if "ncomp" in good:
        add("ncomp=0", ncomp=0)
        add("ncomp=3", ncomp=3)
    if "k" in good:
        add("k=-1", k=-1)
        if name not in ("plfem_stage_modes", "plfem_sample_fields"):
            add("k=0", k=0)
    if name in ("plfem_mode_quartic", "plfem_mode_project", "plfem_mode_project_sampled"):
        add("k=65", k=65)
    for p in POINTERS[name].split():
        add(f"{p}=null", **{p: None})
    if "ncore" in good and name != "plfem_mode_indicators":         # (its profile path, the accepted call here, reads no cores)
        add("ncore=65", ncore=65)
        if name in ("plfem_mode_grams", "plfem_moment_grams"):
            add("ncore=-1", ncore=-1)
    if name in SIZER:
        add("work one byte short", nbytes=good["nbytes"] - 1)
        add("work misaligned by 8", work=good["work"] + 8)
    if name == "plfem_stage_modes":
        add("nrows=-1", nrows=-1)
        add("ncomp=0, src=null", ncomp=0, src=None)
    if name == "plfem_sample_fields":
        add("npts=-1", npts=-1)
        add("ncomp=0, points=null", ncomp=0, points=None)
    if name in ("plfem_field_overlap", "plfem_field_overlap_posed"):
        add("Lb=null", Lb=None)
        add("ka=-1", ka=-1)
        add("kb=-1", kb=-1)
    if name == "plfem_field_overlap":
        add("Lb=null, ncomp=0", Lb=None, ncomp=0)
        add("ncomp=0, modes_a=null", ncomp=0, modes_a=None)
    if name == "plfem_field_overlap_posed":
        add("ka=0", ka=0)
        add("kb=0", kb=0)
        add("nposes=0", nposes=0)
        add("ka=kb=545: 324 chunk pairs", ka=545, kb=545)
        P = good["_poses"]
        add("pose: nan shift", poses=_bad_row(P, 1, 0, NAN))
        add("pose: m=0", poses=_bad_row(P, 2, 4, 0.0))
        add("pose: no rotation", poses=_bad_row(P, 0, 2, 0.5))
        add("ncomp=3, nposes=0", ncomp=3, nposes=0)
        add("ncore=65, pose: m=0", ncore=65, poses=_bad_row(P, 2, 4, 0.0))
    if name == "plfem_mode_grams":
        add("ncomp=0, ncore=65", ncomp=0, ncore=65)
        add("ncore=65, modes=null", ncore=65, modes=None)
    if name in ("plfem_profile_grams", "plfem_mode_indicators"):
        add("nlayer=-1", nlayer=-1)
        add("nlayer=65", nlayer=65)
        add("eps_bg=nan", eps_bg=NAN)
        add("eps_bg=0", eps_bg=0.0)
        add("layer: inf entry", layers=_bad_layer(0, INF))
        add("layer: r_in<0", layers=_bad_layer(2, -0.1))
        add("layer: r_out<=r_in", layers=_bad_layer(3, 0.0))
        add("layer: eps<=0", layers=_bad_layer(5, 0.0))
        add("layer: g<0", layers=_bad_layer(6, -1.0))
    if name == "plfem_profile_grams":
        add("nlayer=65, modes=null", nlayer=65, modes=None)
    if name == "plfem_mode_indicators":
        add("k0=nan", k0=NAN)
        add("alpha_p=inf", alpha_p=INF)
        add("lam: nan", lam=np.array([1.0, NAN, 1.0]))
        add("cores: ncore=65", nlayer=0, ncore=65)
        add("cores: ncore=-1", nlayer=0, ncore=-1)
        add("cores: cores=null", nlayer=0, cores=None)
        add("cores: eps_core=nan", nlayer=0, eps_core=NAN)
        add("cores: eps_clad=0", nlayer=0, eps_clad=0.0)
        add("cores: work one byte short", nlayer=0, nbytes=good["nbytes"] - 1)
        add("modes=null, k0=nan", modes=None, k0=NAN)
        add("k0=nan, nlayer=65", k0=NAN, nlayer=65)
    if name == "plfem_core_grams":
        add("ncore=0", ncore=0)
        add("k=0, ncore=0", k=0, ncore=0)
        add("ncore=65, modes=null", ncore=65, modes=None)
    if name == "plfem_moment_grams":
        add("origin: nan", origin=np.array([0.0, NAN]))
        add("ncore=65, origin: nan", ncore=65, origin=np.array([0.0, NAN]))
        add("modes=null, origin: nan", modes=None, origin=np.array([0.0, NAN]))
    if name == "plfem_mode_quartic":
        add("ncore=-1, cores=null is no weight: work one byte short", ncore=-1, cores=None, nbytes=good["nbytes"] - 1)
        add("k=65, ncore=65", k=65, ncore=65)
        add("ncore=65, modes=null", ncore=65, modes=None)
    if name == "plfem_mode_project":
        for a in ("la", "lb"):
            add(f"{a}=0", **{a: 0})
            add(f"{a}=4097", **{a: 4097})
        add("xfac: nan", xfac=_bad_row(good["_xfac"], 1, 2, NAN))
        add("xfac: s<0", xfac=_bad_row(good["_xfac"], 0, 1, -1.0))
        add("yfac: inf", yfac=_bad_row(good["_yfac"], 0, 0, INF))
        add("yfac: s<0", yfac=_bad_row(good["_yfac"], 1, 1, -1.0))
        add("la=0, modes=null", la=0, modes=None)
        add("modes=null, xfac: nan", modes=None, xfac=_bad_row(good["_xfac"], 1, 2, NAN))
    if name == "plfem_mode_project_sampled":
        for a, bad in (("nf", (0, 4097)), ("nx", (1, 8193)), ("ny", (1, 8193))):
            for v in bad:
                add(f"{a}={v}", **{a: v})
        add("dx=0", dx=0.0)
        add("dx=nan", dx=NAN)
        add("dy=-1", dy=-1.0)
        add("dy=inf", dy=INF)
        add("x0=inf", x0=INF)
        add("y0=nan", y0=NAN)
        add("dx=1e-310: 1 / dx overflows", dx=1e-310)
        add("nx=1, dx=0", nx=1, dx=0.0)
        add("dx=0, frames=null", dx=0.0, frames=None)
    if name == "plfem_field_overlap":
        add("ncore=-1, cores=null is no weight: work one byte short", ncore=-1, cores=None, nbytes=good["nbytes"] - 1)
        add("modes_b=null, ncore=65", modes_b=None, ncore=65)
    return c


def observe(mf):
    """{"sizes": {call: bytes}, "errors": {entry point: {case: text}}} of the library on ``mf``'s locator.  Asserts on the
    way that every case is rejected with PLFEM_EINVAL and writes no output."""
    import torch
    from pl_fem_vectoriel_amd import _native
    mf._ensure_locator()
    lib, L = mf._lib, mf._loc
    EINVAL = _native.PLFEM_EINVAL

    sizes = {}
    for sizer, shapes in LOCATOR_SIZES.items():
        for args in shapes:
            need = ctypes.c_int64(-7)
            assert getattr(lib, sizer)(L, *args, ctypes.byref(need)) == _native.PLFEM_OK
            sizes[f"{sizer}({', '.join(map(str, args))})"] = int(need.value)
            assert getattr(lib, sizer)(L, *args, None) == EINVAL and getattr(lib, sizer)(None, *args, ctypes.byref(need)) == EINVAL

    # device arrays: modes (ncomp, n, k) and everything a call would write on the device, the latter sentinel-filled
    n = mf.nsolve
    dev = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=mf.tdev)
    modes, src, frames, points = dev(2, n, K), dev(2, K, n), dev(4, 4, 2, 2), dev(2, 5)
    dst = torch.full((2, n, K), SENTINEL, dtype=torch.float64, device=mf.tdev)
    out_dev = torch.full((2, K, 5), SENTINEL, dtype=torch.float64, device=mf.tdev)
    elem = torch.full((5,), int(SENTINEL), dtype=torch.int32, device=mf.tdev)
    host = {"out": np.full(1 << 16, SENTINEL), "count": np.full(64, int(SENTINEL), dtype=np.int64)}
    cores = np.array([[0.3, 0.3, 0.1], [0.7, 0.7, 0.1]])
    poses = np.array([[0.0, 0.0, 1.0, 0.0, 1.0], [0.1, 0.0, 0.0, 1.0, 1.0], [0.0, 0.1, 1.0, 0.0, 2.0]])
    xfac = np.array([[0.0, 0.0, 0.0], [0.5, 1.0, 2.0]])
    yfac = np.array([[0.0, 0.0, 0.0], [0.5, 1.0, -2.0]])
    head = dict(L=L, ncomp=2, k=K, modes=modes.data_ptr(), indexed=1)
    pair = dict(L=L, modes_a=modes.data_ptr(), ka=K, indexed_a=1, Lb=L, modes_b=modes.data_ptr(), kb=K, indexed_b=1, ncomp=2,
                cores=cores, ncore=2, eps_core=2.2, eps_clad=2.1)
    weight = dict(cores=cores, ncore=2)
    good = {
        "plfem_stage_modes": dict(L=L, ncomp=2, k=K, nrows=n, src=src.data_ptr(), dst=dst.data_ptr()),
        "plfem_sample_fields": dict(head, beta=None, npts=5, points=points.data_ptr(), out_dev=out_dev.data_ptr(),
                                    elem=elem.data_ptr()),
        "plfem_field_overlap": pair,
        "plfem_field_overlap_posed": dict(pair, nposes=3, poses=poses, _poses=poses),
        "plfem_mode_grams": dict(head, **weight),
        "plfem_profile_grams": dict(head, layers=np.array([LAYER]), nlayer=1, eps_bg=2.1),
        "plfem_mode_indicators": dict(head, lam=np.ones(K), k0=4.0, alpha_p=1.0, **weight, eps_core=2.2, eps_clad=2.1,
                                      layers=np.array([LAYER]), nlayer=1, eps_bg=2.1),
        "plfem_core_grams": dict(head, **weight, count=host["count"]),
        "plfem_moment_grams": dict(head, **weight, origin=np.zeros(2)),
        "plfem_mode_quartic": dict(head, **weight, w_core=1.0, w_clad=1.0),
        "plfem_mode_project": dict(head, la=2, xfac=xfac, lb=2, yfac=yfac, _xfac=xfac, _yfac=yfac),
        "plfem_mode_project_sampled": dict(head, nx=4, ny=4, x0=0.0, y0=0.0, dx=0.25, dy=0.25, nf=2, frames=frames.data_ptr()),
    }

    def raw(v):
        return v.ctypes.data_as(ctypes.c_void_p) if isinstance(v, np.ndarray) else v

    def invoke(name, args):
        return getattr(lib, name)(*[raw(args[a]) for a in ORDER[name].split()])

    def last_error():
        return lib.plfem_locator_last_error(L).decode()

    keep = []                                                    # the work buffers stay alive until the end
    errors = {}
    for name in ORDER:
        g = good[name]
        if name in SIZER:
            sizer, names = SIZER[name]
            need = ctypes.c_int64(-7)
            assert getattr(lib, sizer)(*[g[a] for a in names.split()], ctypes.byref(need)) == _native.PLFEM_OK, name
            work = torch.empty(int(need.value) + 256, dtype=torch.uint8, device=mf.tdev)
            keep.append(work)
            g.update(work=(work.data_ptr() + 255) & ~255, nbytes=int(need.value), out=host["out"])
        # a rejection of another entry point in between: the text read below is this call's, not the previous case's
        other = "plfem_sample_fields" if name == "plfem_stage_modes" else "plfem_stage_modes"
        errors[name] = {}
        for label, kw in cases(name, g):
            assert invoke(other, dict(good[other], ncomp=0)) == EINVAL
            assert invoke(name, {**g, **kw}) == EINVAL, (name, label)
            assert label not in errors[name]
            errors[name][label] = last_error()
            assert errors[name][label].startswith(name + ": "), (name, label)
    torch.cuda.synchronize(mf.tdev)
    assert (host["out"] == SENTINEL).all() and (host["count"] == int(SENTINEL)).all()
    assert bool((dst == SENTINEL).all()) and bool((out_dev == SENTINEL).all()) and bool((elem == int(SENTINEL)).all())
    del keep
    return {"sizes": sizes, "errors": errors}


def test_rejections_and_locator_bound_sizes_are_the_recorded_ones(gpu_device, built_library):
    from pl_fem_vectoriel_amd import ModeFields
    from pl_fem_vectoriel_amd.mesh import unit_square_mesh
    with open(GOLDEN) as f:
        recorded = json.load(f)
    mf = ModeFields(unit_square_mesh(6), device=gpu_device)
    try:
        assert mf.ne == 72
        got = observe(mf)
    finally:
        mf.close()
    assert got["sizes"] == recorded["sizes"]
    assert set(got["errors"]) == set(recorded["errors"]) and len(got["errors"]) == 12
    for name, texts in got["errors"].items():
        assert texts == recorded["errors"][name], name
    # every distinct message of an entry point is reached (the interior-DOF check needs an analysis without interior DOFs)
    print({name: len(set(texts.values())) for name, texts in got["errors"].items()})


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pl_fem_vectoriel_amd import ModeFields
    from pl_fem_vectoriel_amd.mesh import unit_square_mesh
    fields = ModeFields(unit_square_mesh(6), device=0)
    with open(GOLDEN if len(sys.argv) < 2 else sys.argv[1], "w") as f:
        json.dump(observe(fields), f, indent=1, sort_keys=True)
        f.write("\n")
    fields.close()
