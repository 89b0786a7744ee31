"""What plfem_flux_grams and plfem_sample_efields reject, and with which words: every rejection branch of the two calls that
an analysis with interior DOFs can reach is driven once on a 72-element mesh, in the check order include/plfem.h
documents, plus calls with two faults at once (which check comes first).  Every rejected call returns PLFEM_EINVAL, leaves
the full text recorded in tests/golden/power_call_errors.json in plfem_locator_last_error -- it starts with the entry
point's name -- and writes none of its outputs: the host array, the device outputs and the work buffer keep their
sentinel.  Host validation rejects every call here before any launch.  (The interior-DOF check cannot be reached:
plfem_symbolic_create refuses a mesh without interior DOFs, as for the other field calls.)
``python tests/test_gpu_power_call_contract.py`` writes the record anew from the built library (on a GPU)."""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "power_call_errors.json")
K = 3
NPTS = 5
SENTINEL = -7.0
NAN, INF = float("nan"), float("inf")
LAYER = [0.5, 0.5, 0.0, 0.2, 2.2, 2.1, 1.0, 0.0]        # (x, y, r_in, r_out, eps_in, eps_out, g, -)

HEAD = "L ncomp k modes indexed"
MATERIAL = "cores ncore eps_core eps_clad layers nlayer eps_bg use_profile"
ORDER = {
    "plfem_flux_grams": f"{HEAD} {MATERIAL} work nbytes out",
    "plfem_sample_efields": f"{HEAD} beta k0 {MATERIAL} npts points out_dev eps_dev elem",
}
# pointer arguments whose null is a rejection (`eps_dev` may be null; `cores` only with ncore = 0, `layers` only with nlayer = 0)
POINTERS = {
    "plfem_flux_grams": "modes work out cores",
    "plfem_sample_efields": "modes beta points out_dev elem cores",
}


def _bad_layer(j, v):
    row = list(LAYER)
    row[j] = v
    return np.array([row])


def cases(name, good):
    """[(label, {argument: value})] of the rejected calls of one entry point, in the documented check order; ``good`` is
    its accepted argument set (the disc material).  The last cases have two faults."""
    c = []
    add = lambda label, **kw: c.append((label, kw))
    # sizes
    add("ncomp=1", ncomp=1)
    add("ncomp=3", ncomp=3)
    add("k=0", k=0)
    add("k=-1", k=-1)
    if name == "plfem_sample_efields":
        add("npts=-1", npts=-1)
    # core count
    add("ncore=65", ncore=65)
    add("ncore=-1", ncore=-1)
    # null arrays
    for p in POINTERS[name].split():
        add(f"{p}=null", **{p: None})
    # the material: a profile's table ...
    prof = dict(use_profile=1)
    add("profile: nlayer=-1", **prof, nlayer=-1)
    add("profile: nlayer=65", **prof, nlayer=65)
    add("profile: layers=null", **prof, layers=None)
    add("profile: eps_bg=nan", **prof, eps_bg=NAN)
    add("profile: eps_bg=0", **prof, eps_bg=0.0)
    add("profile: layer inf entry", **prof, layers=_bad_layer(0, INF))
    add("profile: layer r_in<0", **prof, layers=_bad_layer(2, -0.1))
    add("profile: layer r_out<=r_in", **prof, layers=_bad_layer(3, 0.0))
    add("profile: layer eps<=0", **prof, layers=_bad_layer(5, 0.0))
    add("profile: layer g<0", **prof, layers=_bad_layer(6, -1.0))
    # ... or the two permittivities of the discs, and no map on the locator
    add("discs: eps_core=nan", eps_core=NAN)
    add("discs: eps_core=-1", eps_core=-1.0)
    add("discs: eps_clad=0", eps_clad=0.0)
    add("discs: eps_clad=inf", eps_clad=INF)
    add("discs: a map on the locator", _map=True)
    if name == "plfem_sample_efields":
        add("k0=nan", k0=NAN)
        add("k0=0", k0=0.0)
        add("k0=-1", k0=-1.0)
        add("k0=inf", k0=INF)
    else:
        add("work one byte short", nbytes=good["nbytes"] - 1)
        add("work misaligned by 8", work=good["work"] + 8)
    # two faults: the earlier check speaks
    add("ncomp=1, ncore=65", ncomp=1, ncore=65)
    add("ncore=65, modes=null", ncore=65, modes=None)
    add("modes=null, discs: eps_core=nan", modes=None, eps_core=NAN)
    add("profile: eps_bg=nan with bad discs", **prof, eps_bg=NAN, eps_core=NAN)
    if name == "plfem_sample_efields":
        add("discs: eps_clad=0, k0=nan", eps_clad=0.0, k0=NAN)
        add("npts=-1, ncore=65", npts=-1, ncore=65)
    else:
        add("discs: eps_clad=0, work one byte short", eps_clad=0.0, nbytes=good["nbytes"] - 1)
        add("work one byte short and misaligned", nbytes=good["nbytes"] - 1, work=good["work"] + 8)
    return c


def observe(mf):
    """{entry point: {case: text}} of the library on ``mf``'s locator.  Asserts on the way that every case is rejected
    with PLFEM_EINVAL and writes no output."""
    import torch
    from pl_fem_vectoriel_amd import _native
    mf._ensure_locator()
    lib, L = mf._lib, mf._loc
    EINVAL, OK = _native.PLFEM_EINVAL, _native.PLFEM_OK
    n = mf.nsolve
    modes = torch.zeros((2, n, K), dtype=torch.float64, device=mf.tdev)
    beta = torch.ones(K, dtype=torch.float64, device=mf.tdev)
    points = torch.zeros((2, NPTS), dtype=torch.float64, device=mf.tdev)
    out_dev = torch.full((4, K, NPTS), SENTINEL, dtype=torch.float64, device=mf.tdev)
    eps_dev = torch.full((NPTS,), SENTINEL, dtype=torch.float64, device=mf.tdev)
    elem = torch.full((NPTS,), int(SENTINEL), dtype=torch.int32, device=mf.tdev)
    out = np.full(4 * K * K, SENTINEL)
    need = ctypes.c_int64(-7)
    assert lib.plfem_flux_gram_work_bytes(K, ctypes.byref(need)) == OK
    work = torch.full((int(need.value) // 8 + 32,), SENTINEL, dtype=torch.float64, device=mf.tdev)
    cores = np.array([[0.3, 0.3, 0.1], [0.7, 0.7, 0.1]])
    head = dict(L=L, ncomp=2, k=K, modes=modes.data_ptr(), indexed=1)
    material = dict(cores=cores, ncore=2, eps_core=2.2, eps_clad=2.1, layers=np.array([LAYER]), nlayer=1, eps_bg=2.1, use_profile=0)
    good = {
        "plfem_flux_grams": dict(head, **material, work=(work.data_ptr() + 255) & ~255, nbytes=int(need.value), out=out),
        "plfem_sample_efields": dict(head, beta=beta.data_ptr(), k0=4.0, **material, npts=NPTS, points=points.data_ptr(),
                                     out_dev=out_dev.data_ptr(), eps_dev=eps_dev.data_ptr(), elem=elem.data_ptr()),
    }
    a_map = np.full((2, 2), 2.0)

    def raw(v):
        return v.ctypes.data_as(ctypes.c_void_p) if isinstance(v, np.ndarray) else v

    def invoke(name, args):
        return getattr(lib, name)(*[raw(args[a]) for a in ORDER[name].split()])

    def set_map(on):
        rc = (lib.plfem_locator_set_index_map(L, raw(a_map), 2, 2, 0.0, 0.0, 1.0, 1.0) if on else
              lib.plfem_locator_set_index_map(L, None, 0, 0, 0.0, 0.0, 0.0, 0.0))
        assert rc == OK

    errors = {}
    for name in ORDER:
        other = next(o for o in ORDER if o != name)
        errors[name] = {}
        for label, kw in cases(name, good[name]):
            kw = dict(kw)
            with_map = kw.pop("_map", False)
            # a rejection of the other entry point in between: the text read below is this call's, not the previous case's
            assert invoke(other, dict(good[other], ncomp=0)) == EINVAL
            if with_map:
                set_map(True)
            try:
                assert invoke(name, {**good[name], **kw}) == EINVAL, (name, label)
                text = lib.plfem_locator_last_error(L).decode()
            finally:
                if with_map:
                    set_map(False)
            assert label not in errors[name]
            errors[name][label] = text
            assert text.startswith(name + ": "), (name, label, text)
    # npts = 0 is no error and launches nothing, whatever the arrays are
    assert invoke("plfem_sample_efields", dict(good["plfem_sample_efields"], npts=0, points=None, out_dev=None, elem=None)) == OK
    torch.cuda.synchronize(mf.tdev)
    assert (out == SENTINEL).all()
    assert bool((work == SENTINEL).all()) and bool((out_dev == SENTINEL).all()) and bool((eps_dev == SENTINEL).all())
    assert bool((elem == int(SENTINEL)).all())
    return errors


def test_rejections_are_the_recorded_ones(gpu_device, built_library):
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
    assert set(got) == set(recorded) == set(ORDER)
    for name, texts in got.items():
        assert texts == recorded[name], name
    # the documented check order: a call with two faults speaks of the earlier one
    for name, texts in got.items():
        assert texts["ncomp=1, ncore=65"] == texts["ncomp=1"]
        assert texts["ncore=65, modes=null"] == texts["ncore=65"]
        assert texts["modes=null, discs: eps_core=nan"] == texts["modes=null"]
        assert texts["profile: eps_bg=nan with bad discs"] == texts["profile: eps_bg=nan"]      # eps_core is not read
    assert got["plfem_sample_efields"]["discs: eps_clad=0, k0=nan"] == got["plfem_sample_efields"]["discs: eps_clad=0"]
    assert got["plfem_sample_efields"]["npts=-1, ncore=65"] == got["plfem_sample_efields"]["npts=-1"]
    assert got["plfem_flux_grams"]["discs: eps_clad=0, work one byte short"] == got["plfem_flux_grams"]["discs: eps_clad=0"]
    assert (got["plfem_flux_grams"]["work one byte short and misaligned"] == got["plfem_flux_grams"]["work one byte short"]
            != got["plfem_flux_grams"]["work misaligned by 8"])
    print({name: len(set(texts.values())) for name, texts in got.items()})


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
