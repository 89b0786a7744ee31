"""Work-buffer sizes of the field calls, host side (no GPU): every sizer that needs no locator returns the bytes recorded in
tests/golden/field_work_bytes.json at the chunk and instance boundaries of its kernels, and rejects what it rejected
when the record was made, leaving ``*bytes`` alone.  The record pins the layouts: a change of one is a change of the C
ABI's contract with callers that keep a work buffer.  ``python tests/test_field_work_bytes_host.py`` writes the record
anew from the built library."""
import ctypes
import itertools
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "field_work_bytes.json")

NCOMP = (1, 2)
K64 = (1, 31, 32, 33, 64)               # calls of at most 64 modes
K = K64 + (65, 96)
KAB = (0, 1, 32, 33)
LAB = (1, 8, 9, 4096)
NF = (1, 32, 33, 1025, 4096)

# sizer -> (accepted argument tuples, rejected argument tuples)
SIZERS = {
    "plfem_overlap_work_bytes": (list(itertools.product(KAB, KAB)), [(-1, 1), (1, -1)]),
    "plfem_gram_work_bytes": (list(itertools.product(NCOMP, K)), [(0, 1), (3, 1), (1, 0), (1, -1)]),
    "plfem_profile_gram_work_bytes": (list(itertools.product(NCOMP, K)), [(0, 1), (3, 1), (1, 0), (1, -1)]),
    "plfem_moment_gram_work_bytes": (list(itertools.product(NCOMP, K)), [(0, 1), (3, 1), (1, 0), (1, -1)]),
    "plfem_quartic_work_bytes": (list(itertools.product(NCOMP, K64)), [(0, 1), (3, 1), (1, 0), (1, -1), (1, 65), (2, 65)]),
    "plfem_project_work_bytes": (list(itertools.product(NCOMP, K64, LAB, LAB)),
                                 [(0, 1, 1, 1), (3, 1, 1, 1), (1, 0, 1, 1), (1, -1, 1, 1), (1, 65, 1, 1), (1, 1, 4097, 1),
                                  (1, 1, 1, 4097), (1, 1, 0, 1), (1, 1, 1, 0)]),
    "plfem_project_sampled_work_bytes": (list(itertools.product(NCOMP, K64, NF)),
                                         [(0, 1, 1), (3, 1, 1), (1, 0, 1), (1, -1, 1), (1, 65, 1), (1, 1, 4097), (1, 1, 0)]),
}


def key(name, args):
    return f"{name}({', '.join(str(a) for a in args)})"


def observe(lib):
    """{call: bytes} of every accepted call; the rejections are asserted on the way."""
    from pl_fem_vectoriel_amd import _native
    sizes = {}
    for name, (accepted, rejected) in SIZERS.items():
        fn = getattr(lib, name)
        for args in accepted:
            need = ctypes.c_int64(-7)
            assert fn(*args, ctypes.byref(need)) == _native.PLFEM_OK, key(name, args)
            sizes[key(name, args)] = int(need.value)
            assert fn(*args, None) == _native.PLFEM_EINVAL, key(name, args)                 # a null `bytes`
        for args in rejected:
            need = ctypes.c_int64(-7)
            assert fn(*args, ctypes.byref(need)) == _native.PLFEM_EINVAL, key(name, args)
            assert need.value == -7, key(name, args)
    return sizes


def test_sizers_return_the_recorded_bytes(built_library):
    with open(GOLDEN) as f:
        recorded = json.load(f)
    got = observe(built_library)
    assert set(got) == set(recorded)
    assert {c: (got[c], recorded[c]) for c in got if got[c] != recorded[c]} == {}


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pl_fem_vectoriel_amd import _native
    with open(GOLDEN, "w") as f:
        json.dump(observe(_native.load_library()), f, indent=0, sort_keys=True)
        f.write("\n")
