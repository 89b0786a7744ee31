"""No C++ exception crosses the C ABI: a host-side allocation failure inside an entry point comes back as
PLFEM_EHOST with the cause in the message, and the calling process lives on.  Runs in a child process that loads the
library without opening a GPU and then lowers its address-space limit below what the call needs."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes, json, resource
import numpy as np
from pl_fem_vectoriel_amd import _native

lib = _native.load_library()
n = 1000                                     # structured n x n square, two triangles per cell: 2e6 elements
ij = np.arange((n + 1) ** 2).reshape(n + 1, n + 1)
x, y = np.meshgrid(np.linspace(0.0, 1.0, n + 1), np.linspace(0.0, 1.0, n + 1))
p = np.ascontiguousarray(np.stack([x.ravel(), y.ravel()]))
a, b, c, d = ij[:-1, :-1].ravel(), ij[:-1, 1:].ravel(), ij[1:, :-1].ravel(), ij[1:, 1:].ravel()
t = np.ascontiguousarray(np.concatenate([np.stack([a, b, d]), np.stack([a, d, c])], axis=1).astype(np.int32))
nv, ne = p.shape[1], t.shape[1]
p_out = np.empty((2, nv + 3 * n * n + 2 * n))
t_out = np.empty((3, 4 * ne), dtype=np.int32)
err = ctypes.create_string_buffer(512)
margin = 48 << 20                            # the numbering of this mesh needs several times as much
with open("/proc/self/statm") as f:
    vm_bytes = int(f.read().split()[0]) * resource.getpagesize()
soft, hard = resource.getrlimit(resource.RLIMIT_AS)
try:
    if hard != resource.RLIM_INFINITY and hard < vm_bytes + margin:
        raise ValueError("hard limit too low")
    resource.setrlimit(resource.RLIMIT_AS, (vm_bytes + margin, hard))
except (ValueError, OSError) as e:
    print(json.dumps({"skip": str(e)}))
    raise SystemExit(0)
rc = lib.plfem_mesh_refine(nv, ne, p.ctypes.data, t.ctypes.data, p_out.ctypes.data, t_out.ctypes.data, err, 512)
resource.setrlimit(resource.RLIMIT_AS, (soft, hard))
print(json.dumps({"rc": rc, "msg": err.value.decode()}))
"""


def test_host_allocation_failure_returns_ehost(built_library):
    from pl_fem_vectoriel_amd import _native

    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    res = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, f"child died ({res.returncode}): {res.stderr[-2000:]}"
    out = json.loads(res.stdout.strip().splitlines()[-1])
    if "skip" in out:
        pytest.skip(f"cannot lower RLIMIT_AS here: {out['skip']}")
    assert out["rc"] == _native.PLFEM_EHOST, out
    assert out["msg"], out
