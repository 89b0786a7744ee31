"""``bench.py --dump-outputs DIR`` on the headline configuration: ``--steps`` timed steps, the mode records of the last
one written as float64 arrays within 64 MB, the same arrays from a second run with the same arguments, and n_eff as
the CPU oracle computes it on the same mesh."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_dump(out_dir):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "PLFEM_BENCH_FAKE", "PLFEM_BENCH_FORCE_DIST")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--no-cpu-baseline", "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_dump_outputs_of_the_headline_step(tmp_path, gpu_device, built_library):
    from pl_fem_vectoriel_amd import MCFGeometry, generate_mesh
    from oracle import hfield
    from oracle.p2 import MeshTriLite

    lines = [_bench_dump(tmp_path / d) for d in ("a", "b")]
    for d in lines:
        assert d["steps"] == 3 and len(d["step_ms"]) == 3 and d["ms_per_step"] > 0
        assert 0 < d["outputs_dumped"]["bytes"] <= 64 << 20
    names = lines[0]["outputs_dumped"]["arrays"]
    assert {"n_eff", "beta", "Ex_dofs", "Ey_dofs"} <= set(names) and names == lines[1]["outputs_dumped"]["arrays"]
    for name in names:
        a, b = (np.load(tmp_path / d / f"{name}.npy") for d in ("a", "b"))
        assert a.dtype == np.float64 and a.shape == b.shape, name
        assert np.allclose(a, b, rtol=1e-9, atol=1e-9), name            # same inputs, same outputs
    ex = np.load(tmp_path / "a" / "Ex_dofs.npy")
    n_eff = np.load(tmp_path / "a" / "n_eff.npy")
    assert ex.shape[0] == len(n_eff) > 0 and np.all(np.isfinite(ex))
    # the headline workload (C1) through the oracle: the same modes
    geom = MCFGeometry(7, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55)
    mesh = generate_mesh(geom, 1.0, 1)
    ref = hfield.solve_vectorial_modes(geom, MeshTriLite(mesh.p, mesh.t), 10, fused=True)
    assert len(ref) == len(n_eff)
    assert np.max(np.abs(n_eff - np.array([m["n_eff"] for m in ref]))) < 5e-5
