"""Timing aid of the nonlinear-overlap path at C1: ``ModeFields.quartic`` (staging + k_mode_quartic + k_quartic_reduce +
copy) and the whole ``mode_nonlinearity`` call for 22 vectorial and 22 scalar solver records, ``ModeFields.quartic`` for
k = 64 random fields, and the NumPy emulation (tests/quartic_emulation.py) of the scalar k = 22 call on the host for
scale.

    python scripts/time_nonlinear.py [--modes 22] [--reps 5] [--out FILE]

Run it under ``rocprofv3 --kernel-trace --stats`` for the kernel times (k_mode_quartic, k_quartic_reduce); the wall
times printed here include the host-device copies and the host math.  TFLOP/s counts the useful products only: 2 FLOP
per quadrature point and pair of pairs on the upper triangle."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pl_fem_vectoriel_amd import MCFGeometry, ModeFields, generate_mesh, mode_nonlinearity
    from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver

    if not torch.cuda.is_available():
        raise SystemExit("time_nonlinear.py needs a GPU")
    geom = MCFGeometry(7, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55)
    mesh = generate_mesh(geom, 1.0, 1)
    solver = TrueVectorialMaxwellSolver(geom, device=0)
    vec = solver.solve_vectorial_modes(mesh, args.modes)[:args.modes]
    scal = ScalarHelmholtzSolver(geom, device=0).solve(mesh, args.modes)[:args.modes]
    mf = ModeFields(mesh, device=0, solver=solver)
    nq = 16 * int(mesh.t.shape[1])
    res = {"ne": int(mesh.t.shape[1]), "quadrature_points": nq}

    def timed(f):
        best, out = None, None
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best * 1e3, out

    def useful_flop(k):
        npair = k * (k + 1) // 2
        return 2.0 * nq * npair * (npair + 1) / 2

    for kind, modes in (("vectorial", vec), ("scalar", scal)):
        k = len(modes)
        t_q, Q = timed(lambda: mf.quartic(modes))
        t_n, d = timed(lambda: mode_nonlinearity(modes, mf, geom, n2=(2.6e-20, 0.0)))
        res[kind] = {"k": k, "useful_flop": useful_flop(k), "quartic_wall_ms": t_q, "mode_nonlinearity_wall_ms": t_n,
                     "a_eff_um2_min": float(d["a_eff"].min()), "a_eff_um2_max": float(d["a_eff"].max()),
                     "mfd_um_min": float(d["mfd_petermann"].min()), "mfd_um_max": float(d["mfd_petermann"].max())}
        if kind == "scalar":
            from quartic_emulation import QuarticEmulation
            em = QuarticEmulation(mesh.p, mesh.t)
            vals = np.array([m["field_vector"] for m in modes])[None]
            t0 = time.perf_counter()
            ref = em.quartic(vals, False)
            res[kind]["numpy_emulation_ms"] = (time.perf_counter() - t0) * 1e3
            res[kind]["rel_err_vs_emulation"] = float(np.abs(Q - ref).max() / np.abs(ref).max())
    k = 64
    rng = np.random.default_rng(0)
    rnd = [{"field_vector": rng.standard_normal(mf.N)} for _ in range(k)]
    t_r, _ = timed(lambda: mf.quartic(rnd))
    res["random_k64_scalar"] = {"k": k, "useful_flop": useful_flop(k), "quartic_wall_ms": t_r}
    mf.close()
    line = json.dumps(res, default=lambda o: float(o) if isinstance(o, np.floating) else str(o))
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
