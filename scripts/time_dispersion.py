"""Timing aid of the group-index path at C1 (vectorial, 22 modes): ``ModeFields.grams`` (staging + k_mode_grams +
k_overlap_reduce + copy) and the whole ``mode_dispersion`` call, for vectorial and scalar records.

    python scripts/time_dispersion.py [--modes 22] [--reps 5] [--out FILE]

Run it under ``rocprofv3 --kernel-trace --stats`` for the kernel times (k_mode_grams, k_overlap_reduce, k_stage_modes);
the wall times printed here include the host-device copies and the k x k host math."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pl_fem_vectoriel_amd import MCFGeometry, ModeFields, generate_mesh, mode_dispersion
    from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver

    if not torch.cuda.is_available():
        raise SystemExit("time_dispersion.py needs a GPU")
    geom = MCFGeometry(7, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55)
    mesh = generate_mesh(geom, 1.0, 1)
    solver = TrueVectorialMaxwellSolver(geom, device=0)
    vec = solver.solve_vectorial_modes(mesh, args.modes)[:args.modes]
    scal = ScalarHelmholtzSolver(geom, device=0).solve(mesh, args.modes)[:args.modes]
    mf = ModeFields(mesh, device=0, solver=solver)
    nq = 6 * int(mesh.t.shape[1])
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

    for kind, modes in (("vectorial", vec), ("scalar", scal)):
        k = len(modes)
        ncomp = 2 if kind == "vectorial" else 1
        nrows = mf.nsolve if kind == "vectorial" else mf.N
        t_g, _ = timed(lambda: mf.grams(modes, geom))
        t_d, d = timed(lambda: mode_dispersion(modes, mf, geom))
        # products per (point, mode pair): vectorial 10 (M 2, K 4, D 4), scalar 3; 2 FLOP each
        flop = 2.0 * nq * k * k * (10 if kind == "vectorial" else 3)
        res[kind] = {"k": k, "staged_mb": ncomp * nrows * k * 8 / 1e6, "gram_flop": flop, "grams_wall_ms": t_g,
                     "mode_dispersion_wall_ms": t_d, "rayleigh_defect_max": float(d["rayleigh_defect"].max()),
                     "n_g_min": float(d["n_g"].min()), "n_g_max": float(d["n_g"].max()),
                     "dmgd_ps_per_m": d["dmgd_ps_per_m"], "clusters": int(d["cluster"].max()) + 1}
    mf.close()
    line = json.dumps(res, default=lambda o: float(o) if isinstance(o, np.floating) else str(o))
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
