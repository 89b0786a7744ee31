"""Timing aid of the per-core path at C1 (22 modes): ``ModeFields.core_grams`` (staging + k_core_owner + k_core_count +
k_core_fill + k_core_grams + k_overlap_reduce + copy) and the whole ``core_decomposition`` call, for vectorial and scalar
records, beside ``ModeFields.grams``.

    python scripts/time_cores.py [--modes 22] [--reps 5] [--out FILE]

Run it under ``rocprofv3 --kernel-trace --stats`` for the kernel times of the three passes (k_core_owner; k_core_count and
k_core_fill; k_core_grams) next to k_mode_grams; the wall times printed here include the host-device copies and the
k x k host math."""
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
    from pl_fem_vectoriel_amd import MCFGeometry, ModeFields, core_decomposition, generate_mesh
    from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver

    if not torch.cuda.is_available():
        raise SystemExit("time_cores.py needs a GPU")
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

    ones = np.ones(geom.n_cores)
    for kind, modes in (("vectorial", vec), ("scalar", scal)):
        k = len(modes)
        t_g, _ = timed(lambda: mf.grams(modes, geom))
        t_c, c = timed(lambda: mf.core_grams(modes, geom))
        t_d, d = timed(lambda: core_decomposition(modes, mf, geom, n_cores=geom.n_core * ones, direction=ones))
        owned = int(c["points"].sum())
        # products per (owned point, mode pair): vectorial 6 (Mx 1, My 1, K 4), scalar 1; 2 FLOP each
        flop = 2.0 * owned * k * k * (6 if kind == "vectorial" else 1)
        res[kind] = {"k": k, "points": c["points"].tolist(), "owned_points": owned, "core_gram_flop": flop,
                     "grams_wall_ms": t_g, "core_grams_wall_ms": t_c, "core_decomposition_wall_ms": t_d,
                     "rayleigh_defect_max": float(d["rayleigh_defect"].max()),
                     "power_in_cores_min": float(d["power"].sum(1).min()), "power_in_cores_max": float(d["power"].sum(1).max()),
                     "dneff_dn_max": float(np.abs(d["dneff_dn"]).max()), "clusters": int(d["cluster"].max()) + 1}
    mf.close()
    line = json.dumps(res, default=lambda o: float(o) if isinstance(o, np.floating) else str(o))
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
