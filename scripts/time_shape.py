"""Timing aid of the shape-sensitivity path: ``shape_response`` and ``ModeFields.velocity_grams`` with
the default core velocities (five per core) for ``--modes`` vectorial and scalar modes of the ``--cores``-core section
(7: C1's geometry), beside the do-nothing-clever alternative: ``ModeFields.profile_tangent_grams`` with the same number
of columns on the same modes, one full tile walk per column.

    python scripts/time_shape.py [--cores 7] [--levels 0] [--modes 22] [--reps 10] [--inner 1.5] [--out FILE]

Run it under ``rocprofv3 --kernel-trace --stats``, in a run of its own, for the kernel times of k_velocity_flag,
k_velocity_count, k_velocity_fill, k_velocity_grams and k_velocity_symmetrise next to k_profile_point_weights and
k_weighted_grams; the wall times printed here include the copies and the launches."""
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
    ap.add_argument("--cores", type=int, default=7)
    ap.add_argument("--levels", type=int, default=0)
    ap.add_argument("--modes", type=int, default=22)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=float, default=1.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pl_fem_vectoriel_amd import (IndexProfile, MCFGeometry, ModeFields, ProfiledGeometry, core_velocities, generate_mesh,
                                      shape_response)
    from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver

    if not torch.cuda.is_available():
        raise SystemExit("time_shape.py needs a GPU")
    geom = MCFGeometry(args.cores, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55)
    mesh = generate_mesh(geom, 1.0, args.levels)
    vel, labels = core_velocities(mesh, geom, inner=args.inner)
    prof = IndexProfile(geom.n_clad)                                    # the step model as a profile: the yardstick's columns
    for (cx, cy), r in zip(np.atleast_2d(geom.positions), geom.core_radii):
        prof.disc((cx, cy), r, geom.n_core)
    pg = ProfiledGeometry(geom, prof, n_core=geom.n_core, n_clad=geom.n_clad)
    unit = prof.unit_tangents()
    tans = [unit[i % len(unit)] for i in range(vel.shape[0])]
    res = {"cores": args.cores, "ne": int(mesh.t.shape[1]), "velocities": int(vel.shape[0])}

    def timed(f):
        best = None
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best * 1e3

    solver = TrueVectorialMaxwellSolver(geom, device=0)
    vec = solver.solve_vectorial_modes(mesh, args.modes)[:args.modes]
    scal = ScalarHelmholtzSolver(geom, device=0).solve(mesh, args.modes)[:args.modes]
    mf = ModeFields(mesh, device=0, solver=solver)
    for kind, modes in (("vectorial", vec), ("scalar", scal)):
        out = mf.velocity_grams(modes, geom, vel)
        res[kind] = {"k": len(modes), "count_min": int(out["count"].min()), "count_max": int(out["count"].max()),
                     "velocity_grams_wall_ms": timed(lambda: mf.velocity_grams(modes, geom, vel)),
                     "shape_response_wall_ms": timed(lambda: shape_response(modes, mf, geom, velocities=vel, labels=labels)),
                     "core_velocities_host_ms": timed(lambda: core_velocities(mesh, geom, inner=args.inner)),
                     "tangent_grams_same_columns_wall_ms": timed(lambda: mf.profile_tangent_grams(modes, pg, tans))}
    mf.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
