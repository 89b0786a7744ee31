"""Timing aid of the posed overlaps at C1, mesh level 0, 22 scalar modes on both sides (the set spliced onto itself):

* ``map``: the 41 x 41 offset map (1681 poses) -- ``mode_overlap_poses`` alone and the whole ``splice_map`` call;
* ``single``: one identity pose per call, ``--reps`` calls;
* ``baseline``: ``mode_overlap`` of the same pair (k_field_overlap), ``--reps`` calls;
* ``flux_map``, ``flux_single``: the same map and the same single identity pose with vectorial records of the same
  geometry and mesh -- ``flux_overlap_poses`` (k_flux_overlap_posed) and, as its yardstick on the same records and poses,
  ``mode_overlap_poses`` (k_field_overlap_posed); ``flux_map`` also times the whole ``splice_power_map`` call.  ``all``
  runs the three scalar legs only.

    python scripts/time_splice.py [--leg map|single|baseline|flux_map|flux_single|all] [--grid 41] [--span 4.0] [--modes 22]
                                  [--reps 5] [--out FILE]

Run one leg at a time under ``rocprofv3 --kernel-trace --stats`` for the kernel times (k_field_overlap_posed, k_field_overlap,
k_overlap_reduce, k_stage_modes): the statistics are per kernel name, so legs run together would mix.  The wall times
printed here include staging, the host-device copies and the k x k host math."""
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
    ap.add_argument("--leg", default="all", choices=("map", "single", "baseline", "flux_map", "flux_single", "all"))
    ap.add_argument("--grid", type=int, default=41, help="offsets per axis of the map")
    ap.add_argument("--span", type=float, default=4.0, help="the offsets run over [-span, span] um")
    ap.add_argument("--modes", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pl_fem_vectoriel_amd import MCFGeometry, ModeFields, generate_mesh, mode_overlap
    from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver

    if not torch.cuda.is_available():
        raise SystemExit("time_splice.py needs a GPU")
    geom = MCFGeometry(7, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55)
    mesh = generate_mesh(geom, 1.0, 0)
    modes = ScalarHelmholtzSolver(geom, device=0).solve(mesh, args.modes)[:args.modes]
    mf = ModeFields(mesh, device=0)
    nq = 6 * int(mesh.t.shape[1])
    res = {"k": len(modes), "ne": int(mesh.t.shape[1]), "quadrature_points": nq, "tiles": (nq + 63) // 64}

    def timed(f, reps):
        best, out = None, None
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best * 1e3, out

    mode_overlap(modes[:1], mf, modes[:1], mf)               # the locator, outside the timings
    if args.leg in ("baseline", "all"):
        t, O = timed(lambda: mode_overlap(modes, mf, modes, mf), args.reps)
        res["baseline"] = {"calls": args.reps, "wall_ms": t, "offdiag_max": float(np.abs(O - np.diag(np.diag(O))).max())}
    if args.leg in ("single", "map", "all"):
        from pl_fem_vectoriel_amd import mode_overlap_poses, pose_table, splice_map
    if args.leg in ("single", "all"):
        t, O = timed(lambda: mode_overlap_poses(modes, mf, modes, mf, pose_table()), args.reps)
        ref = mode_overlap(modes, mf, modes, mf) if args.leg == "all" else None
        res["single"] = {"calls": args.reps, "wall_ms": t,
                         "rel_diff_to_mode_overlap": None if ref is None else float(np.abs(O[0] - ref).max() / np.abs(ref).max())}
    if args.leg in ("map", "all"):
        x = np.linspace(-args.span, args.span, args.grid)
        poses = pose_table(x[None, :], x[:, None])
        t_o, O = timed(lambda: mode_overlap_poses(modes, mf, modes, mf, poses), 1)
        t_s, r = timed(lambda: splice_map(modes, mf, modes, mf, x, x), 1)
        c = args.grid // 2
        res["map"] = {"poses": int(poses.shape[0]), "mode_overlap_poses_wall_ms": t_o, "splice_map_wall_ms": t_s,
                      "posed_kernel_calls": 2, "IL_dB_centre": float(r["IL_dB"][c, c]), "IL_dB_corner": float(r["IL_dB"][0, 0]),
                      "IL_dB_one_step": float(r["IL_dB"][c, c + 1]), "step_um": float(x[1] - x[0]),
                      "map_equals_overlaps": bool(np.array_equal(r["overlap"].reshape(O.shape), O))}
    if args.leg in ("flux_map", "flux_single"):
        from pl_fem_vectoriel_amd import flux_overlap_poses, mode_overlap_poses, pose_table, splice_map, splice_power_map
        from pl_fem_vectoriel_amd.solver_fem import TrueVectorialMaxwellSolver
        vmodes = TrueVectorialMaxwellSolver(geom, device=0).solve_vectorial_modes(mesh, n_modes_target=args.modes)[:args.modes]
        res["k_vectorial"] = len(vmodes)
        mf.flux_grams(vmodes[:1], geom)                      # the staging path, outside the timings (another kernel's name)
    if args.leg == "flux_single":
        t_f, G = timed(lambda: flux_overlap_poses(vmodes, mf, geom, vmodes, mf, geom, pose_table()), args.reps)
        t_h, O = timed(lambda: mode_overlap_poses(vmodes, mf, vmodes, mf, pose_table()), args.reps)
        F = mf.flux_grams(vmodes, geom)
        M = F["M_w_core"] + F["M_w_rest"]
        res["flux_single"] = {"calls": args.reps, "flux_wall_ms": t_f, "field_wall_ms": t_h,
                              "MA_rel_diff_to_flux_grams": float(np.abs(G["MA"][0] - M).max() / np.abs(M).max())}
    if args.leg == "flux_map":
        x = np.linspace(-args.span, args.span, args.grid)
        poses = pose_table(x[None, :], x[:, None])
        t_f, G = timed(lambda: flux_overlap_poses(vmodes, mf, geom, vmodes, mf, geom, poses), 1)
        t_h, O = timed(lambda: mode_overlap_poses(vmodes, mf, vmodes, mf, poses), 1)
        t_s, r = timed(lambda: splice_power_map(vmodes, mf, geom, vmodes, mf, geom, x, x), 1)
        hh = splice_map(vmodes, mf, vmodes, mf, x, x)
        c = args.grid // 2
        res["flux_map"] = {"poses": int(poses.shape[0]), "flux_overlap_poses_wall_ms": t_f, "mode_overlap_poses_wall_ms": t_h,
                           "splice_power_map_wall_ms": t_s, "flux_kernel_calls": 2, "field_kernel_calls": 2,
                           "IL_dB_centre": float(r["IL_dB"][c, c]), "IL_dB_one_step": float(r["IL_dB"][c, c + 1]),
                           "IL_dB_corner": float(r["IL_dB"][0, 0]), "hh_IL_dB_centre": float(hh["IL_dB"][c, c]),
                           "hh_IL_dB_one_step": float(hh["IL_dB"][c, c + 1]), "hh_IL_dB_corner": float(hh["IL_dB"][0, 0]),
                           "step_um": float(x[1] - x[0]), "offdiag_T_centre_max":
                           float(np.abs(r["transfer"][c, c] - np.diag(np.diag(r["transfer"][c, c]))).max())}
    mf.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
