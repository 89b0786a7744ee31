"""Timing aid of the bend path at C1 (22 modes): ``ModeFields.moment_grams`` (staging + k_moment_grams + k_overlap_reduce +
copy) and the whole ``bend_response`` call, for vectorial and scalar records, beside ``ModeFields.grams``.

    python scripts/time_bend.py [--modes 22] [--reps 5] [--out FILE]

Run it under ``rocprofv3 --kernel-trace --stats`` for the kernel times of k_moment_grams (two instances for vectorial
records) next to k_mode_grams; the wall times printed here include the host-device copies and the k x k host math."""
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
    from pl_fem_vectoriel_amd import MCFGeometry, ModeFields, bend_response, generate_mesh
    from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver

    if not torch.cuda.is_available():
        raise SystemExit("time_bend.py needs a GPU")
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

    radii = np.array([np.inf, 8000.0, 4000.0, 2000.0])
    for kind, modes in (("vectorial", vec), ("scalar", scal)):
        k = len(modes)
        t_g, _ = timed(lambda: mf.grams(modes, geom))
        t_m, _ = timed(lambda: mf.moment_grams(modes, geom))
        t_b, b = timed(lambda: bend_response(modes, mf, geom, radius=radii, angle=0.3))
        # products per (point, mode pair): vectorial 2 + 4 (m, kk) + 4 x 11 (the outputs), scalar 1 + 4 x 7; k_mode_grams 14 and 3
        flop = 2.0 * nq * k * k * (50 if kind == "vectorial" else 29)
        res[kind] = {"k": k, "moment_gram_flop": flop, "grams_wall_ms": t_g, "moment_grams_wall_ms": t_m,
                     "bend_response_wall_ms": t_b, "rayleigh_defect_max": float(b["rayleigh_defect"].max()),
                     "dneff_dkappa_max_um": float(np.abs(b["dneff_dkappa"]).max()),
                     "d4sigma_min_um": float(b["width_d4sigma"].min()), "d4sigma_max_um": float(b["width_d4sigma"].max()),
                     "n_eff_shift_max": [float(np.nanmax(np.abs(b["n_eff_ritz"][i] - b["n_eff_ritz"][0]))) for i in range(1, 4)],
                     "clusters": int(b["cluster"].max()) + 1}
    mf.close()
    line = json.dumps(res, default=lambda o: float(o) if isinstance(o, np.floating) else str(o))
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
