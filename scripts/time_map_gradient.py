"""Timing aid of the pixel gradient of a sampled index map at C1: ``ModeFields.index_map_densities`` and
``index_map_gradient`` for 22 vectorial and 22 scalar modes on a map of NX x NY pixels over the bounding box of the mesh.

    python scripts/time_map_gradient.py [--map 41 33] [--modes 22] [--reps 10] [--unit-tangents] [--out FILE]

The profile is the map alone -- a super-Gaussian cladding plateau in air with seven Gaussian cores, no layers -- so that
every quadrature point inside the map contributes: the heaviest case for the sort and the gather.

``--unit-tangents`` also times the only other route to the same numbers: one unit tangent per pixel through
``ModeFields.profile_tangent_grams`` (eight tangent maps per call), NX NY tangents in all.  It is meant for small maps
(41 x 33: 1 353 tangents) and checks the two routes against each other.

Run it under ``rocprofv3 --kernel-trace --stats``, one map size per run, for the kernel times per family: keys
(k_map_point_keys, k_map_cell_ranges), sort (rocprim's kernels), densities (k_point_densities), gather (k_map_gather);
the wall times printed here include staging, the copies and the launches."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def map_profile(geom, mesh, nx: int, ny: int):
    """n = 1 + 0.45 P + P sum of seven Gaussian cores of 0.085 on the cores of ``geom``, P a super-Gaussian plateau of
    radius 14, sampled on nx x ny pixels over the bounding box of the mesh."""
    from pl_fem_vectoriel_amd import IndexProfile
    x = np.linspace(mesh.p[0].min(), mesh.p[0].max(), nx)
    y = np.linspace(mesh.p[1].min(), mesh.p[1].max(), ny)
    X, Y = np.meshgrid(x, y)
    P = np.exp(-(((X * X + Y * Y) / 196.0) ** 4))
    cores = sum(0.085 * np.exp(-((X - cx) ** 2 + (Y - cy) ** 2) / 1.5 ** 2) for cx, cy in np.atleast_2d(geom.positions))
    return IndexProfile(1.0).sampled(x, y, 1.0 + 0.45 * P + P * cores)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", type=int, nargs=2, metavar=("NX", "NY"), default=(41, 33))
    ap.add_argument("--modes", type=int, default=22)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--unit-tangents", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pl_fem_vectoriel_amd import MCFGeometry, ModeFields, ProfiledGeometry, generate_mesh, index_map_gradient
    from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver

    if not torch.cuda.is_available():
        raise SystemExit("time_map_gradient.py needs a GPU")
    geom = MCFGeometry(7, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55)
    mesh = generate_mesh(geom, 1.0, 1)
    nx, ny = args.map
    prof = map_profile(geom, mesh, nx, ny)
    pg = ProfiledGeometry(geom, prof)
    res = {"ne": int(mesh.t.shape[1]), "points": 6 * int(mesh.t.shape[1]), "map": [nx, ny]}

    def timed(f, reps=args.reps):
        best = None
        for _ in range(reps):
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
        G = mf.index_map_densities(modes, pg)                                # (warm-up: locator, map upload)
        sup = G["support"]
        r = {"k": len(modes), "nodes_seen": int((sup > 0).sum()), "longest_list": int(sup.max()),
             "densities_wall_ms": timed(lambda: mf.index_map_densities(modes, pg)),
             "gradient_wall_ms": timed(lambda: index_map_gradient(modes, mf, pg))}
        if args.unit_tangents:
            E = prof.index_map[0]
            tans = []
            for j in range(ny):
                for i in range(nx):
                    d = np.zeros_like(E)
                    d[j, i] = 1.0
                    tans.append(prof.tangent_eps(0.0, 0.0, d))

            def route():
                out = []
                for s in range(0, len(tans), 256):
                    out.append(mf.profile_tangent_grams(modes, pg, tans[s:s + 256]))
                return out

            t0 = time.perf_counter()
            parts = route()
            torch.cuda.synchronize()
            r["unit_tangents"] = len(tans)
            r["unit_tangent_grams_wall_ms"] = min((time.perf_counter() - t0) * 1e3, timed(route, reps=max(1, args.reps // 5)))
            worst = 0.0
            for nm, tnm in (("M_px", "M_d"), ("K_px", "K_d")) if kind == "vectorial" else (("M_px", "M_d"),):
                T = np.concatenate([p[tnm] for p in parts])                  # (npix, k, k)
                diag = np.einsum("tkk->kt", T).reshape(len(modes), ny, nx)
                worst = max(worst, float((np.abs(diag - G[nm]).max(axis=(1, 2)) / np.abs(G[nm]).max(axis=(1, 2))).max()))
            r["routes_agree_to"] = worst
        res[kind] = r
    mf.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
