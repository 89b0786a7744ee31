"""Timing aid of the sampled projection at C1 (vectorial, 22 modes, mesh level 1): ``ModeFields.project_sampled`` on
batches of ``--pixels`` x ``--pixels`` complex frames over the mesh's bounding box, one batch size per entry of ``--nf``,
and, with ``--baseline``, what the package offered before for the same numbers: ``ModeFields.sample`` at the points of
the 16-point rule (k x Q values to the host), the host's bilinear interpolation (a sparse Q x pixels matrix) and the
matmul, per batch; and the host matmul alone on the cached modes-to-pixels matrix, which serves a caller whose modes and
grid stay fixed over many batches.

    python scripts/time_sampled_projection.py [--nf 8,64,1024] [--pixels 128] [--reps 5] [--baseline] [--out FILE]

Run it under ``rocprofv3 --kernel-trace --stats`` (one ``--nf`` per run, without ``--baseline``) for the kernel times of
k_mode_project_sampled and k_project_sampled_reduce: a batch of more than 512 frames takes one launch of each per 512;
the wall times printed here include the upload of the frames and their permutation on the device."""
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
    ap.add_argument("--nf", default="8,64,1024", help="frames per batch, one timing each")
    ap.add_argument("--pixels", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--modes", type=int, default=22)
    ap.add_argument("--baseline", action="store_true", help="also time sample + host interpolation + matmul")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pl_fem_vectoriel_amd import MCFGeometry, ModeFields, generate_mesh
    from pl_fem_vectoriel_amd.solver_fem import TrueVectorialMaxwellSolver

    if not torch.cuda.is_available():
        raise SystemExit("time_sampled_projection.py needs a GPU")
    geom = MCFGeometry(7, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55)
    mesh = generate_mesh(geom, 1.0, 1)
    solver = TrueVectorialMaxwellSolver(geom, device=0)
    modes = solver.solve_vectorial_modes(mesh, args.modes)[:args.modes]
    mf = ModeFields(mesh, device=0, solver=solver)
    n = args.pixels
    x, y = np.linspace(mf.bbox[0], mf.bbox[1], n), np.linspace(mf.bbox[2], mf.bbox[3], n)
    nq = 16 * mesh.t.shape[1]
    res = {"k": len(modes), "ne": int(mesh.t.shape[1]), "nq": nq, "pixels": n, "reps": args.reps, "batches": {}}
    rng = np.random.default_rng(5)

    def timed(f):
        f()                                                          # warm-up of this shape
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return out, min(times) * 1e3, float(np.median(times)) * 1e3

    if args.baseline:
        from scipy import sparse
        from sampled_projection_emulation import SampledProjectionEmulation
        em = SampledProjectionEmulation(mesh.p, mesh.t)
        X, Y = em.points16()
        pts = np.vstack([X.reshape(-1), Y.reshape(-1)])
        wq = em.weights16().reshape(-1)
        tx, ty = (t.reshape(-1) for t in em.grid_coordinates(x, y))
        i0 = np.minimum(np.floor(tx).astype(np.int64), n - 2)
        j0 = np.minimum(np.floor(ty).astype(np.int64), n - 2)
        a, b = tx - i0, ty - j0
        rows = np.tile(np.arange(nq), 4)
        cols = np.concatenate([j0 * n + i0, j0 * n + i0 + 1, (j0 + 1) * n + i0, (j0 + 1) * n + i0 + 1])
        wts = np.concatenate([(1 - a) * (1 - b), a * (1 - b), (1 - a) * b, a * b])
        W = sparse.csr_matrix((wts, (rows, cols)), shape=(nq, n * n))          # (the bounding box holds every point)

        def to_pixels():
            s = mf.sample(modes, pts, hz=False)
            U = np.concatenate([s["Hx"], s["Hy"]]) * wq[None]        # (2 k, Q), the order of the amplitude's first two axes
            return (W.T @ U.T).T                                     # (2 k, pixels): the modes on the pixels' hat functions

    for nf in (int(v) for v in args.nf.split(",")):
        frames = rng.standard_normal((nf, n, n)) + 1j * rng.standard_normal((nf, n, n))
        P, best, med = timed(lambda: mf.project_sampled(modes, frames, x, y))
        entry = {"wall_ms": best, "wall_ms_median": med, "flop": 2.0 * 2 * len(modes) * 2 * nf * nq, "max_abs": float(np.abs(P).max())}
        if args.baseline:
            flat = frames.reshape(nf, -1).T                          # (pixels, nf)
            ref, best, med = timed(lambda: to_pixels() @ flat)
            entry["baseline_wall_ms"], entry["baseline_wall_ms_median"] = best, med
            entry["baseline_rel_diff"] = float(np.abs(ref.reshape(P.shape) - P).max() / np.abs(P).max())
            G = to_pixels()
            _, best, med = timed(lambda: G @ flat)
            entry["cached_matmul_wall_ms"], entry["cached_matmul_wall_ms_median"] = best, med
        res["batches"][str(nf)] = entry
        print(f"nf = {nf}: {json.dumps(entry)}", flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
