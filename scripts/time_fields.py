"""Timing aid of the mode-field calls at C1 (vectorial, 22 modes): sampling on an nx x nx grid with Hx, Hy, Hz_im;
mode_overlap C1 -> C1 refined (the C1 modes sampled at the DOF locations of mesh.refined(): ~1.1 M quadrature points of
the finer mesh, 22 x 22); locator build times at C1 and L = 2; the projection on a 1 x 1 Gaussian beam and on 64 x 64 and
256 x 256 plane-wave grids up to k0 (``ModeFields.project``); optionally the NumPy emulation of the same calls (the
projection up to ``--emulation-grid`` factors per axis: the 256 x 256 grid would take the host hours); the power leg:
``ModeFields.flux_grams`` with the discs, with the seven cores written as seven layers and with those layers over a sampled
map, next to ``ModeFields.profile_grams`` on the same two profiles (the yardstick), and ``ModeFields.sample_grid_e`` next to
``ModeFields.sample_grid`` on the same grid.

    python scripts/time_fields.py [--grid 1024] [--reps 3] [--project-only | --power-only] [--emulation] [--out FILE]

Run it under ``rocprofv3 --kernel-trace --stats`` for the kernel times (k_sample_fields, k_field_overlap,
k_overlap_reduce, k_stage_modes, k_mode_project, k_project_reduce, k_flux_grams, k_profile_grams, k_sample_efields; the
power leg dispatches each kernel instance ``--reps`` times, in the order discs, layers, map; the projection leg dispatches k_mode_project ``--reps``
times per grid, in the order of ``--project-grids``); the wall times printed here include the host-device copies."""
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
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", type=int, default=22)
    ap.add_argument("--emulation", action="store_true", help="also time the NumPy emulation (minutes)")
    ap.add_argument("--project-only", action="store_true", help="run the projection leg alone")
    ap.add_argument("--power-only", action="store_true", help="run the power leg alone")
    ap.add_argument("--project-grids", default="1,64,256", help="factors per axis of the projection leg (1: one Gaussian beam)")
    ap.add_argument("--emulation-grid", type=int, default=64, help="largest projection grid the emulation is timed on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pl_fem_vectoriel_amd import MCFGeometry, ModeFields, generate_mesh, mode_overlap
    from pl_fem_vectoriel_amd import _native
    from pl_fem_vectoriel_amd.solver_fem import TrueVectorialMaxwellSolver

    if not torch.cuda.is_available():
        raise SystemExit("time_fields.py needs a GPU")
    geom = MCFGeometry(7, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55)
    mesh = generate_mesh(geom, 1.0, 1)
    fine = mesh.refined()
    solver = TrueVectorialMaxwellSolver(geom, device=0)
    modes = solver.solve_vectorial_modes(mesh, args.modes)[:args.modes]
    res = {"k": len(modes), "ne_c1": int(mesh.t.shape[1]), "ne_l2": int(fine.t.shape[1])}

    # locator build (host) on fresh analyses
    for name, m in () if args.project_only or args.power_only else (("c1", mesh), ("l2", fine)):
        sym = _native.Symbolic(m.p, m.t)
        t0 = time.perf_counter()
        st = sym.array("loc_stats")
        res[f"locator_{name}"] = {"build_ms": st[3] * 1e3, "wall_ms": (time.perf_counter() - t0) * 1e3, "cells": int(st[0]),
                                  "mean_candidates": float(st[1]), "max_candidates": int(st[2])}

    mf = ModeFields(mesh, device=0, solver=solver)
    mf1 = ModeFields(fine, device=0)

    def timed(f):
        best = None
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return out, best

    if args.power_only:
        power_leg(args, geom, mf, modes, timed, res)
        return finish(args, res)
    project_leg(args, geom, mesh, mf, modes, timed, res)
    if args.project_only:
        return finish(args, res)
    power_leg(args, geom, mf, modes, timed, res)
    img, dt = timed(lambda: mf.sample_grid(modes, args.grid, args.grid))
    out_bytes = 3 * len(modes) * args.grid * args.grid * 8
    res["sample_grid"] = {"nx": args.grid, "wall_ms": dt * 1e3, "output_bytes": out_bytes,
                          "inside": float((img["element"] >= 0).mean())}
    dl1 = mf1.sym.array("doflocs").reshape(2, mf1.N)[:, mf1.sym.array("interior")]
    s = mf.sample(modes, dl1, hz=False)
    fine_modes = [{"Ex_dofs": s["Hx"][i], "Ey_dofs": s["Hy"][i]} for i in range(len(modes))]
    O, dt = timed(lambda: mode_overlap(modes, mf, fine_modes, mf1))
    nq = 6 * fine.t.shape[1]
    res["overlap"] = {"nq": nq, "wall_ms": dt * 1e3, "flop": 2.0 * 2 * nq * len(modes) ** 2,
                      "max_abs_offdiag": float(np.abs(O - np.diag(np.diag(O))).max()), "diag_min": float(np.diag(O).min())}
    if args.emulation:
        from fields_emulation import Emulation, overlap
        em = Emulation(mesh.p, mesh.t)
        em1 = Emulation(fine.p, fine.t)
        vals = np.stack([np.array([m["Ex_dofs"] for m in modes]), np.array([m["Ey_dofs"] for m in modes])])
        beta = np.array([m["beta"] for m in modes])
        x = np.linspace(mf.bbox[0], mf.bbox[1], args.grid)
        y = np.linspace(mf.bbox[2], mf.bbox[3], args.grid)
        pts = np.vstack([np.tile(x, args.grid), np.repeat(y, args.grid)])
        t0 = time.perf_counter()
        ref, _ = em.sample(vals, pts, True, beta=beta)
        res["emulation_sample_grid_s"] = time.perf_counter() - t0
        for c, nm in enumerate(("Hx", "Hy")):
            res[f"emulation_max_diff_{nm}"] = float(np.abs(ref[c] - img[nm].reshape(len(modes), -1)).max() / np.abs(ref[c]).max())
        vf = np.stack([s["Hx"], s["Hy"]])
        t0 = time.perf_counter()
        Oe = overlap(em, vals, em1, vf, True)
        res["emulation_overlap_s"] = time.perf_counter() - t0
        res["emulation_overlap_rel_diff"] = float(np.abs(Oe - O).max() / np.abs(O).max())
    finish(args, res)


def project_factors(geom, n):
    """The factor tables of one projection grid: n = 1 a w = 1.5 um beam on the central core, else n x n plane waves up to k0."""
    if n == 1:
        return np.array([[0.0, 1.0 / 1.5 ** 2, 0.0]]), np.array([[0.0, 1.0 / 1.5 ** 2, 0.0]])
    kap = np.linspace(-geom.k0, geom.k0, n)
    fac = np.stack([np.zeros(n), np.zeros(n), kap], 1)
    return fac, fac


def project_leg(args, geom, mesh, mf, modes, timed, res):
    """``ModeFields.project`` per grid: wall time, and the 8 ncomp k la lb Q real multiply-adds counted as flop."""
    nq = 16 * mesh.t.shape[1]
    res["project"] = {}
    for n in (int(v) for v in args.project_grids.split(",")):
        xf, yf = project_factors(geom, n)
        P, dt = timed(lambda: mf.project(modes, xf, yf))
        entry = {"wall_ms": dt * 1e3, "flop": 8.0 * 2 * len(modes) * n * n * nq, "nq": nq, "max_abs": float(np.abs(P).max())}
        if args.emulation and n <= args.emulation_grid:
            from projection_emulation import ProjectionEmulation
            em = ProjectionEmulation(mesh.p, mesh.t)
            vals = np.stack([np.array([m["Ex_dofs"] for m in modes]), np.array([m["Ey_dofs"] for m in modes])])
            t0 = time.perf_counter()
            ref = em.project(vals, True, xf, yf)
            entry["emulation_s"] = time.perf_counter() - t0
            entry["emulation_excess"] = float((np.abs(P - ref) / em.tolerance(vals, True, xf, yf)).max())
        res["project"][f"{n}x{n}"] = entry


def power_leg(args, geom, mf, modes, timed, res):
    """``ModeFields.flux_grams`` under the three material instances next to ``ModeFields.profile_grams``, and
    ``ModeFields.sample_grid_e`` next to ``ModeFields.sample_grid``: wall times (staging and copies included)."""
    from pl_fem_vectoriel_amd import IndexProfile, ProfiledGeometry, power_quantities_from_grams

    def layers(prof):
        for (cx, cy), r in zip(np.atleast_2d(geom.positions), np.asarray(geom.core_radii).reshape(-1)):
            prof.disc((cx, cy), r, geom.n_core)
        return ProfiledGeometry(geom, prof, n_core=geom.n_core, n_clad=geom.n_clad)

    x0, x1, y0, y1 = mf.bbox
    x, y = np.linspace(x0, x1, 257), np.linspace(y0, y1, 257)
    geoms = {"discs": geom, "layers": layers(IndexProfile(geom.n_clad)),
             "map": layers(IndexProfile(geom.n_clad).sampled(x, y, np.full((257, 257), float(geom.n_clad))))}
    res["power"] = {"layers": len(geoms["layers"].index_profile)}
    for name, g in geoms.items():
        G, dt = timed(lambda: mf.flux_grams(modes, g))
        q = power_quantities_from_grams(G, np.array([m["beta"] for m in modes]), float(geom.k0))
        entry = {"flux_grams_wall_ms": dt * 1e3, "orthogonality_max": float(q["orthogonality"].max()),
                 "core_fraction_min": float(q["core_fraction"].min()), "core_fraction_max": float(q["core_fraction"].max())}
        if name != "discs":
            _, dt = timed(lambda: mf.profile_grams(modes, g))
            entry["profile_grams_wall_ms"] = dt * 1e3
        res["power"][name] = entry
    _, dt = timed(lambda: mf.sample_grid(modes, args.grid, args.grid))
    res["power"]["sample_grid_wall_ms"] = dt * 1e3
    img, dt = timed(lambda: mf.sample_grid_e(modes, args.grid, args.grid, geom))
    res["power"]["sample_grid_e_wall_ms"] = dt * 1e3
    res["power"]["output_bytes"] = 4 * len(modes) * args.grid * args.grid * 8
    res["power"]["finite"] = bool(all(np.all(np.isfinite(img[nm])) for nm in ("Ex", "Ey", "Ez_im", "Sz")))


def finish(args, res):
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
