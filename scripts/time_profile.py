"""Timing aid of the index-profile path at C1: the assembly with a profile of ``--layers`` layers beside the step
assembly, and ``ModeFields.profile_grams`` beside ``ModeFields.grams`` for 22 vectorial and scalar modes.

    python scripts/time_profile.py [--layers 7] [--map NX NY] [--modes 22] [--reps 10] [--tangents N] [--out FILE]

``--map NX NY`` puts a sampled index map of NX x NY pixels over the bounding box of the mesh under the layers
(``IndexProfile.sampled``): the profile kernels are then their map instances (k_element_matrices<true, EpsMap>,
k_profile_grams<.., EpsMap>).

``--tangents N`` also times ``ModeFields.profile_tangent_grams`` with N tangents (the profile's unit tangents, repeated or
cut to N) and, on the same modes, ``profile_dispersion`` and ``profile_sensitivity`` with those tangents: the kernels are
k_profile_point_weights and k_weighted_grams, one launch of each per group of four columns.

Run it under ``rocprofv3 --kernel-trace --stats``, in a run of its own and once per ``--layers`` / ``--map`` (the profile
assemblies without a map are the one instance k_element_matrices<true>), for the kernel times of k_element_matrices and
of k_profile_grams next to k_mode_grams; the wall times printed here include the copies and the launches."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def c1_profile(geom, layers: int):
    """A cladding disc in air, a trench ring and a graded centre core (3 layers), then the outer cores as step discs at
    unequal indices while ``layers`` allows (4 of the 6 at the default 7; all 6 from 9 on), then thin rings round the
    outer cores up to ``layers``."""
    from pl_fem_vectoriel_amd import IndexProfile
    pos = np.atleast_2d(geom.positions)
    prof = IndexProfile(1.0).disc((0.0, 0.0), 14.0, 1.45).ring(pos[1], 1.5, 2.4, 1.44).graded(pos[0], 1.5, 1.535, 1.50, 2)
    for i, p in enumerate(pos[1:]):
        if len(prof) < layers:
            prof.disc(p, 1.5, 1.530 + 1e-3 * i)
    i = 0
    while len(prof) < layers:
        prof.ring(pos[1 + i % 6], 1.6 + 0.05 * (i // 6), 1.64 + 0.05 * (i // 6), 1.445)
        i += 1
    return prof


def add_map(prof, mesh, nx: int, ny: int):
    """A smooth index image under the layers: a super-Gaussian plateau of 1.45 in air with a slow tilt, sampled on
    nx x ny pixels over the bounding box of the mesh."""
    x = np.linspace(mesh.p[0].min(), mesh.p[0].max(), nx)
    y = np.linspace(mesh.p[1].min(), mesh.p[1].max(), ny)
    X, Y = np.meshgrid(x, y)
    return prof.sampled(x, y, 1.0 + 0.45 * np.exp(-(((X * X + Y * Y) / 196.0) ** 4)) * (1.0 + 1e-3 * X))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=7)
    ap.add_argument("--map", type=int, nargs=2, metavar=("NX", "NY"), default=None)
    ap.add_argument("--modes", type=int, default=22)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tangents", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pl_fem_vectoriel_amd import MCFGeometry, ModeFields, ProfiledGeometry, _native, generate_mesh
    from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver, _core_table

    if not torch.cuda.is_available():
        raise SystemExit("time_profile.py needs a GPU")
    geom = MCFGeometry(7, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55)
    mesh = generate_mesh(geom, 1.0, 1)
    prof = c1_profile(geom, args.layers)
    if args.map:
        add_map(prof, mesh, *args.map)
    pg = ProfiledGeometry(geom, prof)
    res = {"ne": int(mesh.t.shape[1]), "layers": len(prof), "map": args.map}

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

    ctx = _native.Context(_native.Symbolic(mesh.p, mesh.t), 0, max_ncv=65)
    cores = _core_table(geom)
    asm = lambda: ctx.assemble(cores, geom.n_core ** 2, geom.n_clad ** 2, geom.k0, 1.0)
    ctx.set_index_profile(None)
    res["assemble_step_wall_ms"] = timed(asm)
    ctx.set_index_profile(prof)
    res["assemble_profile_wall_ms"] = timed(asm)
    ctx.close()

    solver = TrueVectorialMaxwellSolver(geom, device=0)
    vec = solver.solve_vectorial_modes(mesh, args.modes)[:args.modes]
    scal = ScalarHelmholtzSolver(geom, device=0).solve(mesh, args.modes)[:args.modes]
    mf = ModeFields(mesh, device=0, solver=solver)
    for kind, modes in (("vectorial", vec), ("scalar", scal)):
        res[kind] = {"k": len(modes), "grams_wall_ms": timed(lambda: mf.grams(modes, geom)),
                     "profile_grams_wall_ms": timed(lambda: mf.profile_grams(modes, pg))}
        if args.tangents > 0:
            from pl_fem_vectoriel_amd import profile_dispersion, profile_sensitivity
            unit = prof.unit_tangents()
            tans = [unit[i % len(unit)] for i in range(args.tangents)]
            slope = prof.tangent_index(-0.012, -0.012, -0.012 if args.map else None)
            res[kind].update(tangents=len(tans),
                             tangent_grams_wall_ms=timed(lambda: mf.profile_tangent_grams(modes, pg, tans)),
                             profile_dispersion_wall_ms=timed(lambda: profile_dispersion(modes, mf, pg, dn_dlambda=slope)),
                             profile_sensitivity_wall_ms=timed(lambda: profile_sensitivity(modes, mf, pg, tangents=tans)))
    mf.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
