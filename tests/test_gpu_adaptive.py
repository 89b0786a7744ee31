"""The adaptive loop end to end on the GPU (pl_fem_vectoriel_amd.adapt: solve, plfem_mode_indicators, Doerfler marking,
plfem_mesh_refine_marked).

Scalar: one parabolic graded core (radius 3 um, n 1.535 -> 1.0, centre (0.3, -0.2), lambda = 1.55 um) on a jittered
12 x 12 square mesh of [-8, 8]^2 um, three modes, against the same solver on the level-4 uniform mesh.  From the level-0
mesh with theta = 0.5 and the DOF budget of uniform level 1 (2 401), the adaptive mesh must give each of the three sorted
eigenvalues at least as well as uniform level 2 (9 409 DOFs), and error / indicator total of the fundamental mode must
stay within a factor 2 over the uniform levels 0-2 and every adaptive step.  A CPU prototype on the oracle measured
margins of 3x to 9x for the first and a factor 1.4 for the second.

Vectorial: two adaptive steps at C1 level 0.  Every refined mesh must solve and return the same number of modes, with
finite, positive indicators; the totals and the drift of n_eff are printed, not asserted: nobody has measured them."""
import time

import numpy as np
import pytest

from pl_fem_vectoriel_amd import (IndexProfile, PhotonicLanternGeometry, ProfiledGeometry, TriMesh, adaptive_solve,
                                  generate_mesh, mode_error_indicators)
from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver

pytestmark = pytest.mark.gpu
CENTRE, RADIUS = (0.3, -0.2), 3.0


def start_mesh(n=12, half=8.0, jitter=0.2, seed=1):
    g = np.linspace(-half, half, n + 1)
    X, Y = np.meshgrid(g, g)
    p = np.vstack([X.ravel(), Y.ravel()])
    inner = (np.abs(p[0]) < half - 1e-9) & (np.abs(p[1]) < half - 1e-9)
    p[:, inner] += np.random.default_rng(seed).uniform(-jitter, jitter, (2, int(inner.sum()))) * (2 * half / n)
    idx = np.arange((n + 1) ** 2).reshape(n + 1, n + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    return TriMesh(p, np.hstack([np.vstack([a, b, d]), np.vstack([a, d, c])]))


def graded_geometry():
    base = PhotonicLanternGeometry(1, "single", np.array([CENTRE]), np.array([RADIUS]), 1.535, 1.0, wavelength=1.55,
                                   use_complex_pml=False)
    return ProfiledGeometry(base, IndexProfile(1.0).graded(CENTRE, RADIUS, 1.535, 1.0, 2.0), n_core=1.535, n_clad=1.0)


def eigenvalues(modes, k0):
    """The three sorted pencil eigenvalues -beta^2 of the records with the largest n_eff."""
    assert len(modes) >= 3
    return -(k0 * np.array([m["n_eff"] for m in modes[:3]])) ** 2


def test_scalar_adaptive_path_beats_uniform_refinement(gpu_device, built_library):
    geo = graded_geometry()
    solver = ScalarHelmholtzSolver(geo, device=gpu_device)
    m0 = start_mesh()
    ref = eigenvalues(solver.solve(m0.refined(4), 3), geo.k0)
    ratios, uniform_err = [], None
    for level in range(3):
        mesh = m0.refined(level)
        modes = solver.solve(mesh, 3)
        _, totals = mode_error_indicators(modes[:3], mesh, geo)
        err = np.abs(eigenvalues(modes, geo.k0) - ref)
        ratios.append(err[0] / totals[0])
        uniform_err = err
        print(f"uniform level {level}: N = {solver.last_stats['N']}, |lambda - ref| = {err}, totals = {totals}, "
              f"error / total = {ratios[-1]:.4f}")
    assert solver.last_stats["N"] == 9409
    budget = 2401                                                # N of uniform level 1
    t0 = time.perf_counter()
    modes, mesh, history = adaptive_solve(solver, m0, 3, n_track=3, theta=0.5, max_dofs=budget, max_steps=40)
    wall = time.perf_counter() - t0
    solver.clear_cache()
    assert history[0]["N"] == 625 and history[-1]["mesh"] is mesh and len(history) >= 3
    assert all(a["N"] < b["N"] for a, b in zip(history, history[1:])) and history[-1]["N"] <= budget
    for h in history:
        err = np.abs(-(geo.k0 * h["n_eff"][:3]) ** 2 - ref)
        assert h["totals"].shape == (3,) and np.all(np.isfinite(h["totals"])) and np.all(h["totals"] > 0)
        ratios.append(err[0] / h["totals"][0])
        print(f"adaptive: N = {h['N']}, ne = {h['ne']}, |lambda - ref| = {err}, totals = {h['totals']}, "
              f"error / total = {ratios[-1]:.4f}, solve {1e3 * h['t_solve']:.1f} ms, indicators {1e3 * h['t_indicators']:.1f} ms")
    err = np.abs(eigenvalues(modes, geo.k0) - ref)
    print(f"adaptive run: {len(history)} solves, {wall:.2f} s, final N = {history[-1]['N']}; errors {err} against uniform "
          f"level 2 {uniform_err}: margins {uniform_err / err}")
    print(f"error / total of the fundamental: {min(ratios):.4f} .. {max(ratios):.4f}, factor {max(ratios) / min(ratios):.2f}")
    assert np.all(err <= uniform_err)
    assert max(ratios) <= 2.0 * min(ratios)


def test_vectorial_adaptive_steps_solve(gpu_device, built_library, c1_geometry):
    mesh = generate_mesh(c1_geometry, 1.0, 0)
    assert mesh.t.shape[1] == 11313
    solver = TrueVectorialMaxwellSolver(c1_geometry, device=gpu_device)
    modes, final, history = adaptive_solve(solver, mesh, 6, theta=0.5, max_dofs=10 ** 7, max_steps=3)
    assert len(history) == 3 and history[0]["ne"] == 11313 and final is history[-1]["mesh"]
    assert history[0]["ne"] < history[1]["ne"] < history[2]["ne"]
    n = len(history[0]["n_eff"])
    assert n > 0
    for h in history:
        assert len(h["n_eff"]) == n == len(h["totals"])
        assert np.all(np.isfinite(h["totals"])) and np.all(h["totals"] > 0)
        print(f"vectorial: N = {h['N']}, ne = {h['ne']}, totals = {h['totals']}, "
              f"n_eff drift from step 0 = {np.abs(h['n_eff'] - history[0]['n_eff']).max():.2e}")
    eta2, totals = mode_error_indicators(modes, final, c1_geometry, alpha_p=solver.ALPHA_P)
    solver.clear_cache()
    assert eta2.shape == (n, final.t.shape[1]) and np.all(np.isfinite(eta2)) and np.all(eta2 > 0)
    assert np.array_equal(totals, history[-1]["totals"])
