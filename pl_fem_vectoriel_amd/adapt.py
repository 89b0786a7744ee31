"""Adaptive meshes: error indicators for solved modes, Doerfler marking, marked refinement and the loop that drives them.

Accuracy used to be bought with ``TriMesh.refined()`` alone, a uniform refinement that quadruples the elements
everywhere.  Here one more reduction over the mesh with the solved modes says where the mesh limits the eigenvalues
(:func:`mode_error_indicators`: ``plfem_mode_indicators`` on the GPU, element residual plus flux jumps of the pencil the
mode was solved with), :func:`mark_elements` picks the elements that carry a fraction ``theta`` of it,
:func:`refine_marked` bisects them (longest-edge bisection with a conformity closure, ``plfem_mesh_refine_marked`` on the
host) and :func:`adaptive_solve` repeats solve -> indicators -> mark -> refine up to a budget of DOFs.  Both solvers
accept any conforming :class:`.mesh.TriMesh`, so nothing else changes.

Left out on purpose: coarsening, snapping new vertices to core rims, start vectors prolongated from the previous mesh.
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .fields import ModeFields
from .mesh import TriMesh


def mode_error_indicators(modes: Sequence[Dict], mesh, geometry, alpha_p: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
    """``(eta2 (k, ne), total (k,))``: the error indicator of every mode on every element of ``mesh`` and its sum per mode
    (:meth:`.fields.ModeFields.indicators`).  ``mesh`` may be a :class:`.fields.ModeFields`, whose locator is reused."""
    f = mesh if isinstance(mesh, ModeFields) else ModeFields(mesh)
    try:
        res = f.indicators(modes, geometry, alpha_p=alpha_p)
    finally:
        if f is not mesh:
            f.close()
    return res["eta2"], res["total"]


def mark_elements(eta2, theta: float = 0.5) -> np.ndarray:
    """Doerfler marking, (ne,) bool: with the combined indicator ``c = sum over the modes of eta2[m] / eta2[m].sum()`` (a
    mode whose total is 0 adds nothing), the elements of the smallest prefix of the stable descending order of ``c`` whose
    sum reaches ``theta`` of ``c.sum()``.  ``eta2`` is (k, ne) or, for one mode, (ne,); 0 < theta <= 1."""
    try:
        e = np.asarray(eta2, dtype=np.float64)
        theta = float(theta)
    except (TypeError, ValueError):
        raise ValueError("eta2 must be an array (k, ne) of numbers and theta a number") from None
    if e.ndim == 1:
        e = e[None]
    if e.ndim != 2 or not np.all(np.isfinite(e)) or np.any(e < 0):
        raise ValueError("eta2 must be (k, ne), finite and non-negative")
    if not 0 < theta <= 1:
        raise ValueError("theta must be in (0, 1]")
    tot = e.sum(axis=1)
    live = tot > 0
    c = (e[live] / tot[live, None]).sum(axis=0)
    marked = np.zeros(e.shape[1], dtype=bool)
    if c.size == 0 or not c.sum() > 0:
        return marked
    order = np.argsort(-c, kind="stable")
    cum = np.cumsum(c[order])
    n = min(int(np.searchsorted(cum, theta * cum[-1])) + 1, c.size)
    marked[order[:n]] = True
    return marked


def refine_marked(mesh, marked) -> Tuple[TriMesh, np.ndarray]:
    """``(TriMesh, parent)``: ``mesh`` with the elements flagged in ``marked`` bisected (:meth:`.mesh.TriMesh.refined_marked`)."""
    m = mesh if isinstance(mesh, TriMesh) else TriMesh(mesh.p, mesh.t)
    return m.refined_marked(marked)


def _solve(solver, mesh, n_modes_target: int) -> List[Dict]:
    if hasattr(solver, "solve_vectorial_modes"):
        return solver.solve_vectorial_modes(mesh, n_modes_target=n_modes_target)
    return solver.solve(mesh, n_modes_target=n_modes_target)


def adaptive_solve(solver, mesh, n_modes_target: int = 20, n_track: Optional[int] = None, theta: float = 0.5,
                   max_dofs: int = 100000, max_steps: int = 20) -> Tuple[List[Dict], TriMesh, List[Dict]]:
    """Solve, estimate, mark, refine -- until the next mesh would pass ``max_dofs`` P2 nodes or ``max_steps`` solves are
    done.  ``solver`` is a :class:`.solver_fem.TrueVectorialMaxwellSolver` or :class:`.solver_fem.ScalarHelmholtzSolver`;
    every step solves for ``n_modes_target`` modes and steers with the indicators of the first ``n_track`` of them by
    n_eff (default: all that came back).  Returns ``(modes, mesh, history)``: the modes and the mesh of the last solve and
    one record per solve, ``{"N", "ne", "n_eff", "totals", "mesh", "t_solve", "t_indicators"}`` (N = P2 nodes of the mesh,
    totals = the tracked modes' indicator sums, times in seconds).  A refined mesh that would exceed the budget is not
    solved: the result is always that of a mesh within it.  The solver's per-mesh caches are cleared between steps (a
    device context holds the factors of one mesh)."""
    if max_steps < 1:
        raise ValueError("max_steps must be >= 1")
    if n_track is not None and n_track < 1:
        raise ValueError("n_track must be >= 1")
    geometry = solver.geometry
    alpha_p = float(getattr(solver, "ALPHA_P", 1.0))
    mesh = mesh if isinstance(mesh, TriMesh) else TriMesh(mesh.p, mesh.t)
    history: List[Dict] = []
    modes: List[Dict] = []
    for step in range(int(max_steps)):
        t0 = time.perf_counter()
        modes = _solve(solver, mesh, n_modes_target)
        t1 = time.perf_counter()
        N = mesh.p.shape[1] + mesh.edges()[0].shape[1]
        rec = {"N": int(N), "ne": int(mesh.t.shape[1]), "n_eff": np.array([m["n_eff"] for m in modes]), "totals": np.zeros(0),
               "mesh": mesh, "t_solve": t1 - t0, "t_indicators": 0.0}
        history.append(rec)
        tracked = modes[:len(modes) if n_track is None else int(n_track)]
        if not tracked:
            break
        eta2, totals = mode_error_indicators(tracked, mesh, geometry, alpha_p=alpha_p)
        rec["totals"] = totals
        rec["t_indicators"] = time.perf_counter() - t1
        if step + 1 == int(max_steps):
            break
        finer, _parent = refine_marked(mesh, mark_elements(eta2, theta))
        if finer.p.shape[1] + finer.edges()[0].shape[1] > max_dofs or finer.t.shape[1] == mesh.t.shape[1]:
            break
        solver.clear_cache()
        mesh = finer
    return modes, mesh, history


__all__ = ["mode_error_indicators", "mark_elements", "refine_marked", "adaptive_solve"]
