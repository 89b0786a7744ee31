"""The host side of pl_fem_vectoriel_amd.adapt: Doerfler marking, and the control flow of adaptive_solve with a solver and
an indicator that need no GPU."""
import numpy as np
import pytest

from core_ties import jittered_square_mesh
from pl_fem_vectoriel_amd import adapt, mark_elements


def test_doerfler_marking():
    eta = np.array([[1.0, 5.0, 2.0, 2.0], [0.0, 0.0, 0.0, 0.0]])          # the second mode has no error: it adds nothing
    assert mark_elements(eta, 0.5).tolist() == [False, True, False, False]
    assert mark_elements(eta, 0.51).tolist() == [False, True, True, False]  # stable: the first of the two equal ones
    assert mark_elements(eta, 1.0).tolist() == [True, True, True, True]
    assert mark_elements(eta[0], 0.7).tolist() == [False, True, True, False]
    # modes are weighed by their own totals: a mode a million times smaller marks its elements as well
    two = np.array([[4.0, 0.0, 0.0, 1.0], [0.0, 3e-6, 1e-6, 0.0]])
    assert mark_elements(two, 0.75).tolist() == [True, True, False, False]
    assert not mark_elements(np.zeros((2, 5)), 0.5).any()
    rng = np.random.default_rng(0)
    e = rng.random((3, 200))
    m = mark_elements(e, 0.5)
    c = (e / e.sum(axis=1, keepdims=True)).sum(axis=0)
    assert c[m].sum() >= 0.5 * c.sum() and c[m].min() >= c[~m].max()
    assert c[m].sum() - c[m].min() < 0.5 * c.sum()                          # the smallest such prefix
    for bad in (dict(eta2=e, theta=0.0), dict(eta2=e, theta=1.5), dict(eta2=-e, theta=0.5), dict(eta2=np.zeros((2, 2, 2)), theta=0.5),
                dict(eta2=np.array([np.nan, 1.0]), theta=0.5), dict(eta2="x", theta=0.5)):
        with pytest.raises(ValueError):
            mark_elements(**bad)


class StubSolver:
    """Counts the solves and the cache clears; returns two records whose n_eff depends on the mesh size."""
    geometry = None

    def __init__(self):
        self.solved, self.cleared = [], 0

    def solve(self, mesh, n_modes_target=20):
        self.solved.append(mesh.t.shape[1])
        return [{"n_eff": 1.5 - 1.0 / mesh.t.shape[1]}, {"n_eff": 1.4}]

    def clear_cache(self):
        self.cleared += 1


def test_adaptive_solve_control_flow(monkeypatch, built_library):
    def indicators(modes, mesh, geometry, alpha_p=1.0):
        p, t = mesh.p, mesh.t
        cx = p[0, t].mean(axis=0)
        e = np.stack([np.exp(-20 * cx) for _ in modes])          # the error sits at the left edge
        return e, e.sum(axis=1)

    monkeypatch.setattr(adapt, "mode_error_indicators", indicators)
    mesh = jittered_square_mesh(4)
    N0 = mesh.p.shape[1] + mesh.edges()[0].shape[1]
    solver = StubSolver()
    modes, final, hist = adapt.adaptive_solve(solver, mesh, 2, n_track=1, theta=0.5, max_dofs=3 * N0, max_steps=50)
    assert len(hist) >= 3 and hist[0]["N"] == N0 and hist[0]["mesh"] is mesh and hist[-1]["mesh"] is final
    assert [h["ne"] for h in hist] == solver.solved and solver.cleared == len(hist) - 1
    assert all(a["N"] < b["N"] for a, b in zip(hist, hist[1:])) and hist[-1]["N"] <= 3 * N0
    assert all(h["totals"].shape == (1,) and h["n_eff"].shape == (2,) for h in hist)
    assert modes[0]["n_eff"] == 1.5 - 1.0 / final.t.shape[1]
    # the refinement went where the indicator is
    cx = final.p[0, final.t].mean(axis=0)
    assert (cx < 0.5).sum() > 2 * (cx >= 0.5).sum()
    # the step limit
    solver = StubSolver()
    _, _, hist = adapt.adaptive_solve(solver, mesh, 2, theta=0.5, max_dofs=10 ** 9, max_steps=2)
    assert len(hist) == 2 and hist[1]["totals"].shape == (2,)
    with pytest.raises(ValueError):
        adapt.adaptive_solve(solver, mesh, 2, max_steps=0)
    with pytest.raises(ValueError):
        adapt.adaptive_solve(solver, mesh, 2, n_track=0)
