"""The two Lanczos drivers past their first cycle (the host logic of csrc/api_device.hip: ThickRestart::restart,
lanczos_block, lanczos_run), on the 16-square (n2 = 1089 scalar, odd; 2178 vectorial) and three copies of it in one mesh:

* the state after one and two restarts, read back at stop points that cannot converge (le.restart_state: the basis is
  B-orthonormal, B V is B times V, OP V_mm = V_{mm+P} T with the device's columns, the first block after the restart is full
  and the later ones banded), at tolerances measured on the float64 restatement of the drivers on the same pencil
  (le.lanczos_reference; tests/test_lanczos_emulation_host.py shows that each driver mistake it can plant exceeds them 100-fold);
* tight bases that restart many times, against one dense scipy.linalg.eigh of the pencil read from the context;
* every eigenvalue three times, closer together than the tolerance: the block driver returns all copies, the single-vector
  driver returns true eigenpairs but may miss copies (the limit of a one-vector Krylov space, not asserted away);
* the edges of the accepted (k, ncv): ncv = k + 1 on the single-vector driver, the block driver's dispatch boundary, a basis
  clamped by max_ncv."""
import numpy as np
import pytest

import lanczos_emulation as le
from lanczos_cases import cases  # noqa: F401  (the module-scoped fixture of the contexts)
from oracle.compare import column_errors
from pl_fem_vectoriel_amd._native import ArpackLikeNoConvergence

pytestmark = pytest.mark.gpu
P = le.BLOCK_P
TOL = 1e-10
FIELD_TOL = 1e-6      # north_star (test_gpu_parity.py)
GAP_TOL = 1e-4        # eigenvalues closer than this (relative) are compared as one subspace (test_gpu_parity._match_fields)


def maxiter_of(c):
    return 12000 if c.dpn == 2 else 6000        # the defaults of the vectorial and the scalar solver


def solve(c, monkeypatch, driver, k, ncv, maxiter, refine=0):
    """One factorisation (if the context holds none for the shift) and one driver call; driver "single" switches the block
    driver off, "auto" leaves the dispatch alone."""
    if driver == "single":
        monkeypatch.setenv("PLFEM_LANCZOS_BLOCK", "0")
    else:
        monkeypatch.delenv("PLFEM_LANCZOS_BLOCK", raising=False)
    c.ctx.set_option("refine_steps", refine)
    try:
        c.ctx.factor(c.sigma)
        return c.ctx.lanczos(k, ncv, TOL, maxiter, c.sigma)
    finally:
        c.ctx.set_option("refine_steps", 0)


# ---- the state after a restart ----------------------------------------------------------------------------------------
STATES = ([(name, "block", refine, 24, 48, mi) for name in ("sca16", "vec16") for refine in (0, 1) for mi in (1, 2)] +
          [("sca16", "block", 0, 20, 48, 1)] +
          [(name, "single", 0, 30, 48, mi) for name in ("sca16", "vec16") for mi in (1, 2)])


@pytest.mark.parametrize("name,driver,refine,k,ncv,maxiter", STATES)
def test_state_after_restarts(cases, monkeypatch, name, driver, refine, k, ncv, maxiter):
    """A stop point that cannot converge (test_stop_points_do_not_converge): the call raises after exactly maxiter restarts
    and one more full cycle, and leaves V, B V and the projected columns of that cycle.  Block: the first restart keeps 30
    (sca16) or 31 (vec16) columns, so the steps after it start off the multiples of BLOCK_P; (20, 48) keeps 27, an odd column
    of the odd n2 = 1089.  Measured on the MI355X (orth / relation / symmetry / outside the band), the worst of the cases:
    see DESIGN.md section 16."""
    c = cases(name)
    Pd = 1 if driver == "single" else P
    m = ncv if Pd == 1 else -(-ncv // P) * P
    ld = m + Pd
    with pytest.raises(ArpackLikeNoConvergence) as ei:
        solve(c, monkeypatch, driver, k, ncv, maxiter, refine)
    stats = ei.value.stats
    assert stats["restarts"] == maxiter and stats["nconv"] < k
    assert (stats["n_block_solves"] == 0) == (driver == "single")
    n2 = c.n2
    V = c.ctx.debug_copy("V", 0, n2 * ld).reshape(ld, n2).T
    BV = c.ctx.debug_copy("BV", 0, n2 * ld).reshape(ld, n2).T
    H = c.ctx.debug_copy("Hcols", 0, ld * ld).reshape(ld, ld).T
    st = le.restart_state(V, H, Pd, k, m, c.op, BV)
    # the restatement on the same pencil from the same start block: the tolerances, and the columns the first restart keeps
    ref = le.lanczos_reference(Pd, c.op, k, ncv, TOL, maxiter, le.start_field(c.sym, Pd))
    rst = le.restart_state(ref["V"], ref["Hcols"], Pd, k, ref["m"], c.op, ref["BV"])
    assert ref["restarts"] == maxiter and ref["nconv"] < k and not rst["structure"]
    tol = le.state_tolerances(rst)
    print(f"\n[state] {name} {driver} refine={refine} ({k}, {ncv}) maxiter={maxiter}: pk={st['pk']} (restatement "
          f"{ref['pks']}) mm={st['mm']} nconv={stats['nconv']} max_rel_res={stats['max_rel_res']:.2e} | " +
          " ".join(f"{q}={st[q]:.2e} (ref {rst[q]:.2e}, tol {tol[q]:.1e})" for q in le.STATE_KEYS))
    pk, mm = st["pk"], st["mm"]
    assert k <= pk <= m - 2 * Pd and mm == pk + Pd * ((m - pk) // Pd)
    assert not (H[:, :pk] != 0).any()
    assert not st["structure"], st["structure"]
    if maxiter == 1:
        assert pk == ref["pks"][0]                      # the same restart rule on the same residuals
        if driver == "block":
            assert pk % P != 0 and (k != 20 or pk % 2 == 1)
    for q in le.STATE_KEYS:
        assert st[q] <= tol[q], (q, st[q], tol[q])
    assert not BV[~c.live_rows(), :mm + Pd].any()          # Dirichlet rows of B V exactly 0


# ---- converged solves against the dense reference --------------------------------------------------------------------
def wanted_reference(c, k):
    """The k reference pairs of largest |1 / (lambda - sigma)|, ascending in lambda: (lam, X, lo, lam_all ascending), lo the
    place of the first of them in lam_all."""
    lam, X, _ = c.dense
    o = np.argsort(lam[:k])
    lam_all = np.sort(lam)
    lo = le.wanted_interval(lam_all, lam[:k][o])                      # the wanted set is an interval of the spectrum
    return lam[:k][o], X[:, :k][:, o], lo, lam_all


def check_pairs(c, evals, evecs, k):
    """B-orthonormal vectors (the bound of test_eigenpairs_match_scipy_eigsh), Dirichlet rows exactly 0."""
    V = evecs.cpu().numpy().T
    assert V.shape == (c.n2, k) and np.isfinite(V).all()
    assert not V[~c.live_rows()].any()
    assert np.abs(V.T @ (c.pencil.matrix("B") @ V) - np.eye(k)).max() < 1e-10
    return V


def check_converged(c, monkeypatch, driver, k, ncv, min_restarts=2, maxiter=None):
    """Everything the many-restart tests assert on one (k, ncv); returns the stats."""
    maxiter = maxiter or maxiter_of(c)
    evals, evecs, st = solve(c, monkeypatch, driver, k, ncv, maxiter)
    print(f"\n[converged] {c.name} {driver} ({k}, {ncv}): {st}")
    assert st["nconv"] == k and st["restarts"] >= min_restarts
    if driver == "block":
        assert st["n_block_solves"] > 0 and st["n_opinv"] == P * st["n_block_solves"]
    elif driver == "single":
        assert st["n_block_solves"] == 0
    assert (np.diff(evals) >= 0).all()
    lam, X, lo, lam_all = wanted_reference(c, k)
    th, th_ref = 1.0 / (evals - c.sigma), 1.0 / (lam - c.sigma)
    err = np.abs(th - th_ref)
    assert (err <= le.theta_bound(th_ref, TOL)).all(), (err / np.abs(th_ref)).max()
    V = check_pairs(c, evals, evecs, k)
    keep = le.whole_clusters(lam_all, lo, lo + k, GAP_TOL)          # a cluster the wanted set cuts has no subspace to compare
    live = c.live_rows()
    if keep.any():
        assert column_errors(V[live][:, keep], X[live][:, keep], lam[keep], GAP_TOL).max() < FIELD_TOL
    evals2, evecs2, st2 = solve(c, monkeypatch, driver, k, ncv, maxiter)
    assert np.array_equal(evals2, evals) and c.torch.equal(evecs2, evecs) and st2 == st, "not deterministic"
    return st


TIGHT = ([("block", k, ncv) for k, ncv in ((12, 28), (4, 16), (13, 26), (12, 24))] +
         [("single", k, ncv) for k, ncv in ((12, 28), (13, 26), (12, 14))] + [("auto", 3, 8)])


@pytest.mark.parametrize("driver,k,ncv", TIGHT)
@pytest.mark.parametrize("name", ["sca16", "vec16"])
def test_many_restarts_match_the_dense_reference(cases, monkeypatch, name, driver, k, ncv):
    """Tight bases (the restatement restarts 5 to 16 times for the block driver, 2 to 62 for the single-vector one): the k
    pairs nearest sigma of the dense reference, each Ritz value within 2 tol |theta| + 64 u max |theta|.  (3, 8) reaches the
    single-vector driver through the dispatch (k < BLOCK_P); (4, 16) is the smallest basis the block driver takes."""
    st = check_converged(cases(name), monkeypatch, driver, k, ncv)
    if driver == "auto":
        assert st["n_block_solves"] == 0


@pytest.mark.parametrize("k,ncv", [(12, 28), (13, 26), (20, 48)])
@pytest.mark.parametrize("name", ["sca16x3", "vec16x3"])
def test_block_driver_returns_every_copy_of_a_triplet(cases, monkeypatch, name, k, ncv):
    """Every eigenvalue three times with a relative splitting of 1e-15 .. 6e-11, below the tolerance: the block driver
    (BLOCK_P = 4 >= 3 copies) returns all copies; k = 13 cuts a triplet, whose subspace is left out of the field check."""
    c = cases(name)
    lam, _, ncomp = c.dense
    assert ncomp == 3
    trip = np.sort(lam[:24]).reshape(8, 3)
    assert (np.ptp(trip, axis=1) <= 1e-9 * np.abs(trip[:, 0])).all()
    check_converged(c, monkeypatch, "block", k, ncv)


@pytest.mark.parametrize("name", ["sca16x3", "vec16x3"])
def test_single_vector_driver_on_triplets_returns_true_pairs(cases, monkeypatch, name):
    """The single-vector driver does not resolve eigenvalues closer together than its tolerance (a one-vector Krylov space
    holds one direction of each cluster; ARPACK shares the limit): it may miss copies and return pairs further from sigma in
    their place.  Asserted is what holds: every returned value is a reference eigenvalue within the bound, none more often
    than its multiplicity, the pairs are true B-orthonormal eigenpairs."""
    c = cases(name)
    k, ncv = 12, 28
    evals, evecs, st = solve(c, monkeypatch, "single", k, ncv, maxiter_of(c))
    assert st["nconv"] == k and st["n_block_solves"] == 0
    assert (np.diff(evals) >= 0).all()
    lam_all = np.sort(c.dense[0])                          # ascending: the three copies of a triplet are neighbours
    assert lam_all.size % 3 == 0
    th_ref = 1.0 / (lam_all - c.sigma)
    th = 1.0 / (evals - c.sigma)
    bound = le.theta_bound(th_ref, TOL)
    hit = np.abs(th[:, None] - th_ref[None, :]) <= bound[None, :]
    assert hit.any(axis=1).all(), "a returned value is no eigenvalue of the pencil"
    first = hit.argmax(axis=1) // 3                        # the triplet of each returned value
    counts = np.bincount(first)
    print(f"\n[triplets] {name} single (12, 28): copies returned per triplet {counts.tolist()}, restarts {st['restarts']}")
    assert counts.max() <= 3
    check_pairs(c, evals, evecs, k)


# ---- the edges of (k, ncv) ----------------------------------------------------------------------------------------------
def test_single_vector_driver_converges_at_ncv_k_plus_1(cases, monkeypatch):
    """ncv = k + 1: the restart keeps all k wanted columns (never fewer than min(k, mm - P)) and the call converges on the
    reference pairs; with the clamp pk <= mm - 2 P alone it kept k - 1 and stayed at nconv = 4 for any number of restarts
    (confirmed on the MI355X at 300 restarts).  The restatement needs 63 restarts."""
    c = cases("sca16")
    st = check_converged(c, monkeypatch, "auto", 5, 6, maxiter=2000)
    assert st["n_block_solves"] == 0


@pytest.mark.parametrize("k,ncv,block", [(4, 16, True), (4, 15, True), (3, 16, False), (4, 12, False)])
def test_block_dispatch_boundary(cases, monkeypatch, k, ncv, block):
    """The block driver takes a call when k >= BLOCK_P and the rounded basis has k + 3 BLOCK_P columns: (4, 16) and (4, 15)
    (rounded up to 16) do, k = 3 and a 12-column basis do not."""
    st = check_converged(cases("vec16"), monkeypatch, "auto", k, ncv, min_restarts=0)
    assert (st["n_block_solves"] > 0) == block
    if block:
        assert st["n_opinv"] == P * st["n_block_solves"]


def test_basis_clamped_by_max_ncv(cases, monkeypatch):
    """A context with max_ncv = 65: ncv = 65 rounds down to the 64-column basis ncv = 63 rounds up to, so the two calls are
    one computation, and both return the reference pairs."""
    c = cases("sca16m65")
    assert c.ctx.max_ncv == 65
    k = 12
    a = solve(c, monkeypatch, "block", k, 65, maxiter_of(c))
    b = solve(c, monkeypatch, "block", k, 63, maxiter_of(c))
    assert np.array_equal(a[0], b[0]) and c.torch.equal(a[1], b[1]) and a[2] == b[2]
    assert a[2]["n_block_solves"] > 0
    st = check_converged(c, monkeypatch, "block", k, 65, min_restarts=0)
    assert st == a[2]
    with pytest.raises(ValueError):
        c.ctx.lanczos(k, 66, TOL, 10, c.sigma)


# ---- true residuals ----------------------------------------------------------------------------------------------------
RESIDUALS = ([(name, d, k, ncv) for name in ("sca16", "vec16") for d, k, ncv in TIGHT] +
             [(name, "block", k, ncv) for name in ("sca16x3", "vec16x3") for k, ncv in ((12, 28), (13, 26), (20, 48))] +
             [("sca16x3", "single", 12, 28), ("vec16x3", "single", 12, 28), ("sca16", "auto", 5, 6), ("vec16", "auto", 4, 15),
              ("sca16m65", "block", 12, 65), ("sca16m65", "block", 12, 63)])


@pytest.mark.parametrize("name,driver,k,ncv", RESIDUALS)
def test_true_residuals_at_the_parity_bound(cases, monkeypatch, name, driver, k, ncv):
    """Every converged call of this file: max || A v - lambda B v || / || A v || < 1e-8, the bound of
    test_eigenpairs_match_scipy_eigsh.  The bound is relative to || A v || = |lambda| || B v ||, while the drivers (like ARPACK)
    stop on the residual of OP relative to |theta| = 1 / |lambda - sigma|: at tol = 1e-10 a plain Ritz vector with
    |lambda| << |sigma| stops above it (sca16: 7.7e-8 at block (4, 16), lambda = 1.54 next to sigma = -27.7, on the MI355X and
    in the restatement; 3.2e-8 at (5, 6) in the restatement).  ThickRestart::finish therefore purifies the converged vectors
    as ARPACK does in shift-invert mode (x + V_res R_m s_last / theta = OP x / theta), which takes these two to 8.9e-10 and
    2.8e-10, in the restatement (test_purified_vectors_meet_the_residual_bound) and on the MI355X; no other case is above 2.6e-10."""
    c = cases(name)
    evals, evecs, st = solve(c, monkeypatch, driver, k, ncv, 2000 if (k, ncv) == (5, 6) else maxiter_of(c))
    assert st["nconv"] == k
    V = evecs.cpu().numpy().T
    AV = c.pencil.matrix("A") @ V
    R = AV - (c.pencil.matrix("B") @ V) * evals
    rel = np.linalg.norm(R, axis=0) / np.linalg.norm(AV, axis=0)
    i = int(rel.argmax())
    print(f"\n[residual] {name} {driver} ({k}, {ncv}): max {rel[i]:.3e} at lambda = {evals[i]:.6g} (absolute "
          f"{np.linalg.norm(R, axis=0)[i]:.2e}), max_rel_res {st['max_rel_res']:.2e}")
    assert rel.max() < 1e-8, rel.max()
