"""Host checks of the references of tests/lanczos_emulation.py (no GPU): the start field's jump-ahead equals the sequential
LCG, the extended-precision CholQR reproduces G and its inverse, the front-order permutation round-trips, and the mutation
margins the GPU tests assert hold for the shapes they use.  Then the conditions the driver tests
(test_gpu_lanczos_drivers.py) rest on, shown on the float64 restatement of the drivers (le.lanczos_reference) and the
oracle's pencils of the same meshes: their stop points do not converge, their tight bases do after at least two restarts,
the triple mesh repeats every eigenvalue three times, and each planted driver mistake moves a quantity those tests assert
at least 100 times past its tolerance."""
import numpy as np
import pytest

import lanczos_emulation as le
from lanczos_cases import P, host_case
from oracle.compare import column_errors


def test_jump_ahead_equals_the_sequential_lcg():
    seq = le.lcg_sequence(3000)
    assert all(le.lcg_jump(e) == int(seq[e]) for e in range(3000))
    # far into the stream (the C1 start block has ~4 x 2 x 90 000 elements): jump(a + b) from the state after a + 1 steps
    s = int(seq[-1])
    for _ in range(1000):
        s = (le.LCG_A * s + le.LCG_C) & ((1 << 64) - 1)
    assert le.lcg_jump(3999) == s
    v = le.lcg_values(seq)
    assert v.min() >= -1.0 and v.max() < 1.0 and abs(v.mean()) < 0.05


@pytest.mark.parametrize("cond", [1e1, 1e6, 1e12])
def test_longdouble_cholqr_reproduces_g(cond):
    rng = np.random.default_rng(int(np.log10(cond)))
    G = le.spd_matrix(rng, le.BLOCK_P, cond)
    R = le.cholesky_upper(G)
    X = le.upper_inverse(R)
    assert np.array_equal(np.asarray(R, np.float64), np.triu(np.asarray(R, np.float64)))
    assert (np.diag(np.asarray(R, np.float64)) > 0).all()
    gb, ib = le.chol_bounds(np.asarray(R, np.float64), np.asarray(X, np.float64))
    assert le.within(np.asarray(R.T @ R, np.float64), le.L(G), gb) <= 1.0
    assert le.within(np.asarray(X @ R, np.float64), le.L(np.eye(le.BLOCK_P)), ib) <= 1.0
    # an antisymmetric part is ignored, as k_chol_small symmetrises
    E = rng.standard_normal(G.shape)
    R2 = np.asarray(le.cholesky_upper(G + 1e-3 * (E - E.T)), np.float64)      # (the sum rounds: u |G| more)
    assert le.within(R2.T @ R2, le.L(G), gb + 2 * le.U * np.abs(G)) <= 1.0


@pytest.mark.parametrize("nchunks", [1, 7, 449, 2833])
def test_split_partials_sum_to_g(nchunks):
    rng = np.random.default_rng(nchunks)
    G = le.spd_matrix(rng, le.BLOCK_P, 1e12)
    parts = le.split_partials(G, nchunks, rng)
    S = np.asarray(le.partials_sum(parts), np.float64)
    assert np.abs(S - G).max() <= 64 * le.U * np.abs(G).max()
    assert np.linalg.eigvalsh((S + S.T) / 2).min() > 0


def test_interleave_and_front_order_round_trip():
    class Sym:                 # two fronts of 3 padded nodes; node 1 Dirichlet
        N, dofs_per_node = 4, 2

        def array(self, name):
            return {"npos": np.array([0, -1, 6, 8], np.int32), "fnode_ptr": np.array([0, 3, 6])}[name]
    f = le.FrontOrder(Sym())
    X = np.arange(32, dtype=np.float64).reshape(8, 4) + 1
    xl = f.permute_in(X, fill=np.nan)
    Y = f.permute_out(xl)
    live = np.array([1, 0, 1, 1] * 2, bool)
    assert np.array_equal(Y[live], X[live]) and not Y[~live].any()
    assert f.addressed().sum() == 6 * 4 and np.isnan(xl[~f.addressed()]).all()
    assert np.array_equal(le.deinterleave(le.interleave(X, 4, 2), 4, 2, 4), X)
    assert le.interleave(X, 4, 2)[4:8].tolist() == X[4].tolist()        # node 0, component 1 = row N + 0


@pytest.mark.parametrize("n2,ncols,P", [(1089, 1, 4), (1089, 17, 4), (2178, 164, 4), (261121, 5, 1), (181278, 69, 4)])
def test_mutation_margins_of_the_panel_products(n2, ncols, P):
    """The tail row, the last chunk, a column shift and a transposition move h and W - Pm h far past their bounds."""
    rng = np.random.default_rng(ncols)
    Pm = rng.uniform(0.5, 1.5, (n2, ncols)) * rng.choice((-1.0, 1.0), (n2, ncols))
    W = rng.uniform(0.5, 1.5, (n2, P)) * rng.choice((-1.0, 1.0), (n2, P))
    h, hb = le.panel_dot(Pm, W)
    m = le.assert_margins(h, hb, le.panel_dot_mutants(Pm, W, h))
    assert "tail_row_dropped" in m and "last_chunk_twice" in m
    hf = np.asarray(h, np.float64)
    w, wb = le.panel_axpy(W, Pm, hf)
    le.assert_margins(w, wb, le.panel_axpy_mutants(W, Pm, hf))


@pytest.mark.parametrize("m,p", [(1, 1), (5, 17), (137, 49), (324, 320)])
def test_mutation_margins_of_the_rotation(m, p):
    rng = np.random.default_rng(m)
    V = rng.uniform(0.5, 1.5, (300, m)) * rng.choice((-1.0, 1.0), (300, m))
    S = rng.uniform(-1, 1, (m, p))
    ref, bnd = le.rotate(V, S)
    le.assert_margins(ref, bnd, le.rotate_mutants(V, S, ref))


def test_mutation_margins_of_block_scale_and_cholqr():
    rng = np.random.default_rng(1)
    W = rng.uniform(0.5, 1.5, (1089, 4))
    R = np.triu(rng.uniform(0.5, 1.5, (4, 4))) + np.eye(4)
    X = np.asarray(le.upper_inverse(R), np.float64)
    ref, bnd = le.block_scale(W, X)
    le.assert_margins(ref, bnd, le.block_scale_mutants(W, X, ref))
    G = le.spd_matrix(rng, 4, 1e12)
    parts = le.split_partials(G, 2833, rng)
    Rg = le.cholesky_upper(le.partials_sum(parts))
    gb, _ = le.chol_bounds(np.asarray(Rg, np.float64), np.asarray(le.upper_inverse(Rg), np.float64))
    gb = gb + le.GAMMA * le.U * np.abs(parts).sum(axis=1).reshape(4, 4)
    last = parts[:, -1].reshape(4, 4)
    le.assert_margins(le.partials_sum(parts), gb, {"last_chunk_twice": ("delta", (last + last.T) / 2)})
    # a mistake below the tolerance is reported as such
    with pytest.raises(AssertionError):
        le.assert_margins(ref, bnd, {"rounding": ("delta", bnd * 2)})


# ---- the drivers across restarts: what test_gpu_lanczos_drivers.py rests on --------------------------------------------
TOL = 1e-10
# (P, k, ncv, maxiters, floor of the largest relative residual at the stop): the stop points of the GPU tests
STOPS = [(P, 24, 48, (1, 2), 4e-5), (P, 20, 48, (1,), 1e-5), (1, 30, 48, (1, 2), 2e-5)]
TIGHT = [(P, 12, 28), (P, 4, 16), (P, 13, 26), (P, 12, 24), (1, 12, 28), (1, 13, 26), (1, 12, 14), (1, 3, 8)]


def run(hc, Pd, k, ncv, maxiter, seed=None, mistake=None, max_ncv=None):
    return le.lanczos_reference(Pd, hc.op, k, ncv, TOL, maxiter, hc.start_block(Pd, seed), mistake=mistake, max_ncv=max_ncv)


@pytest.mark.parametrize("name", ["sca16", "vec16"])
def test_stop_points_do_not_converge(name):
    """The (k, ncv, maxiter) at which the GPU tests read the state back stop unconverged by a wide margin (at least six
    wanted pairs open, the largest residual 1e5 tol and more) for the drivers' own start block and two random ones, after
    exactly maxiter restarts; the block cases restart at a column that is no multiple of BLOCK_P, (20, 48) at an odd one."""
    hc = host_case(name)
    for Pd, k, ncv, maxiters, floor in STOPS:
        for mi in maxiters:
            for seed in (None, 1, 2):
                r = run(hc, Pd, k, ncv, mi, seed)
                assert r["restarts"] == mi and len(r["pks"]) == mi
                assert r["nconv"] <= k - 6 and r["max_rel_res"] >= floor, (Pd, k, ncv, mi, seed, r["nconv"], r["max_rel_res"])
                assert all(k <= pk <= r["m"] - 2 * Pd for pk in r["pks"])
                st = le.restart_state(r["V"], r["Hcols"], Pd, k, r["m"], hc.op, r["BV"])
                assert st["pk"] == r["pks"][-1] and st["mm"] == r["mm"] and not st["structure"], st
                tol = le.state_tolerances(st)
                # float64 shows nothing near the first-cycle numbers, except in the rotated B V (see le.restart_state)
                assert all(tol[q] == le.FIRST_CYCLE_TOL[q] for q in le.STATE_KEYS if q != "bv_kept"), tol
                assert tol["bv_kept"] <= 100.0, tol
        if Pd == P:
            pk = run(hc, Pd, k, ncv, 1)["pks"][0]
            assert pk % P != 0 and (k != 20 or pk % 2 == 1), (k, pk)
    if name == "sca16":
        assert hc.n2 % 2 == 1                               # an odd column of an odd n2: an address 8 bytes off 16


def check_against_dense(hc, r, k, cut_ok=True):
    """The assertions of the GPU tests on a converged run of the restatement; returns the wanted reference values."""
    lam_ref, X_ref, _ = hc.dense
    th_ref = 1.0 / (lam_ref[:k] - hc.sigma)
    o = np.argsort(lam_ref[:k])
    th = 1.0 / (r["lam"] - hc.sigma)
    assert (np.diff(r["lam"]) >= 0).all()
    assert (np.abs(th - th_ref[o]) <= le.theta_bound(th_ref, TOL)[o]).all(), np.abs(th / th_ref[o] - 1).max()
    X = r["X"]
    assert np.abs(X.T @ (hc.B @ X) - np.eye(k)).max() < 1e-10
    lam_all = np.sort(lam_ref)
    lo = le.wanted_interval(lam_all, lam_ref[:k][o])
    keep = le.whole_clusters(lam_all, lo, lo + k, 1e-4)
    if keep.any():
        assert column_errors(X[hc.live][:, keep], X_ref[hc.live][:, :k][:, o][:, keep], lam_ref[:k][o][keep], 1e-4).max() < 1e-6
    return lam_ref[:k][o]


@pytest.mark.parametrize("name", ["sca16", "vec16"])
def test_tight_bases_converge_after_restarts(name):
    """The (k, ncv) of the many-restart GPU tests converge in the restatement after at least two restarts, on the k values
    of the dense reference nearest sigma within the bound those tests use; ncv = k + 1 converges with the restart that
    never keeps fewer than min(k, mm - P) columns, and never with the one that keeps k - 1."""
    hc = host_case(name)
    for Pd, k, ncv in TIGHT:
        r = run(hc, Pd, k, ncv, 12000)
        assert r["nconv"] == k and r["restarts"] >= 2, (Pd, k, ncv, r["nconv"], r["restarts"])
        check_against_dense(hc, r, k)
    if name == "sca16":
        r = run(hc, 1, 5, 6, 2000)
        assert r["nconv"] == 5 and 2 <= r["restarts"] <= 200, r["restarts"]
        assert set(r["pks"]) == {5}
        check_against_dense(hc, r, 5)
        bad = run(hc, 1, 5, 6, 300, mistake="keep_k_minus_1")          # the rule before the fix: pk = mm - 2 P = k - 1
        assert bad["nconv"] < 5 and bad["restarts"] == 300 and set(bad["pks"]) == {4}
        # max_ncv = 65: ncv = 65 rounds down to the 64 columns ncv = 63 rounds up to
        a, b = run(hc, P, 12, 65, 12000, max_ncv=65), run(hc, P, 12, 63, 12000, max_ncv=65)
        assert a["m"] == b["m"] == 64 and np.array_equal(a["lam"], b["lam"])
        check_against_dense(hc, a, 12)


def true_residual(hc, r):
    """max || A x - lambda B x || / || A x || over the returned pairs, on the live rows."""
    X = r["X"][hc.live]
    AX = hc.A[hc.live][:, hc.live] @ X
    R = AX - (hc.B[hc.live][:, hc.live] @ X) * r["lam"]
    return (np.linalg.norm(R, axis=0) / np.linalg.norm(AX, axis=0)).max()


@pytest.mark.parametrize("name,tight", [("sca16", [(P, 4, 16), (1, 5, 6), (1, 12, 14), (P, 12, 28)]),
                                        ("vec16", [(P, 4, 16), (1, 12, 14)])])
def test_purified_vectors_meet_the_residual_bound(name, tight):
    """The residual of the pencil relative to || A x ||, which the GPU tests hold below 1e-8: the plain Ritz vectors of the
    scalar square miss it at (4, 16) and (5, 6), where the last pair to converge has |lambda| << |sigma| (7.7e-8 and 3.2e-8);
    purified as ThickRestart::finish purifies them, every case is at least ten times below the bound, and as B-orthonormal
    as before."""
    hc = host_case(name)
    for Pd, k, ncv in tight:
        r = run(hc, Pd, k, ncv, 12000)
        assert r["nconv"] == k
        res = true_residual(hc, r)
        assert res < 1e-9, (Pd, k, ncv, res)
        assert np.abs(r["X"].T @ (hc.B @ r["X"]) - np.eye(k)).max() < 1e-12
        if name == "sca16" and ncv in (16, 6):
            plain = le.lanczos_reference(Pd, hc.op, k, ncv, TOL, 12000, hc.start_block(Pd), purify=False)
            assert true_residual(hc, plain) > 1e-8


@pytest.mark.parametrize("name", ["sca16x3", "vec16x3"])
def test_triple_mesh_repeats_every_eigenvalue(name):
    """Three copies of the 16-square in one mesh pass the analysis with one and two unknowns per node; the pencil is block
    diagonal (three components) and every eigenvalue near sigma has three copies within 1e-9 relative; the block
    restatement returns all three copies of every wanted triplet."""
    import scipy.sparse.linalg as spla
    from scipy.sparse.csgraph import connected_components
    hc = host_case(name)
    one = host_case(name[:-2])
    assert hc.sym.N == 3 * one.sym.N and hc.sym.nsolve == 3 * one.sym.nsolve
    live = np.nonzero(hc.live)[0]
    Al, Bl = hc.A[live][:, live], hc.B[live][:, live]
    ncomp, lab = connected_components(abs(Al) + abs(Bl), directed=False)
    assert ncomp == 3 and (np.bincount(lab) == live.size // 3).all()
    w = []
    for cpt in range(3):
        idx = np.nonzero(lab == cpt)[0]
        wc = spla.eigsh(Al[idx][:, idx], k=24, M=Bl[idx][:, idx], sigma=hc.sigma, which="LM", tol=1e-13)[0]
        w.append(np.sort(wc))
    w = np.array(w)
    split = np.abs(w - w[0]).max(axis=0) / np.abs(w[0])
    assert split.max() <= 1e-9, split.max()
    gaps = np.abs(np.diff(w[0])) / np.abs(w[0][1:])
    assert gaps.min() > 100 * split.max()                   # triplets, not a continuum
    for k, ncv in ((12, 28), (13, 26), (20, 48)):
        r = run(hc, P, k, ncv, 12000)
        assert r["nconv"] == k and r["restarts"] >= 2
        near = np.sort(np.abs(1.0 / (w.ravel() - hc.sigma)))[::-1][:k]
        th = np.sort(np.abs(1.0 / (r["lam"] - hc.sigma)))[::-1]
        assert (np.abs(th - near) <= le.theta_bound(near, TOL) + 1e-9 * near).all()     # (eigsh's own 1e-13 and the split)
    # the single-vector restatement converges on true eigenvalues, none more often than three times
    r = run(hc, 1, 12, 28, 12000)
    assert r["nconv"] == 12
    ref_th = 1.0 / (w.ravel() - hc.sigma)
    th = 1.0 / (r["lam"] - hc.sigma)
    d = np.abs(th[:, None] - ref_th[None, :])
    assert (d.min(axis=1) <= le.theta_bound(ref_th, TOL)[d.argmin(axis=1)] + 1e-9 * np.abs(th)).all()


@pytest.mark.parametrize("name", ["sca16", "vec16"])
@pytest.mark.parametrize("Pd,k,ncv", [(P, 24, 48), (1, 30, 48)])
def test_planted_driver_mistakes_exceed_the_state_tolerances(name, Pd, k, ncv):
    """Each mistake of le.MISTAKES, planted in the restatement, moves at least one quantity the GPU tests assert on the state
    after a restart (maxiter 1 or 2) at least MARGIN times past the tolerance they allow."""
    hc = host_case(name)
    states = {}
    for mi in (1, 2):
        r = run(hc, Pd, k, ncv, mi)
        states[mi] = le.restart_state(r["V"], r["Hcols"], Pd, k, r["m"], hc.op, r["BV"])
    ref = np.concatenate([le.state_vector(states[mi]) for mi in (1, 2)])
    bound = np.concatenate([[le.state_tolerances(states[mi])[q] for q in le.STATE_KEYS] + [0.0] for mi in (1, 2)])
    assert le.within(ref, le.L(np.zeros_like(ref)), bound) <= 1.0 / le.STATE_FACTOR       # the restatement itself passes
    mutants = {}
    for mistake in le.MISTAKES:
        v = []
        for mi in (1, 2):
            r = run(hc, Pd, k, ncv, mi, mistake=mistake)
            v.append(le.state_vector(le.restart_state(r["V"], r["Hcols"], Pd, k, r["m"], hc.op, r["BV"])))
        mutants[mistake] = np.concatenate(v)
    m = le.assert_margins(le.L(ref), bound, mutants)
    assert set(m) == set(le.MISTAKES)
