"""Host checks of the references of tests/lanczos_emulation.py (no GPU): the start field's jump-ahead equals the sequential
LCG, the extended-precision CholQR reproduces G and its inverse, the front-order permutation round-trips, and the mutation
margins the GPU tests assert hold for the shapes they use."""
import numpy as np
import pytest

import lanczos_emulation as le


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
