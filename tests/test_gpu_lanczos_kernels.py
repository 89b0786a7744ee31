"""The device kernels of the two Lanczos drivers, one by one on the GPU, against the extended-precision restatements of
tests/lanczos_emulation.py (test hooks plfem_debug_panel / _scale_store / _first_pass / _spmv_block / _chol /
_block_scale / _rotate / _start_field, and the ABI's plfem_postprocess / plfem_residuals), at the shapes where they go
wrong: n2 mod 1024 tails of 65, 130, 1 and 30 rows, column counts off the 16-column workgroups, m mod 4 and p mod 16 of the
rotation and its LDS chunking, k mod 4 of the per-mode kernels, and enough chunks for the unrolled partial sums.  Every
test asserts its shape property and that its inputs make each cheap kernel mistake (a tail row dropped, the last chunk
counted twice, columns shifted, coefficients transposed, ...) exceed the tolerance at least 100-fold.  A composed check
reads back the basis and the projected matrix of one Lanczos cycle of each driver form."""
import numpy as np
import pytest

import lanczos_emulation as le
from lanczos_cases import CASES, K0, cases  # noqa: F401  (cases: the module-scoped fixture of the contexts)

pytestmark = pytest.mark.gpu
P = le.BLOCK_P
GAP = 37                                                # NaN-filled gap between the columns of a block


def ok(gpu, ref, bound, what):
    assert np.isfinite(gpu).all(), f"{what}: non-finite result"
    r = le.within(gpu, ref, bound)
    assert r <= 1.0, f"{what}: {r:.3g} times the bound"


@pytest.mark.parametrize("name", CASES)
def test_panel_products_block_and_single(cases, name):
    """k_panel_dot_p + k_panel_dot_finish_p (with and without the CGS2 hacc accumulation), k_panel_axpy_p (with and without
    the interleaved wil copy) at P = BLOCK_P, and their P = 1 instances of the single-vector driver (one column per wave, the
    hacc accumulation included), at column counts off the 16-column workgroups up to max_ncv + P."""
    c = cases(name)
    n2, ldw = c.n2, c.n2 + GAP
    nmax = max(c.ncols)
    Pm_h = c.random(n2, nmax)
    W_h = c.random(n2, P)
    Pm = c.dev(Pm_h.T)                                  # column c at Pm + c n2
    href, hbnd = le.panel_dot(Pm_h, W_h)                # h of ncols columns = the first ncols rows
    for ncols in c.ncols:
        ldh = ncols + 3
        H = c.dev(np.full((P, ldh), np.nan))
        Wd = c.block(W_h, ldw)
        c.ctx.debug_panel("dot_block", ncols, Pm, Wd, ldw, H, ldh)
        Hh = c.host(H).reshape(P, ldh)
        assert np.isnan(Hh[:, ncols:]).all()
        h = Hh[:, :ncols].T
        ok(h, href[:ncols], hbnd[:ncols], f"dot_block ncols={ncols}")
        le.assert_margins(href[:ncols], hbnd[:ncols], le.panel_dot_mutants(Pm_h[:, :ncols], W_h, href[:ncols]))
        H2 = c.dev(np.full((P, ldh), np.nan))
        c.ctx.debug_panel("dot_block", ncols, Pm, Wd, ldw, H2, ldh)
        assert np.array_equal(c.host(H2), c.host(H), equal_nan=True), "panel dot not deterministic"
        # CGS2: hacc += h (same h bits into the second output)
        acc0 = c.random(ncols, P)
        ldacc = ncols + 1
        acc = c.dev(np.vstack([acc0, np.full((1, P), np.nan)]).T)
        c.ctx.debug_panel("dot_block", ncols, Pm, Wd, ldw, H2, ldh, hacc=acc, ldacc=ldacc)
        Ah = c.host(acc).reshape(P, ldacc)
        assert np.isnan(Ah[:, ncols]).all()
        assert np.array_equal(Ah[:, :ncols].T, acc0 + h), "hacc != old hacc + h"
        assert np.array_equal(c.host(H2), c.host(H), equal_nan=True)
        # W -= Pm H, with and without the interleaved copy
        wref, wbnd = le.panel_axpy(W_h, Pm_h[:, :ncols], h)
        for with_il in (False, True):
            Wd = c.block(W_h, ldw)
            wil = c.dev(np.full(n2 * P, np.nan)) if with_il else None
            c.ctx.debug_panel("axpy_block", ncols, Pm, Wd, ldw, H, ldh, wil=wil)
            Wn = c.unblock(Wd, P, ldw)
            ok(Wn, wref, wbnd, f"axpy_block ncols={ncols}")
            if with_il:
                assert np.array_equal(c.host(wil), le.interleave(Wn, c.N, c.dpn)), "wil != interleaved W"
        le.assert_margins(wref, wbnd, le.panel_axpy_mutants(W_h, Pm_h[:, :ncols], h))
        # single-vector driver: P = 1
        w1 = W_h[:, :1]
        hs = c.dev(np.full(ncols + 1, np.nan))
        wd = c.dev(w1)
        c.ctx.debug_panel("dot", ncols, Pm, wd, n2, hs, ncols)
        h1 = c.host(hs)
        assert np.isnan(h1[ncols])
        ok(h1[:ncols, None], href[:ncols, :1], hbnd[:ncols, :1], f"dot ncols={ncols}")
        le.assert_margins(href[:ncols, :1], hbnd[:ncols, :1], le.panel_dot_mutants(Pm_h[:, :ncols], w1, href[:ncols, :1]))
        c.ctx.debug_panel("axpy", ncols, Pm, wd, n2, hs, ncols)
        r1, b1 = le.panel_axpy(w1, Pm_h[:, :ncols], h1[:ncols, None])
        ok(c.host(wd)[:, None], r1, b1, f"axpy ncols={ncols}")
        le.assert_margins(r1, b1, le.panel_axpy_mutants(w1, Pm_h[:, :ncols], h1[:ncols, None]))
        # CGS2 at P = 1: acc[0:ncols] += h (same h bits into the second output)
        a0 = c.random(ncols + 1)
        ad = c.dev(a0)
        c.ctx.debug_panel("dot", ncols, Pm, c.dev(w1), n2, hs, ncols, hacc=ad, ldacc=ncols)
        ah = c.host(ad)
        assert np.array_equal(ah[:ncols], a0[:ncols] + h1[:ncols]) and ah[ncols] == a0[ncols]
        assert np.array_equal(c.host(hs), h1, equal_nan=True)


@pytest.mark.parametrize("name", CASES)
def test_fused_first_pass(cases, name):
    """k_permute_dot_first + k_axpy_first: W = the permuted front-order block (Dirichlet rows 0), Hout = BVm^T W in T, and
    the update applies exactly the Hout it stored; ncols = 1 .. 8; unaddressed front-order slots NaN."""
    c = cases(name)
    n2, ldw = c.n2, c.n2 + GAP
    nseg = -(-n2 // le.PANEL_CHUNK)
    X = c.random(n2, P)
    xl_h = c.front.permute_in(X, fill=np.nan)
    assert np.isnan(xl_h).any() or c.front.addressed().all()
    Wglob = c.front.permute_out(xl_h)                       # what W must be
    assert np.isfinite(Wglob).all()
    BVm_h, Vm_h = c.random(n2, 8, live=True), c.random(n2, 8, live=True)
    xl, BVm, Vm = c.dev(xl_h), c.dev(BVm_h.T), c.dev(Vm_h.T)
    href, hbnd = le.panel_dot(BVm_h, Wglob)
    le.assert_margins(href, hbnd, le.panel_dot_mutants(BVm_h, Wglob, href))
    for ncols in range(1, 9):
        ldh = ncols + 2
        Wd = c.block(np.full((n2, P), 7.0), ldw)
        Ho = c.dev(np.full((P, ldh), np.nan))
        c.ctx.debug_first_pass(xl, BVm, Vm, ncols, Wd, ldw, Ho, ldh)
        Hh = c.host(Ho).reshape(P, ldh)
        assert np.isnan(Hh[:, ncols:]).all()
        h = Hh[:, :ncols].T
        ok(h, href[:ncols], hbnd[:ncols], f"first pass Hout ncols={ncols}")
        Wn = c.unblock(Wd, P, ldw)
        wref, wbnd = le.panel_axpy(Wglob, Vm_h[:, :ncols], h)
        ok(Wn, wref, wbnd, f"first pass update ncols={ncols}")
        assert np.array_equal(Wn[~c.live_rows()], np.zeros(((~c.live_rows()).sum(), P)))
        le.assert_margins(wref, wbnd, le.panel_axpy_mutants(Wglob, Vm_h[:, :ncols], h))
        # the pass alone (Vm = 0) leaves exactly the permuted block
        if ncols == 8:
            Wd = c.block(np.full((n2, P), 7.0), ldw)
            c.ctx.debug_first_pass(xl, BVm, c.dev(np.zeros((8, n2))), ncols, Wd, ldw, Ho, ldh)
            assert np.array_equal(c.unblock(Wd, P, ldw), Wglob), "W != permuted d_xl"
            H2 = c.dev(np.full((P, ldh), np.nan))
            Wd = c.block(np.full((n2, P), 7.0), ldw)
            c.ctx.debug_first_pass(xl, BVm, Vm, ncols, Wd, ldw, H2, ldh)
            assert np.array_equal(c.host(H2), c.host(Ho), equal_nan=True), "first pass not deterministic"
    if name in ("sca255", "c1"):
        assert nseg > 56                                    # k_axpy_first's eight-loads loop


@pytest.mark.parametrize("name", CASES)
def test_block_spmvs_and_gram(cases, name):
    """k_spmv_b_block, k_spmv_b_block_il (with and without the Gram partials) and k_spmv_a_block against the extended-precision
    CSR products; a_block column by column against plfem_spmv("A"); the Gram partials sum to X^T (B X)."""
    c = cases(name)
    n2, ld = c.n2, c.n2 + GAP
    X = c.random(n2, P)
    Bref, Bbnd = c.pencil.apply("B", X)
    Aref, Abnd = c.pencil.apply("A", X)
    le.assert_margins(Bref, Bbnd, le.spmv_mutants(c.pencil, "B", X, Bref))
    le.assert_margins(Aref, Abnd, le.spmv_mutants(c.pencil, "A", X, Aref))
    Xd, Xil = c.block(X, ld), c.dev(le.interleave(X, c.N, c.dpn))
    Y = c.block(np.full((n2, P), np.nan), ld)
    assert c.ctx.debug_spmv_block("b_block", Xd, Y, ld) == 0
    Yb = c.unblock(Y, P, ld)
    ok(Yb, Bref, Bbnd, "b_block")
    Y = c.block(np.full((n2, P), np.nan), ld)
    c.ctx.debug_spmv_block("b_block_il", Xil, Y, ld)
    assert np.array_equal(c.unblock(Y, P, ld), Yb), "b_block_il != b_block"
    nb = -(-c.N * 8 // 256)
    gram_out = c.dev(np.full(P * P * nb, np.nan))
    Y = c.block(np.full((n2, P), np.nan), ld)
    assert c.ctx.debug_spmv_block("b_block_il_gram", Xil, Y, ld, gram_out) == nb
    assert np.array_equal(c.unblock(Y, P, ld), Yb)
    parts = c.host(gram_out).reshape(P * P, nb)
    absBX = np.vstack([c.pencil.abs_csr["Minv"] @ np.abs(X[k * c.N:(k + 1) * c.N]) for k in range(c.dpn)])
    Gref, Gbnd = le.gram(X, Bref, Bbnd, absBX)
    Gsum = le.partials_sum(parts)
    ok(np.asarray(Gsum, np.float64), Gref, Gbnd, "Gram partials")
    le.assert_margins(Gref, Gbnd, le.gram_mutants(parts, Gref))
    if name in ("sca255", "c1"):
        assert nb > 448                                     # k_chol_small's eight-loads loop
    # the CholQR reads the partials the product left (the Lanczos step's order)
    T = c.dev(np.full(P * P, np.nan))
    Rinv = c.dev(np.zeros(P * P))
    assert c.ctx.debug_chol(None, 0, True, nb, T, P, Rinv) == 0
    R = c.host(T).reshape(P, P).T
    Rref = le.cholesky_upper(Gsum)
    gb, _ = le.chol_bounds(R, le.upper_inverse(R))
    sb = le.GAMMA * le.U * np.abs(parts).sum(axis=1).reshape(P, P)      # (the kernel's own sum of the nb partials)
    ok(np.asarray(le.L(R).T @ le.L(R), np.float64), (Gsum + Gsum.T) / 2, gb + (sb + sb.T) / 2, "CholQR of the Gram partials")
    assert np.allclose(R, np.asarray(Rref, np.float64), rtol=1e-10, atol=1e-12 * np.abs(R).max())
    # A, and column by column against plfem_spmv("A")
    Y = c.block(np.full((n2, P), np.nan), ld)
    c.ctx.debug_spmv_block("a_block", Xd, Y, ld)
    Ya = c.unblock(Y, P, ld)
    ok(Ya, Aref, Abnd, "a_block")
    for q in range(P):
        y1 = c.host(c.ctx.spmv("A", c.dev(X[:, q])))
        ok(y1[:, None], Aref[:, q:q + 1], Abnd[:, q:q + 1], "plfem_spmv A")
        ok(Ya[:, q:q + 1], le.L(y1[:, None]), 2 * Abnd[:, q:q + 1], "a_block vs plfem_spmv")
    for form, xin in (("b_block", Xd), ("a_block", Xd)):
        Y2 = c.block(np.full((n2, P), np.nan), ld)
        c.ctx.debug_spmv_block(form, xin, Y2, ld)
        assert np.array_equal(c.unblock(Y2, P, ld), Yb if form == "b_block" else Ya), f"{form} not deterministic"


@pytest.mark.parametrize("cond", [1e1, 1e12])
@pytest.mark.parametrize("nchunks", [0, 1, 7, 449, 2833])
def test_cholqr_both_entry_forms(cases, cond, nchunks):
    """k_chol_small: ready-made G (nchunks = 0) or nchunks partials per entry (past the eight-loads loop at 449 and the C1
    count 2833); R^T R = G and R^-1 R = I within LAPACK-style bounds, R upper with a positive diagonal, placed at ldT in T
    with its surroundings untouched; the mutations (unsymmetrised triangle, R transposed, a chunk twice) are caught."""
    c = cases("c1")
    rng = np.random.default_rng(int(cond) % 97 + nchunks)
    G0 = le.spd_matrix(rng, P, cond) * 3.7
    E = rng.standard_normal((P, P)) * 1e-7 * np.abs(G0).max()
    G = G0 + (E - E.T)                                      # the kernel must use the symmetric part
    ldT, nc, c0 = 23, 9, 5                                  # R at T[nc:nc+P, c0:c0+P] as the driver places it (Hblk + nc)
    Tfull = np.full((ldT, 12), np.nan)
    T = c.dev(Tfull.T)
    Rinv = c.dev(np.full(P * P, np.nan))
    off = c0 * ldT + nc
    if nchunks == 0:
        Gd = c.dev(np.vstack([G, np.full((1, P), np.nan)]).T)                      # G[i + j (P + 1)], a NaN row below
        flag = c.ctx.debug_chol(Gd, P + 1, False, 0, T, ldT, Rinv, Tblk_offset=off)
        Gref = le.L(G)
        mut = {"unsymmetrised": ("delta", np.triu(E - E.T) + np.triu(E - E.T, 1).T)}
    else:
        parts = le.split_partials(G, nchunks, rng)
        flag = c.ctx.debug_chol(c.dev(parts), 0, True, nchunks, T, ldT, Rinv, Tblk_offset=off)
        Gref = le.partials_sum(parts)
        last = parts[:, -1].reshape(P, P)
        mut = {"last_chunk_twice": ("delta", (last + last.T) / 2), "unsymmetrised": ("delta", np.triu(E - E.T) + np.triu(E - E.T, 1).T)}
        sb = le.GAMMA * le.U * np.abs(parts).sum(axis=1).reshape(P, P)      # (the sum of the partials' own rounding)
    assert flag == 0
    Th = c.host(T).reshape(12, ldT).T
    R = Th[nc:nc + P, c0:c0 + P]
    mask = np.ones_like(Th, dtype=bool)
    mask[nc:nc + P, c0:c0 + P] = False
    assert np.isnan(Th[mask]).all(), "T written outside its P x P block"
    assert np.array_equal(R, np.triu(R)) and (np.diag(R) > 0).all()
    X = c.host(Rinv).reshape(P, P).T
    assert np.array_equal(X, np.triu(X))
    Gs = (Gref + Gref.T) / 2
    gb, ib = le.chol_bounds(R, X)
    if nchunks:
        gb = gb + (sb + sb.T) / 2
    ok(np.asarray(le.L(R).T @ le.L(R), np.float64), Gs, gb, "R^T R - G")
    ok(np.asarray(le.L(X) @ le.L(R), np.float64), le.L(np.eye(P)), ib, "R^-1 R - I")
    mut["R_transposed"] = ("delta", np.asarray(le.L(R) @ le.L(R).T - le.L(R).T @ le.L(R), np.float64))
    le.assert_margins(Gs, gb, mut)
    T2 = c.dev(Tfull.T)
    R2 = c.dev(np.full(P * P, np.nan))
    if nchunks == 0:
        c.ctx.debug_chol(Gd, P + 1, False, 0, T2, ldT, R2, Tblk_offset=off)
    else:
        c.ctx.debug_chol(c.dev(parts), 0, True, nchunks, T2, ldT, R2, Tblk_offset=off)
    assert np.array_equal(c.host(T2), c.host(T), equal_nan=True) and np.array_equal(c.host(R2), c.host(Rinv))


def test_cholqr_indefinite_raises_the_rank_flag_once(cases):
    """An indefinite ready-made G: one non-positive pivot, flagged once, replaced by the documented pivot 1."""
    c = cases("c1")
    G = np.array([[4.0, 2.0, 0.0, 0.0], [2.0, 10.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [0.0, 0.0, 0.0, 16.0]])
    T = c.dev(np.zeros(P * P))
    Rinv = c.dev(np.zeros(P * P))
    assert c.ctx.debug_chol(c.dev(G.T), P, False, 0, T, P, Rinv) == 1
    R = c.host(T).reshape(P, P).T
    assert np.array_equal(np.diag(R), [2.0, 3.0, 1.0, 4.0]) and R[0, 1] == 1.0
    assert c.ctx.debug_copy("counters", 2, 1)[0] == 0.0      # the hook re-zeroes the flag


@pytest.mark.parametrize("name", CASES)
def test_block_scale_front_copy_and_export(cases, name):
    """k_block_scale: Vn = W R^-1, BVn = BW R^-1 within the bound, the front-order copy of BVn for the next block solve (exact),
    and the pinned-slot export of the T columns and the counters (bit for bit)."""
    c = cases(name)
    n2, ldw, ldv = c.n2, c.n2 + GAP, c.n2 + 2 * GAP
    W_h, BW_h = c.random(n2, P), c.random(n2, P)
    rng = np.random.default_rng(3)
    R = np.triu(rng.uniform(0.5, 1.5, (P, P))) + np.diag(rng.uniform(1.0, 2.0, P))
    X = np.asarray(le.upper_inverse(R), np.float64)
    Rinv = c.dev(X.T)
    Vref, Vbnd = le.block_scale(W_h, X)
    BVref, BVbnd = le.block_scale(BW_h, X)
    le.assert_margins(Vref, Vbnd, le.block_scale_mutants(W_h, X, Vref))
    exp_n = 5 * P + 3
    src_h = rng.standard_normal(exp_n)
    src, dst = c.dev(src_h), c.dev(np.full(exp_n + 1, np.nan))
    cnt = c.torch.full((5,), -7, dtype=c.torch.int32, device=c.ctx.tdev)
    fvec_before = c.ctx.debug_copy("fvec", 0, c.front.size())
    for want_front in (False, True):
        Vn, BVn = c.block(np.full((n2, P), np.nan), ldv), c.block(np.full((n2, P), np.nan), ldv)
        c.ctx.debug_block_scale(c.block(W_h, ldw), c.block(BW_h, ldw), ldw, Rinv, Vn, BVn, ldv, src, exp_n, dst, cnt,
                                want_front=want_front)
        Vh, BVh = c.unblock(Vn, P, ldv), c.unblock(BVn, P, ldv)
        ok(Vh, Vref, Vbnd, "Vn")
        ok(BVh, BVref, BVbnd, "BVn")
        fvec = c.ctx.debug_copy("fvec", 0, c.front.size())
        if want_front:
            a = c.front.addressed()
            assert np.array_equal(fvec[a], c.front.permute_in(BVh)[a]), "fvec != permute_in(BVn)"
            assert np.array_equal(fvec[~a], fvec_before[~a], equal_nan=True)
        else:
            assert np.array_equal(fvec, fvec_before, equal_nan=True), "fvec written without want_front"
        d = c.host(dst)
        assert np.array_equal(d[:exp_n], src_h) and np.isnan(d[exp_n])
        ch = cnt.cpu().numpy()
        assert np.array_equal(ch[:4], c.ctx.debug_copy("counters", 0, 4).astype(np.int32)) and ch[4] == -7
        if want_front:
            Vn2 = c.block(np.full((n2, P), np.nan), ldv)
            c.ctx.debug_block_scale(c.block(W_h, ldw), c.block(BW_h, ldw), ldw, Rinv, Vn2, BVn, ldv)
            assert np.array_equal(c.unblock(Vn2, P, ldv), Vh), "block scale not deterministic"


@pytest.mark.parametrize("m,p", [(1, 1), (3, 1), (4, 16), (5, 17), (37, 22), (137, 49), (324, 320)])
def test_rotation_mfma(cases, m, p):
    """k_rotate (v_mfma_f64_16x16x4_f64) through launch_rotate: m mod 4, p mod 16, and p past one LDS chunk ((137, 49): chunks
    of 48 columns; (324, 320): 20 chunks of 16)."""
    c = cases("sca16")
    n2 = c.n2
    mpad = (m + 3) & ~3
    chunk = max(16, ((64 * 1024) // (8 * mpad)) & ~15)
    if (m, p) in ((137, 49), (324, 320)):
        assert p > chunk
    V_h = c.random(n2, m)
    rng = np.random.default_rng(m * 1000 + p)
    ldS = m + 3
    S_h = rng.uniform(-1, 1, (ldS, p))
    S_h[m:] = np.nan                                        # rows past m must not be read
    out = c.dev(np.full((p + 1, n2), np.nan))
    c.ctx.debug_rotate(c.dev(V_h.T), m, c.dev(S_h.T), ldS, p, out)
    o = c.host(out).reshape(p + 1, n2)
    assert np.isnan(o[p]).all()
    ref, bnd = le.rotate(V_h, S_h[:m])
    ok(o[:p].T, ref, bnd, f"rotate m={m} p={p}")
    le.assert_margins(ref, bnd, le.rotate_mutants(V_h, S_h[:m], ref))
    out2 = c.dev(np.full((p + 1, n2), np.nan))
    c.ctx.debug_rotate(c.dev(V_h.T), m, c.dev(S_h.T), ldS, p, out2)
    assert np.array_equal(c.host(out2), c.host(out), equal_nan=True)


def test_scale_store_single_vector(cases):
    """k_scale_store: v = w / beta, bv = bw / beta, beta = sqrt(max(beta^2, 0)); beta^2 = 0 or slightly negative gives zero
    vectors and beta = 0, as coded."""
    c = cases("vec16")
    n2 = c.n2
    w, bw = c.random(n2), c.random(n2)
    for b2 in (2.7, 1e-300, 0.0, -1e-17):
        v, bv, beta = c.dev(np.full(n2, np.nan)), c.dev(np.full(n2, np.nan)), c.dev(np.full(1, np.nan))
        c.ctx.debug_scale_store(c.dev(w), c.dev(bw), c.dev([b2]), v, bv, beta)
        bt = np.sqrt(max(b2, 0.0))
        inv = 1.0 / bt if bt > 0 else 0.0
        assert c.host(beta)[0] == bt
        assert np.array_equal(c.host(v), w * inv) and np.array_equal(c.host(bv), bw * inv)
        if bt > 0:       # bit equality: zero tolerance, so a dropped tail row (n2 mod 256 = 130) is caught at any size
            assert n2 % 256 != 0
            le.assert_margins(le.L(w * inv), np.zeros(n2), {"tail_row_dropped": ("delta", np.eye(1, n2, n2 - 1)[0] * w[-1] * inv)})


@pytest.mark.parametrize("name", ["sca16", "vec16"])
def test_start_field_bit_identical(cases, name):
    """k_start_field: every element jumps the LCG to its own place; equals the sequential host loop bit for bit, Dirichlet
    entries exactly 0, for one vector (single-vector driver) and a block of P."""
    c = cases(name)
    ref = le.start_field(c.sym, P)
    assert (~c.live_rows()).any() == (name == "vec16")
    for nvec in (1, P):
        out = c.dev(np.full(nvec * c.n2 + 1, np.nan))
        c.ctx.debug_start_field(nvec, out)
        o = c.host(out)
        assert np.isnan(o[-1])
        o = o[:-1].reshape(nvec, c.n2).T
        assert np.array_equal(o, ref[:, :nvec]), "start field != sequential LCG"
        assert (o[~c.live_rows()] == 0).all()
        assert np.abs(o[c.live_rows()]).max() < 1 and (o[c.live_rows()] != 0).all()


KS = (1, 3, 4, 5, 8, 9, 22)


@pytest.mark.parametrize("name", ["sca16", "vec16"])
def test_post_and_residual_kernels(cases, name):
    """k_post_sums / k_post_finish / k_post_scale (POST_MB = 4 modes per workgroup, clamped last group) and k_resid_sums /
    k_resid_finish through plfem_postprocess / plfem_residuals on arbitrary vectors at k mod 4 = 0..3; the five sums within
    the bound of the per-mode loop, the residuals within 1e-12; mode i bit-identical alone and inside the k = 22 batch."""
    c = cases(name)
    n2, kmax = c.n2, max(KS)
    V = c.random(n2, kmax, live=True)
    mask = le.core_mask(c.sym, c.cores)
    assert mask.any() and not mask.all()
    blocks = {k: c.ctx.block_values(k) for k in (("Dxx", "Dxy", "Dyy") if c.dpn == 2 else ("Minv",))}
    sref, sbnd = le.post_sums(c.sym, blocks, V, mask)
    lam = np.random.default_rng(5).uniform(-30, 30, kmax)
    rref = le.residuals(c.pencil, lam, V)
    # mutation margins: the mode index shifted by one (a clamped group read wrong), the last row dropped
    assert {k % le.POST_MB for k in KS} == {0, 1, 2, 3} and max(KS) > 4 * le.POST_MB
    r = int(np.nonzero(c.live_rows()[:c.N])[0][-1])
    d = np.zeros_like(np.asarray(sref, np.float64))
    d[0] = V[r] ** 2
    le.assert_margins(sref, sbnd, {"modes_shifted": np.roll(np.asarray(sref, np.float64), -1, axis=1),
                                   "tail_row_dropped": ("delta", d)})
    batch = None
    for k in KS:
        ev = c.dev(V[:, :k].T)
        rec, frac, _ = c.ctx.postprocess(ev.view(k, n2), c.cores, want_interior=False)
        s = le.sums_from_records(rec)
        ok(s, sref[:, :k], sbnd[:, :k] + 4 * le.U * np.abs(np.asarray(sref[:, :k], np.float64)), f"post sums k={k}")
        evn = c.host(ev).reshape(k, n2).T
        assert np.allclose(evn, V[:, :k] / rec[:, 0], rtol=4 * le.U, atol=0), "in-place normalisation"
        res = c.ctx.residuals(lam[:k], c.dev(V[:, :k].T).view(k, n2))
        assert np.all(np.abs(res - np.asarray(rref[:k], np.float64)) <= 1e-12 * np.asarray(rref[:k], np.float64)), k
        if k == kmax:
            batch = (rec, res)
    for i in (0, 3, 4, 5, 8, 21):
        ev = c.dev(V[:, i:i + 1].T)
        rec, _, _ = c.ctx.postprocess(ev.view(1, n2), c.cores, want_interior=False)
        res = c.ctx.residuals(lam[i:i + 1], c.dev(V[:, i:i + 1].T).view(1, n2))
        assert np.array_equal(rec[0], batch[0][i]) and res[0] == batch[1][i], f"mode {i} alone != in the batch"


# ---- composed check: one Lanczos cycle of each driver form ------------------------------------------------------------
DRIVERS = [("vec16", "block", 0), ("vec16", "block", 1), ("vec16", "single", 0),
           ("sca16", "block", 0), ("sca16", "block", 1), ("sca16", "single", 0)]


@pytest.mark.parametrize("name,driver,refine", DRIVERS)
def test_first_cycle_basis_and_projected_matrix(cases, monkeypatch, name, driver, refine):
    """The block driver with the fused first pass (refine_steps = 0) and with the dot / axpy pair (1), and the single-vector
    driver: after a first cycle without restart, V^T B V = I, B V = B times V, T block Hessenberg with R blocks upper
    triangular with a positive diagonal and their transposes above, and OP V_mm = V_{mm+P} T (OP through SuperLU)."""
    import scipy.sparse.linalg as spla
    c = cases(name)
    if driver == "single":
        monkeypatch.setenv("PLFEM_LANCZOS_BLOCK", "0")
    c.ctx.set_option("refine_steps", refine)
    sigma = (K0 * 1.3) ** 2 * (1 if c.dpn == 2 else -1)
    k, ncv = 4, 48
    try:
        c.ctx.factor(sigma)
        _, _, st = c.ctx.lanczos(k, ncv, 1e-8, 30, sigma)
    finally:
        c.ctx.set_option("refine_steps", 0)
    assert st["restarts"] == 0
    Pb = 1 if driver == "single" else P
    if driver == "single":
        assert st["n_block_solves"] == 0
        mm = ncv
        m = ncv
    else:
        assert st["n_block_solves"] > 1
        mm = P * (st["n_block_solves"] - 1)                 # block steps launched (the start block is the first solve)
        m = -(-ncv // P) * P
    ld = m + Pb
    n2 = c.n2
    V = c.ctx.debug_copy("V", 0, n2 * (mm + Pb)).reshape(mm + Pb, n2).T
    BV = c.ctx.debug_copy("BV", 0, n2 * (mm + Pb)).reshape(mm + Pb, n2).T
    T = c.ctx.debug_copy("Hcols", 0, ld * ld).reshape(ld, ld).T
    Bm = c.pencil.matrix("B")
    assert np.abs(V.T @ (Bm @ V) - np.eye(mm + Pb)).max() <= 1e-12
    Bref, Bbnd = c.pencil.apply("B", V)
    ok(BV, Bref, 4 * Bbnd + 64 * le.U * np.abs(np.asarray(Bref, np.float64)), "BV vs B V")
    Tn = np.abs(T[:mm + Pb, :mm]).max()
    for c0 in range(Pb, mm, Pb):
        R = T[c0:c0 + Pb, c0 - Pb:c0]
        assert np.array_equal(R, np.triu(R)) and (np.diag(R) > 0).all(), c0
        assert np.abs(T[c0 - Pb:c0, c0:c0 + Pb] - R.T).max() <= 1e-9 * Tn, c0
        if c0 >= 2 * Pb:
            assert np.abs(T[:c0 - Pb, c0:c0 + Pb]).max() <= 1e-10 * Tn, c0
    Rl = T[mm:mm + Pb, mm - Pb:mm]
    assert np.array_equal(Rl, np.triu(Rl)) and (np.diag(Rl) > 0).all()
    live = c.live_rows()
    K = (c.pencil.matrix("A") - sigma * Bm).tocsc()[live][:, live]
    lu = spla.splu(K.tocsc())
    OPV = np.zeros((n2, mm))
    OPV[live] = lu.solve(np.asarray(Bm @ V[:, :mm])[live])
    rel = np.linalg.norm(OPV - V[:, :mm + Pb] @ T[:mm + Pb, :mm]) / np.linalg.norm(OPV)
    assert rel <= 1e-9, rel
