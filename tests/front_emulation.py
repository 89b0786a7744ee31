"""NumPy emulation of the multifrontal block-LDL^T factorisation / solve that libplfem_hip.so runs,
driven by the same symbolic arrays (test infrastructure: checks the front tree on the CPU and the
HIP kernels front by front on the GPU)."""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla


NB = 32                     # pivot-block width of the block LDL^T (plan.h)


class FrontTree:
    def __init__(self, sym):
        self.sym = sym
        self.dpn = int(sym.dofs_per_node)       # unknowns per node: 2 (Hx, Hy) or 1 (scalar pencil)
        self.N = sym.N
        self.ne = sym.ne
        self.fs = sym.array("fs")
        self.fb = sym.array("fb")
        self.fptr = sym.array("fnode_ptr")
        self.fnodes = sym.array("fnodes")
        self.c0 = sym.array("cinv0")
        self.c1 = sym.array("cinv1")
        self.epos = sym.array("epos").reshape(6, sym.ne)
        self.lptr = sym.array("leaf_elem_ptr")
        self.lel = sym.array("leaf_elems")
        self.foff = sym.array("foff")
        self.L = sym.info["levels"]
        self.nf = sym.info["nfronts"]
        self.leaf0 = (1 << self.L) - 1

    def m(self, f):
        return self.dpn * int(self.fs[f] + self.fb[f])

    def s2(self, f):
        return self.dpn * int(self.fs[f])

    def dofs(self, q):
        """Local DOFs of the local nodes q (component-interleaved: node q has DOFs dpn q .. dpn q + dpn - 1)."""
        q = np.asarray(q)
        return (self.dpn * q[:, None] + np.arange(self.dpn)).ravel()

    def nodes(self, f):
        return self.fnodes[self.fptr[f]:self.fptr[f] + self.fs[f] + self.fb[f]]

    def device_front(self, ctx, f, with_schur=False, dump=None):
        """Front f as the device context stores it, rebuilt as one m x m array [row, col] (symbolic.h): [F11; F21] (m x s2,
        leading dimension m) and Z^T (s2 x b2, leading dimension s2) from the permanent storage; the Schur complement F22
        (b2 x b2) from the arena of the front's tree level -- only meaningful while that arena has not been reused (after a
        complete factorisation: levels 0 and 1), NaN otherwise.  dump: the whole permanent storage already copied
        (``ctx.debug_copy("front", 0, front_doubles)``), for callers that walk every front of a large tree."""
        m, s2 = self.m(f), self.s2(f)
        b2 = m - s2
        off = int(self.foff[f])
        F = np.full((m, m), np.nan)

        def stored(o, n):
            return dump[o:o + n] if dump is not None else ctx.debug_copy("front", o, n)

        if s2:
            F[:, :s2] = stored(off, m * s2).reshape(s2, m).T
            if b2:
                F[:s2, s2:] = stored(off + m * s2, s2 * b2).reshape(b2, s2).T
        if with_schur and b2:
            level = int(np.floor(np.log2(f + 1)))
            arena = (int(self.sym.info["arena_doubles"]) + 31) & ~31
            soff = int(self.sym.array("soff")[f])
            F[s2:, s2:] = ctx.debug_copy("schur", (level & 1) * arena + soff, b2 * b2).reshape(b2, b2).T
        return F


def element_K_scalar(em, k0sq, sigma):
    """6x6 element matrices of K = (stiff - k0^2 M_eps) - sigma M of the scalar pencil (oracle.scalar.element_matrices;
    A in the AXX slot, B = M in the MINV slot, as launch_element_matrices_scalar assembles them)."""
    return em["stiff"] - k0sq * em["eps_m"] - sigma * em["mass"]


def element_K(em, k0sq, sigma):
    """12x12 element matrices of K = A - sigma B in the interleaved (node, component) DOF order."""
    Axx = em["kxx"] + em["div_xx"] - k0sq * em["mass"]
    Ayy = em["kyy"] + em["div_yy"] - k0sq * em["mass"]
    Axy = em["kxy"] + em["div_xy"]
    Ayx = em["kyx"] + np.transpose(em["div_xy"], (0, 2, 1))
    Mi = em["mass_eps_inv"]
    ne = Axx.shape[0]
    Ke = np.zeros((ne, 12, 12))
    Ke[:, 0::2, 0::2] = Axx - sigma * Mi
    Ke[:, 0::2, 1::2] = Axy
    Ke[:, 1::2, 0::2] = Ayx
    Ke[:, 1::2, 1::2] = Ayy - sigma * Mi
    return Ke


def assemble_front(T: FrontTree, f, Ke, S):
    """Front f before elimination: leaf = its elements, internal = extend-add of the children's S."""
    mn = int(T.fs[f] + T.fb[f])
    m = T.dpn * mn
    fn = T.nodes(f)
    Fm = np.zeros((m, m), dtype=Ke.dtype)              # (np.longdouble elements: the whole factorisation in extended precision)
    pad = T.dofs(np.nonzero(fn < 0)[0])
    Fm[pad, pad] = 1.0
    if f >= T.leaf0:
        lf = f - T.leaf0
        for e in T.lel[T.lptr[lf]:T.lptr[lf + 1]]:
            pos = T.epos[:, e]
            dofs = T.dofs(pos)
            ok = np.repeat(pos >= 0, T.dpn)
            ii = dofs[ok]
            Fm[np.ix_(ii, ii)] += Ke[e][np.ix_(ok, ok)]
    else:
        for ch, ci in ((2 * f + 1, T.c0), (2 * f + 2, T.c1)):
            inv = ci[T.fptr[f]:T.fptr[f] + mn]
            ok = inv >= 0
            pd = T.dofs(np.nonzero(ok)[0])
            cd = T.dofs(inv[ok])                                   # rows of the child's Schur complement
            Fm[np.ix_(pd, pd)] += S[ch][np.ix_(cd, cd)]
    return Fm


MISTAKES = ("rep_positive", "rmax_block", "rep_thr", "no_det_guard", "d2_uncounted")


def ldl_partial(Fm, s2, kinds=None, log=None, mistake=None):
    """Partial block LDL^T of the first s2 pivots, node pair by node pair in the static order (local DOFs 2q, 2q+1, no
    permutation; kernels_front.hip): two scalar pivots (a, then c - b^2 / a) or one 2 x 2 pivot, whichever amplifies rounding
    errors less ((b / a)^2 against max|E|^2 / |det|).  Returns the storage the HIP path leaves in F: lower(F11) = L11^-1,
    upper(F11) = L11^-T, F21 = Z = L21 L11^-1, F12 = Z^T, F22 = S; and D^-1 as (diagonal, off-diagonal) per row.
    The elimination runs in panels of NB columns (the update of the trailing matrix is one product per panel, as on the
    device), so that fronts of a few thousand rows stay cheap.
    A vanishing pivot is replaced, not permuted away (pair_step / ldl_pivot_block): with rmax the largest entry the pair's
    own two rows have in the nbk x nbk pivot block -- both triangles, as the block arrives at its block step, i.e. after
    the updates of all earlier block steps and before any elimination inside it; the identity padding of a partial block
    adds nothing to the rows of a pair, a padding node is the unit diagonal entry the assembly gave it --
    thr = max(1e-13 rmax, 1e-300), rep = max(1e-8 rmax, 1e-300), and
      "a":   the first scalar pivot a,        |a| < thr       -> +-rep
      "d2":  the second one, d2 = c - g b,    |d2| < thr      -> +-rep
      "det": the determinant of the 2 x 2 form, |det| < thr s -> +-rep s      (s = max|E|)
    each with the sign of the value it replaces (+ for zero).
    kinds (a list, optional): gets (is_2x2, margin) per pair, margin = |lhs - rhs| / max(lhs, rhs) of the kind test.
    log (a list, optional): gets (pair, site, value, rmax) per replacement; its length is what the device counts.
    mistake (one of MISTAKES, optional): a deliberately wrong rule, for the host tests that show the GPU tests would see it."""
    assert mistake is None or mistake in MISTAKES
    F = Fm.copy()
    Dinv = np.zeros((s2, 2), dtype=F.dtype)

    def replaced(value, thr, rep, q, site, rm):
        """value, or its replacement (logged) where it vanishes against thr."""
        if abs(value) >= thr:
            return value
        if log is not None and not (mistake == "d2_uncounted" and site == "d2"):
            log.append((q, site, value, rm))
        return rep if mistake == "rep_positive" or not value < 0 else -rep

    for k0 in range(0, s2, NB):
        k1 = min(k0 + NB, s2)
        Cp = np.zeros((F.shape[0] - k1, k1 - k0), dtype=F.dtype)           # the panel's columns below it, as they were eliminated
        rowmax = np.abs(F[k0:k1, k0:k1]).max(axis=1)                       # of the block on arrival
        if mistake == "rmax_block":
            rowmax[:] = rowmax.max()
        for k in range(k0, k1, 2):
            a, b, c = F[k, k], F[k + 1, k], F[k + 1, k + 1]
            det = a * c - b * b
            s = max(abs(a), abs(b), abs(c))
            rm = max(rowmax[k - k0], rowmax[k + 1 - k0])
            thr, rep = max(1e-13 * rm, 1e-300), max(1e-8 * rm, 1e-300)
            if mistake == "rep_thr":
                rep = thr
            lhs, rhs = b * b * abs(det), a * a * s * s
            if kinds is not None:
                kinds.append((bool(lhs > rhs), abs(lhs - rhs) / max(lhs, rhs, 1e-300)))
            if lhs <= rhs:
                for j in (k, k + 1):                         # two steps of the scalar LDL^T
                    d = replaced(F[j, j], thr, rep, k // 2, "a" if j == k else "d2", rm)
                    col = F[j + 1:, j].copy()
                    l = col / d
                    F[j + 1:, j + 1:k1] -= np.outer(l, col[:k1 - j - 1])
                    F[j + 1:, j] = l
                    Cp[:, j - k0] = col[k1 - j - 1:]
                    Dinv[j] = (1.0 / d, 0.0)
            else:
                if mistake != "no_det_guard":
                    det = replaced(det, thr * s, rep * s, k // 2, "det", rm)
                e11, e12, e22 = c / det, -b / det, a / det
                Dinv[k] = (e11, e12)
                Dinv[k + 1] = (e22, e12)
                C = F[k + 2:, k:k + 2].copy()
                Lc = np.stack([C[:, 0] * e11 + C[:, 1] * e12, C[:, 0] * e12 + C[:, 1] * e22], 1)
                F[k + 2:, k + 2:k1] -= Lc @ C[:k1 - k - 2].T
                F[k + 2:, k:k + 2] = Lc
                F[k + 1, k] = 0.0
                Cp[:, k - k0:k - k0 + 2] = C[k1 - k - 2:]
        F[k1:, k1:] -= F[k1:, k0:k1] @ Cp.T
    L11 = np.tril(F[:s2, :s2], -1) + np.eye(s2)
    if F.dtype == np.float64:
        X = sla.solve_triangular(L11, np.eye(s2), lower=True, unit_diagonal=True) if s2 else np.zeros((0, 0))
    else:                                                   # (LAPACK has no extended precision) column-oriented L^-1
        X = np.eye(s2, dtype=F.dtype)
        for j in range(s2 - 1):
            X[j + 1:, :j + 1] -= np.outer(L11[j + 1:, j], X[j, :j + 1])
    out = F.copy()
    out[:s2, :s2] = np.tril(X) + np.tril(X, -1).T
    Z = F[s2:, :s2] @ np.tril(X)
    out[s2:, :s2] = Z
    out[:s2, s2:] = Z.T
    return out, Dinv


def factor(T: FrontTree, Ke, kinds=None, logs=None, mistake=None):
    """Every front, leaves first.  kinds (a dict, optional): front -> ldl_partial's (is_2x2, margin) list; logs (a dict,
    optional): front -> ldl_partial's replacement log (fronts without a replacement have no entry)."""
    Fs = [None] * T.nf
    Ds = [None] * T.nf
    S = [None] * T.nf
    for f in range(T.nf - 1, -1, -1):
        Fm = assemble_front(T, f, Ke, S)
        s2 = T.s2(f)
        k = [] if kinds is not None else None
        lg = []
        Fs[f], Ds[f] = ldl_partial(Fm, s2, k, lg, mistake)
        if kinds is not None:
            kinds[f] = k
        if logs is not None and lg:
            logs[f] = lg
        S[f] = Fs[f][s2:, s2:]
    return Fs, Ds


def solve(T: FrontTree, Fs, Ds, rhs):
    """Forward / backward sweeps exactly as the HIP kernels do them.  rhs, result: dpn N-vectors (component-major)."""
    N, dpn = T.N, T.dpn
    W = [None] * T.nf
    Y = [None] * T.nf
    for f in range(T.nf - 1, -1, -1):
        mn = int(T.fs[f] + T.fb[f])
        m, s2 = dpn * mn, T.s2(f)
        fn = T.nodes(f)
        w = np.zeros(m)
        node = np.repeat(fn, dpn)
        comp = np.tile(np.arange(dpn), mn)
        own = (np.arange(m) < s2) & (node >= 0)
        w[own] = rhs[comp[own] * N + node[own]]
        if f < T.leaf0:
            for ch, ci in ((2 * f + 1, T.c0), (2 * f + 2, T.c1)):
                inv = np.repeat(ci[T.fptr[f]:T.fptr[f] + mn], dpn)
                ok = inv >= 0
                w[ok] += W[ch][T.s2(ch) + dpn * inv[ok] + comp[ok]]
        F = Fs[f]
        r = w[:s2].copy()
        t = np.triu(F[:s2, :s2]).T @ r                             # L11^-1 r from the mirrored upper storage
        ys = Ds[f][:, 0] * t + Ds[f][:, 1] * t.reshape(-1, 2)[:, ::-1].ravel()        # D^-1 t, partner of row i = i ^ 1
        w[s2:] -= F[s2:, :s2] @ r                                  # u = w_b - Z r
        W[f], Y[f] = w, ys
    x = np.zeros(dpn * N)
    for f in range(T.nf):
        mn = int(T.fs[f] + T.fb[f])
        m, s2 = dpn * mn, T.s2(f)
        fn = T.nodes(f)
        node = np.repeat(fn, dpn)
        comp = np.tile(np.arange(dpn), mn)
        xb = np.where(node[s2:] >= 0, x[comp[s2:] * N + np.maximum(node[s2:], 0)], 0.0)
        F = Fs[f]
        v = np.concatenate([Y[f], -xb])                            # [ys ; -x_b]
        xo = np.tril(F[:, :s2]).T @ v                              # L11^-T ys - Z^T x_b
        ok = node[:s2] >= 0
        x[comp[:s2][ok] * N + node[:s2][ok]] = xo[ok]
    return x


# ---- the launch plan rules of plan.h / plan.cpp / plfem_create, restated -----------------------------------------------
ROW_FORM_MAX_FRONTS = 32
MIX_BIG_S2 = 192
BLOCK_P = 4
LDS_LIMIT = 160 * 1024      # bytes of LDS per workgroup on the MI355X (gfx950)


def lds_need(P, worst_m):
    """LDS the sweeps of P right-hand sides need (plfem_create): the staged vector of the largest front + the tile kernels'
    partial sums."""
    return 8 * P * (worst_m + 2) + 8 * 8 * P * 64


def fwd_block_rows(count):
    return 8 if count <= 8 else 16 if count <= ROW_FORM_MAX_FRONTS else 64


def bwd_block_rows(count, leaf):
    return 64 if leaf else 8 if count <= ROW_FORM_MAX_FRONTS else 16


def level_forms(sym):
    """Per tree level (root first) the record plfem_debug_level_plan returns (_native.PLAN_FIELDS), from the symbolic
    arrays and the rules of plan.cpp, plus the kernel names of the two sweeps ("fwd", "bwd"), "leaf" and the number of
    fronts of the level that have rows at all ("fronts_m") and owned DOFs ("fronts_s2")."""
    dpn = int(sym.dofs_per_node)
    fs, fb = sym.array("fs").astype(np.int64), sym.array("fb").astype(np.int64)
    L = sym.info["levels"]
    s2_all, m_all = dpn * fs, dpn * (fs + fb)
    worst = int(m_all.max())
    max_block_p = BLOCK_P if lds_need(BLOCK_P, worst) <= LDS_LIMIT else 1
    cdiv = lambda a, b: -(-a // b)                      # noqa: E731
    out = []
    for lev in range(L + 1):
        first, count = (1 << lev) - 1, 1 << lev
        s2, m = s2_all[first:first + count], m_all[first:first + count]
        leaf = lev == L
        fr, br = fwd_block_rows(count), bwd_block_rows(count, leaf)
        mixed = fr == 64 and bool((s2 > MIX_BIG_S2).any())
        big = (s2 > MIX_BIG_S2) & (fr == 64)
        fwd_n = int(np.where(big, cdiv(m, 16), cdiv(m, fr)).sum())
        bwd_n = int(cdiv(np.maximum(s2, 0 if leaf else 1), br).sum())
        fwd = {8: "k_fwd_rows<P,1,4>", 16: "k_fwd_rows<P,2,4>"}.get(fr, "k_fwd_mix" if mixed else "k_fwd")
        bwd = {8: "k_bwd_rows<P,1,4>", 16: "k_bwd_rows<P,2,4>"}.get(br, "k_bwd")
        out.append({"count": count, "fwd_rows": fr, "bwd_rows": br, "fwd_mixed": int(mixed), "max_s2": int(s2.max()),
                    "max_m": int(m.max()), "fwd_n": fwd_n, "bwd_n": bwd_n, "steps": cdiv(int(s2.max()), NB),
                    "max_block_p": max_block_p, "fwd": fwd, "bwd": bwd, "leaf": leaf,
                    "fronts_m": int((m > 0).sum()), "fronts_s2": int((s2 > 0).sum())})   # fronts with rows / with owned DOFs
    return out
