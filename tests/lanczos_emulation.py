"""Host references of the device kernels of the Lanczos drivers (csrc/kernels_lanczos.hip and the block SpMVs of
csrc/kernels_assembly.hip), restated in np.longdouble from the kernels' definitions, with the error bounds the GPU tests
hold them to and the mutation margins that show those tests would catch the cheapest plausible kernel mistakes.

Layouts (include/plfem.h): vectors have n2 = dpn N entries, component-major; a block of P vectors is an (n2, P) array;
the interleaved copy of a block is wil[(node dpn + component) P + q]; the front order of the sweeps puts component c of
node i at slot npos[i] + c (npos = -1: Dirichlet node), P values per slot together.
Bounds: a reduction of products gets |gpu - ref| <= GAMMA u sum |a_i b_i|; the MFMA rotation (m + 4) u sum |V| |S|; an axpy
update (ncols + 2) u (|w| + sum |P| |h|) per row.  GAMMA = 128 covers the deepest summation chain at the C1 size (a lane's
run, the 64-lane butterfly, the partials over up to ~3000 chunks: well under 128 additions in any one chain)."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53
GAMMA = 128.0
PANEL_CHUNK = 1024          # rows per partial sum of the panel products (csrc/plan.h) = FIRST_ROWS of the fused first pass
BLOCK_P = 4
GRAM_ROWS = 32              # rows per workgroup of the block B product = per Gram partial
POST_MB = 4                 # modes per workgroup of k_post_sums / k_resid_sums
MARGIN = 100.0              # every mutation must exceed its tolerance this many times over
LCG_A = 6364136223846793005
LCG_C = 1442695040888963407
LCG_SEED = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


def L(a):
    return np.asarray(a, dtype=np.longdouble)


# ---- bounds ------------------------------------------------------------------------------------------------------------
def reduction_bound(absA, absB):
    """GAMMA u sum |a_i b_i| of the products absA^T absB (float64 arrays of |.|)."""
    return GAMMA * U * (absA.T @ absB)


def axpy_bound(W, Pm, H):
    """(ncols + 2) u (|w| + sum_c |P[:, c]| |h[c]|) per row of W - Pm H."""
    return (Pm.shape[1] + 2) * U * (np.abs(W) + np.abs(Pm) @ np.abs(H))


def rotate_bound(V, S):
    return (V.shape[1] + 4) * U * (np.abs(V) @ np.abs(S))


def within(gpu, ref, bound):
    """Largest |gpu - ref| / bound (<= 1 passes); an entry with a zero bound must be exact."""
    d = np.abs(L(gpu) - ref)
    b = np.asarray(bound, dtype=np.float64)
    return float(np.max(np.where(b > 0, d / np.where(b > 0, b, 1.0), np.where(d > 0, np.inf, 0.0))))


def margins(ref, bound, mutants):
    """For every mutant (a name -> the result the mistaken kernel would have produced, or the change it makes), the factor
    by which its most distant entry exceeds the tolerance.  ``("delta", d)`` gives the change directly."""
    out = {}
    for name, m in mutants.items():
        if isinstance(m, tuple) and m[0] == "delta":
            d = np.abs(np.asarray(m[1], dtype=np.float64))
        else:
            d = np.abs(np.asarray(L(m) - ref, dtype=np.float64))
        b = np.asarray(bound, dtype=np.float64)
        out[name] = float(np.max(np.where(b > 0, d / np.where(b > 0, b, 1.0), np.where(d > 0, np.inf, 0.0))))
    return out


def assert_margins(ref, bound, mutants, factor=MARGIN):
    m = margins(ref, bound, mutants)
    assert m, "no mutation to check"
    bad = {k: v for k, v in m.items() if not v >= factor}
    assert not bad, f"inputs would not catch these mistakes {factor:g}-fold: {bad}"
    return m


def last_chunk(n, rows=PANEL_CHUNK):
    """First row of the last (possibly partial) chunk of n rows."""
    return ((n - 1) // rows) * rows


def last_live_row(A):
    """Last row of A that holds a nonzero (a Dirichlet row of a Lanczos vector is zero: dropping it changes nothing)."""
    return int(np.nonzero(np.any(np.asarray(A) != 0, axis=1))[0][-1])


def misread_transposed(H):
    """An (ncols, P) coefficient block read with the two indices swapped (column-major data read row-major)."""
    return np.asarray(H).ravel(order="F").reshape(H.shape)


# ---- panel products ----------------------------------------------------------------------------------------------------
def panel_dot(Pm, W):
    """h[c, q] = Pm[:, c] . W[:, q] in extended precision; bound of the GPU's two-stage reduction."""
    return L(Pm).T @ L(W), reduction_bound(np.abs(Pm), np.abs(W))


def panel_dot_mutants(Pm, W, h):
    n, ncols = Pm.shape
    P = W.shape[1]
    c0 = last_chunk(n)
    r = last_live_row(Pm)
    out = {"tail_row_dropped": ("delta", np.outer(Pm[r], W[r])),
           "last_chunk_twice": ("delta", Pm[c0:].T @ W[c0:])}
    if ncols > 1:
        out["columns_shifted"] = np.roll(np.asarray(h, dtype=np.float64), -1, axis=0)
    if ncols > 1 and P > 1:
        out["transposed"] = misread_transposed(np.asarray(h, dtype=np.float64))
    return out


def panel_axpy(W, Pm, H):
    """W - Pm H in extended precision and its bound."""
    return L(W) - L(Pm) @ L(H), axpy_bound(W, Pm, H)


def panel_axpy_mutants(W, Pm, H):
    ncols = Pm.shape[1]
    tail = np.zeros_like(W)
    r = last_live_row(Pm)
    tail[r] = (Pm[r] @ H)                           # the last row (with data: not a Dirichlet row) left un-updated
    out = {"tail_row_dropped": ("delta", tail), "last_column_dropped": ("delta", np.outer(Pm[:, -1], H[-1]))}
    if ncols > 1:
        out["columns_shifted"] = ("delta", Pm @ (H - np.roll(H, -1, axis=0)))
    if ncols > 1 and H.shape[1] > 1:
        out["transposed"] = ("delta", Pm @ (H - misread_transposed(H)))
    return out


# ---- layouts -----------------------------------------------------------------------------------------------------------
def interleave(W, N, dpn):
    """(n2, P) block -> wil[(node dpn + component) P + q]."""
    P = W.shape[1]
    return np.ascontiguousarray(np.asarray(W).reshape(dpn, N, P).transpose(1, 0, 2)).ravel()


def deinterleave(wil, N, dpn, P):
    return np.ascontiguousarray(np.asarray(wil).reshape(N, dpn, P).transpose(1, 0, 2)).reshape(dpn * N, P)


class FrontOrder:
    """The front-order <-> global permutation of the sweeps (sym.array("npos"), P values per slot together)."""

    def __init__(self, sym, P=BLOCK_P):
        self.N, self.dpn, self.P = sym.N, sym.dofs_per_node, P
        self.npos = sym.array("npos").astype(np.int64)
        self.slots = 2 * int(sym.array("fnode_ptr")[-1])          # slots of the front-order buffers
        live = np.nonzero(self.npos >= 0)[0]
        # global row g = c N + node  <->  slot npos[node] + c
        self.rows = np.concatenate([c * self.N + live for c in range(self.dpn)])
        self.slot_of_row = np.concatenate([self.npos[live] + c for c in range(self.dpn)])
        assert np.unique(self.slot_of_row).size == self.slot_of_row.size

    def size(self):
        return self.slots * self.P

    def permute_in(self, X, fill=0.0):
        """(n2, P) global block -> flat front-order buffer; slots no row maps to get ``fill``."""
        out = np.full((self.slots, self.P), fill, dtype=np.float64)
        out[self.slot_of_row] = np.asarray(X)[self.rows]
        return out.ravel()

    def permute_out(self, xl):
        """flat front-order buffer -> (n2, P) global block, Dirichlet rows 0 (what k_permute_dot_first writes)."""
        xl = np.asarray(xl).reshape(self.slots, self.P)
        out = np.zeros((self.dpn * self.N, self.P), dtype=np.float64)
        out[self.rows] = xl[self.slot_of_row]
        return out

    def addressed(self):
        """Boolean mask of the flat front-order entries some global row maps to."""
        m = np.zeros((self.slots, self.P), dtype=bool)
        m[self.slot_of_row] = True
        return m.ravel()


# ---- the assembled pencil ----------------------------------------------------------------------------------------------
class Pencil:
    """The interior-restricted pencil as the block SpMVs apply it: the CSR pattern of the analysis, the block values of the
    context, Dirichlet rows zero (Dirichlet columns are read like any other)."""

    def __init__(self, sym, ctx):
        import scipy.sparse as sp
        self.N, self.dpn = sym.N, sym.dofs_per_node
        self.rowptr = sym.array("rowptr").astype(np.int64)
        self.colind = sym.array("colind").astype(np.int64)
        self.bmask = sym.array("bmask").astype(bool)
        self.rows = np.repeat(np.arange(self.N), np.diff(self.rowptr))
        live = ~self.bmask[self.rows]
        names = ("Axx", "Axy", "Ayx", "Ayy", "Minv") if self.dpn == 2 else ("Axx", "Minv")
        self.vals = {k: ctx.block_values(k) for k in names}
        self.vals_live = {k: np.where(live, v, 0.0) for k, v in self.vals.items()}
        self.csr = {k: sp.csr_matrix((v, self.colind, self.rowptr), shape=(self.N, self.N)) for k, v in self.vals_live.items()}
        self.abs_csr = {k: abs(m) for k, m in self.csr.items()}

    def _prod(self, name, x):
        """Extended-precision CSR product of one block with the columns of x (N, P)."""
        x = L(x)
        prod = L(self.vals_live[name])[:, None] * x[self.colind]
        return np.add.reduceat(prod, self.rowptr[:-1], axis=0)

    def _blocks(self, which):
        if which == "B":
            return (("Minv", None), (None, "Minv")) if self.dpn == 2 else (("Minv",),)
        return (("Axx", "Axy"), ("Ayx", "Ayy")) if self.dpn == 2 else (("Axx",),)

    def apply(self, which, X):
        """(n2, P) -> B X or A X in extended precision, and the bound GAMMA u |M| |X| of the GPU's row sums."""
        X = np.asarray(X, dtype=np.float64).reshape(self.dpn * self.N, -1)
        N = self.N
        out, bnd = [], []
        for row in self._blocks(which):
            acc = L(np.zeros((N, X.shape[1])))
            b = np.zeros((N, X.shape[1]))
            for c, name in enumerate(row):
                if name is None:
                    continue
                xc = X[c * N:(c + 1) * N]
                acc = acc + self._prod(name, xc)
                b += self.abs_csr[name] @ np.abs(xc)
            out.append(acc)
            bnd.append(GAMMA * U * b)
        return np.concatenate(out), np.concatenate(bnd)

    def matrix(self, which):
        """Float64 sparse matrix of the pencil (Dirichlet rows zero) on full-length vectors."""
        import scipy.sparse as sp
        return sp.bmat([[self.csr[n] if n else None for n in row] for row in self._blocks(which)], format="csr")

    def last_live_row(self):
        """Last global row that is not a Dirichlet row."""
        live = np.nonzero(~self.bmask)[0]
        return (self.dpn - 1) * self.N + int(live[-1])


def spmv_mutants(pencil, which, X, Y):
    """Y = M X (reference): the last live row dropped, the columns of X shifted by one, the last nonzero of that row lost."""
    Yf = np.asarray(Y, dtype=np.float64)
    r = pencil.last_live_row()
    d = np.zeros_like(Yf)
    d[r] = Yf[r]
    out = {"tail_row_dropped": ("delta", d)}
    if X.shape[1] > 1:
        out["columns_shifted"] = np.roll(Yf, -1, axis=1)
    return out


def gram(X, BX, BX_bound, absB_absX):
    """X^T (B X) from the extended-precision B X, bound of the Gram partials' sum (the products' sum plus the B X errors)."""
    G = L(X).T @ L(BX)
    return G, GAMMA * U * (np.abs(X).T @ absB_absX) + np.abs(X).T @ BX_bound


def gram_mutants(partials, G):
    """partials (P P, nb): the last partial counted twice, the last one dropped, the columns of B X shifted by one (G is
    symmetric up to rounding, so a transposed entry order is no mistake the bound could see: the CholQR test covers the
    unsymmetrised triangle)."""
    P = int(round(np.sqrt(partials.shape[0])))
    last = partials[:, last_live_row(partials.T)].reshape(P, P)       # (a chunk of Dirichlet rows only has zero partials)
    return {"last_chunk_twice": ("delta", last), "tail_chunk_dropped": ("delta", last),
            "columns_shifted": np.roll(np.asarray(G, dtype=np.float64), -1, axis=1)}


# ---- CholQR ------------------------------------------------------------------------------------------------------------
def cholesky_upper(G):
    """R upper triangular with R^T R = (G + G^T) / 2 in extended precision (k_chol_small's recurrence, no pivot repair)."""
    G = L(G)
    Gs = (G + G.T) / 2
    P = G.shape[0]
    R = L(np.zeros((P, P)))
    for j in range(P):
        for i in range(j + 1):
            v = Gs[i, j] - sum(R[k, i] * R[k, j] for k in range(i))
            if i == j:
                assert v > 0, "G is not positive definite"
                R[j, j] = np.sqrt(v)
            else:
                R[i, j] = v / R[i, i]
    return R


def upper_inverse(R):
    R = L(R)
    P = R.shape[0]
    X = L(np.zeros((P, P)))
    for j in range(P):
        X[j, j] = 1 / R[j, j]
        for i in range(j - 1, -1, -1):
            X[i, j] = -sum(R[i, k] * X[k, j] for k in range(i + 1, j + 1)) / R[i, i]
    return X


def chol_bounds(R, Rinv):
    """LAPACK-style componentwise bounds: |R^T R - G| <= 8 P u |R|^T |R|, |R^-1 R - I| <= 8 P u |R^-1| |R|."""
    P = R.shape[0]
    aR, aX = np.abs(np.asarray(R, np.float64)), np.abs(np.asarray(Rinv, np.float64))
    return 8 * P * U * (aR.T @ aR), 8 * P * U * (aX @ aR)


def spd_matrix(rng, P, cond):
    """Symmetric positive definite P x P matrix with the given condition number (random orthogonal eigenvectors)."""
    Q, _ = np.linalg.qr(rng.standard_normal((P, P)))
    w = np.logspace(0, -np.log10(cond), P)
    return (Q * w) @ Q.T


def split_partials(G, nchunks, rng):
    """nchunks partials per entry (the layout of k_chol_small: [(c P + q) nchunks + t] -> G[c + q ldg]) that sum to G up to
    rounding: G / nchunks plus telescoping O(|G| / nchunks) noise, so that every chunk matters."""
    P = G.shape[0]
    z = rng.standard_normal((P * P, nchunks)) * (np.abs(G).max() / nchunks)
    base = np.asarray(G).reshape(P * P, 1) / nchunks                # entry cq = c P + q is G[c, q]
    return base + z - np.roll(z, -1, axis=1)


def partials_sum(partials):
    """The matrix k_chol_small forms from the partials, in extended precision: G[c + q P] = sum_t partial[c P + q][t]."""
    P = int(round(np.sqrt(partials.shape[0])))
    return L(partials).sum(axis=1).reshape(P, P)                    # entry cq = c P + q -> G[c + q P]: row c, column q


# ---- block scale, rotation ---------------------------------------------------------------------------------------------
def block_scale(W, Rinv):
    """W R^-1 (R^-1 upper) in extended precision and its bound."""
    X = np.triu(np.asarray(Rinv, dtype=np.float64))
    return L(W) @ L(X), GAMMA * U * (np.abs(W) @ np.abs(X))


def block_scale_mutants(W, Rinv, ref):
    X = np.triu(np.asarray(Rinv, dtype=np.float64))
    d = np.zeros(W.shape)
    d[-1] = np.asarray(ref[-1], dtype=np.float64)
    return {"tail_row_dropped": ("delta", d), "rinv_transposed": ("delta", W @ (X - X.T)),
            "columns_shifted": np.roll(np.asarray(ref, dtype=np.float64), -1, axis=1)}


def rotate(V, S):
    return L(V) @ L(S), rotate_bound(V, S)


def rotate_mutants(V, S, ref):
    m, p = S.shape
    ref = np.asarray(ref, dtype=np.float64)
    d = np.zeros_like(ref)
    d[-1] = ref[-1]
    out = {"tail_row_dropped": ("delta", d), "last_term_dropped": ("delta", np.outer(V[:, -1], S[-1]))}
    if p > 1:
        out["columns_shifted"] = np.roll(ref, -1, axis=1)
    if m == p and m > 1:
        out["transposed"] = ("delta", V @ (S - S.T))
    return out


# ---- start field -------------------------------------------------------------------------------------------------------
def lcg_sequence(count):
    """Element e of the stream = the state after e + 1 updates (a plain sequential loop)."""
    out = np.empty(count, dtype=np.uint64)
    s = LCG_SEED
    for e in range(count):
        s = (LCG_A * s + LCG_C) & _M64
        out[e] = s
    return out


def lcg_jump(e):
    """The jump-ahead of k_start_field's comment: a^(e+1) and its increment by binary powering."""
    k, am, ap, cm, cp = e + 1, 1, 0, LCG_A, LCG_C
    while k:
        if k & 1:
            am = (am * cm) & _M64
            ap = (ap * cm + cp) & _M64
        cp = ((cm + 1) * cp) & _M64
        cm = (cm * cm) & _M64
        k >>= 1
    return (am * LCG_SEED + ap) & _M64


def lcg_values(states):
    """[-1, 1) values of the states: (s >> 11) / 2^53 * 2 - 1."""
    return (np.asarray(states, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) / 9007199254740992.0 * 2.0 - 1.0


def start_field(sym, nvec):
    """(n2, nvec) start block of the drivers: a sequential loop over (vector, component, interior DOF)."""
    N, dpn = sym.N, sym.dofs_per_node
    interior = sym.array("interior").astype(np.int64)
    ns = interior.size
    vals = lcg_values(lcg_sequence(nvec * dpn * ns)).reshape(nvec, dpn, ns)
    out = np.zeros((dpn * N, nvec))
    for q in range(nvec):
        for c in range(dpn):
            out[c * N + interior, q] = vals[q, c]
    return out


# ---- per-mode post-processing and residuals ----------------------------------------------------------------------------
def core_mask(sym, cores):
    """in_any_core of p2_element.h on the DOF locations: closed discs, products rounded separately."""
    loc = sym.array("doflocs").reshape(2, -1)
    x, y = loc[0], loc[1]
    m = np.zeros(x.size, dtype=bool)
    for cx, cy, r in np.asarray(cores, dtype=np.float64).reshape(-1, 3):
        dx, dy = x - cx, y - cy
        m |= dx * dx + dy * dy <= r * r
    return m


def post_sums(sym, ctx_blocks, V, mask):
    """The five sums of k_post_sums per mode (the per-mode loop of oracle/hfield.py postprocess_modes, oracle/scalar.py):
    [0] sum vx^2, [1] sum vy^2, [2] core vx^2, [3] core vy^2, [4] vx.Dxx vx + 2 vx.Dxy vy + vy.Dyy vy (scalar: v.M v), over
    every row (the tests zero the Dirichlet entries, as a mode has them).  V: (n2, k).  Returns (5, k) sums and bounds."""
    import scipy.sparse as sp
    N, dpn = sym.N, sym.dofs_per_node
    rowptr, colind = sym.array("rowptr"), sym.array("colind")

    def csr(name):
        return sp.csr_matrix((ctx_blocks[name], colind, rowptr), shape=(N, N))

    rows = np.repeat(np.arange(N), np.diff(rowptr))

    def quad(name, a, b):           # a^T M b in extended precision, and sum |a_i M_ij b_j|
        prod = L(ctx_blocks[name])[:, None] * L(a)[rows] * L(b)[colind]
        return prod.sum(axis=0), abs(csr(name)) @ np.abs(b) * np.abs(a)

    vx = V[:N]
    vy = V[N:] if dpn == 2 else np.zeros_like(vx)
    s = [L(vx * 0).sum(axis=0)] * 5
    b = [None] * 5
    s[0], b[0] = (L(vx) ** 2).sum(axis=0), (vx ** 2).sum(axis=0)
    s[1], b[1] = (L(vy) ** 2).sum(axis=0), (vy ** 2).sum(axis=0)
    s[2], b[2] = (L(vx[mask]) ** 2).sum(axis=0), (vx[mask] ** 2).sum(axis=0)
    s[3], b[3] = (L(vy[mask]) ** 2).sum(axis=0), (vy[mask] ** 2).sum(axis=0)
    if dpn == 2:
        a1, b1 = quad("Dxx", vx, vx)
        a2, b2 = quad("Dxy", vx, vy)
        a3, b3 = quad("Dyy", vy, vy)
        s[4], b[4] = a1 + 2 * a2 + a3, (b1 + 2 * b2 + b3).sum(axis=0)
    else:
        s[4], bb = quad("Minv", vx, vx)
        b[4] = bb.sum(axis=0)
    return np.stack(s), GAMMA * U * np.stack(b)


def post_records(sums, dpn):
    """The records of post_finish from the five sums (float64, as the host computes them)."""
    s = np.asarray(sums, dtype=np.float64)
    n2 = s[0] + s[1] if dpn == 2 else s[4]
    nrm = np.sqrt(n2) + 1e-30
    inv2 = 1.0 / (nrm * nrm)
    return np.stack([nrm, s[4] * inv2, s[2] * inv2, s[3] * inv2, s[0] * inv2, s[1] * inv2], axis=1)


def sums_from_records(rec):
    """Back from the records (k, 6) to the five sums (5, k): s = record x norm^2."""
    n2 = rec[:, 0] ** 2
    return np.stack([rec[:, 4] * n2, rec[:, 5] * n2, rec[:, 2] * n2, rec[:, 3] * n2, rec[:, 1] * n2])


def residuals(pencil, lam, V):
    """||A v - lambda B v|| / ||A v|| over the interior rows, in extended precision.  V: (n2, k)."""
    AV, _ = pencil.apply("A", V)
    BV, _ = pencil.apply("B", V)
    R = AV - L(lam)[None, :] * BV
    return np.sqrt((R ** 2).sum(axis=0) / (AV ** 2).sum(axis=0))
