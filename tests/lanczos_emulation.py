"""Host references of the device kernels of the Lanczos drivers (csrc/kernels_lanczos.hip and the block SpMVs of
csrc/kernels_assembly.hip), restated in np.longdouble from the kernels' definitions, with the error bounds the GPU tests
hold them to and the mutation margins that show those tests would catch the cheapest plausible kernel mistakes.  Below
them, the two drivers themselves restated as one float64 function (lanczos_reference, with plantable driver mistakes), what
the driver tests measure on the state after a restart (restart_state) and the dense references of a converged solve.

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


# ---- the two drivers as one float64 function ---------------------------------------------------------------------------
RES_FLOOR = 3.7e-11         # floor of |theta| in the relative residual (ThickRestart::count_converged)
MISTAKES = ("residual_at_pk_plus_1", "first_step_two_blocks", "rotation_unsorted", "theta_not_written", "keep_k_minus_1")
# the first-cycle numbers of test_first_cycle_basis_and_projected_matrix: no post-restart tolerance goes below them
# (bv_kept, bv_new: |BV - B V| in units of that test's bound 4 GAMMA u |B| |V| + 64 u |B V|, so 1)
FIRST_CYCLE_TOL = {"orth": 1e-12, "relation": 1e-9, "symmetry": 1e-9, "outside_band": 1e-10, "bv_kept": 1.0, "bv_new": 1.0}
STATE_KEYS = ("orth", "relation", "symmetry", "outside_band", "bv_kept", "bv_new")
STATE_FACTOR = 10.0         # the GPU gets this many times what the float64 restatement shows (start block, summation orders)


class ShiftInvert:
    """OP = (A - sigma B)^-1 B on full-length vectors through SuperLU on the live rows (dead rows give 0)."""

    def __init__(self, A, B, sigma, live=None):
        import scipy.sparse as sp
        import scipy.sparse.linalg as spla
        self.B = sp.csr_matrix(B)
        self.n = self.B.shape[0]
        self.sigma = float(sigma)
        self.live = np.ones(self.n, dtype=bool) if live is None else np.asarray(live, dtype=bool)
        K = (sp.csr_matrix(A) - self.sigma * self.B).tocsc()[self.live][:, self.live]
        self.lu = spla.splu(K.tocsc())

    def __call__(self, X):
        X = np.asarray(X, dtype=np.float64)
        Y = np.zeros_like(X)
        Y[self.live] = self.lu.solve(np.ascontiguousarray(np.asarray(self.B @ X)[self.live]))
        return Y


def restart_pk(P, k, mm, nconv, mistake=None):
    """Columns ThickRestart::restart keeps: the k wanted pairs plus some of the next ones, leaving room for two blocks, but
    never fewer than min(k, mm - P)."""
    if mistake == "keep_k_minus_1":
        return k - 1
    pk = k + min(nconv, (mm - k) // 2)
    pk = max(pk, k + (mm - k) // 4)
    pk = min(pk, mm - 2 * P)
    return max(pk, min(k, mm - P))


def ritz_count(T, P, k, mm, tol):
    """Ritz pairs of the first mm columns (upper triangle of T authoritative) by decreasing |theta|, and the converged
    wanted ones: || R_m s[mm-P:mm] || <= tol max(|theta|, RES_FLOOR).  Returns theta, S, order, nconv, max_rel_res."""
    Tm = np.triu(T[:mm, :mm])
    Tm = Tm + np.triu(Tm, 1).T
    theta, S = np.linalg.eigh(Tm)
    order = np.argsort(-np.abs(theta), kind="stable")
    Rm = np.triu(T[mm:mm + P, mm - P:mm])
    nconv, worst = 0, 0.0
    for q in range(min(k, mm)):
        i = order[q]
        rel = np.linalg.norm(Rm @ S[mm - P:mm, i]) / max(abs(theta[i]), RES_FLOOR)
        worst = max(worst, rel)
        nconv += rel <= tol
    return theta, S, order, int(nconv), float(worst)


def lanczos_reference(P, op, k, ncv, tol, maxiter, V0, mistake=None, max_ncv=None, purify=True):
    """Thick-restart Lanczos of OP = op (a ShiftInvert) in the B inner product as csrc/api_device.hip runs it, in float64:
    P = 1 the single-vector driver (m = ncv columns, tested for convergence when the basis is full), P = BLOCK_P the block
    driver (m = ncv rounded up to a multiple of P, or down under max_ncv; tested after every step once mm >= k + P).
    CGS2 over the whole basis, CholQR of the new block; the pipelining and the held step are scheduling and left out.
    ``mistake`` plants one of MISTAKES.  V0: (n, P) start block (pushed through OP once, as the drivers do).
    B V is kept as the drivers keep it: (B W) R^-1 for a new block, rotated with V at a restart, never recomputed.
    The vectors of a converged run are purified as ThickRestart::finish purifies them (one step of inverse iteration:
    x + V[:, mm:mm+P] (R_m s[mm-P:mm]) / theta = OP x / theta); purify=False returns the plain Ritz vectors.
    Returns a dict: lam (the k wanted values, ascending), X (their vectors), V and BV (n, m + P + 1), T (the host's projected
    matrix, ld = m + P), Hcols (what the device buffer holds: the columns before the last pk zero), pks, mm, nconv,
    restarts, n_op, max_rel_res."""
    assert mistake in (None,) + MISTAKES
    B, n = op.B, op.n
    m = ncv if P == 1 else -(-ncv // P) * P
    if max_ncv is not None and m > max_ncv:
        m = (max_ncv // P) * P
    ld = m + P
    V = np.zeros((n, ld + 1))
    T = np.zeros((ld, ld))

    BV = np.zeros((n, ld + 1))

    def cholqr(W):
        BW = np.asarray(B @ W)
        R = np.linalg.cholesky(W.T @ BW).T
        return np.linalg.solve(R.T, W.T).T, np.linalg.solve(R.T, BW.T).T, R

    V[:, :P], BV[:, :P], _ = cholqr(op(np.asarray(V0, dtype=np.float64).reshape(n, P)))
    n_op = P
    c0, cycle_start, pks, restarts = 0, -1, [], 0
    while True:
        mm, done = c0, False
        while c0 + P <= m:
            nc = c0 + P
            W = op(V[:, c0:nc])
            n_op += P
            lo = max(0, nc - 2 * P) if (mistake == "first_step_two_blocks" and c0 == cycle_start) else 0
            H = np.zeros((nc, P))
            for _ in range(2):
                h = BV[:, lo:nc].T @ W
                W = W - V[:, lo:nc] @ h
                H[lo:] += h
            T[:nc, c0:nc] = H
            V[:, nc:nc + P], BV[:, nc:nc + P], T[nc:nc + P, c0:nc] = cholqr(W)
            c0 = mm = nc
            if P > 1 and mm >= k + P and c0 + P <= m:
                theta, S, order, nconv, worst = ritz_count(T, P, k, mm, tol)
                if nconv >= k:
                    done = True
                    break
        if not done:
            theta, S, order, nconv, worst = ritz_count(T, P, k, mm, tol)
        if nconv >= k or restarts >= maxiter:
            break
        pk = restart_pk(P, k, mm, nconv, mistake)
        keep = np.arange(pk) if mistake == "rotation_unsorted" else order[:pk]
        at = pk + 1 if mistake == "residual_at_pk_plus_1" else pk
        for X in (V, BV):
            Xn = np.zeros_like(X)
            Xn[:, :pk] = X[:, :mm] @ S[:, keep]
            if at != pk:
                Xn[:, pk] = X[:, pk]            # what the double buffer held there: a unit vector of an earlier basis
            Xn[:, at:at + P] = X[:, mm:mm + P]
            X[:] = Xn
        T[:] = 0.0
        if mistake != "theta_not_written":
            T[np.arange(pk), np.arange(pk)] = theta[order[:pk]]
        pks.append(pk)
        restarts += 1
        c0 = cycle_start = pk
    want = order[:k]
    lam = op.sigma + 1.0 / theta[want]
    o = np.argsort(lam)
    Hcols = T.copy()
    if pks:
        Hcols[:, :pks[-1]] = 0.0
    X = V[:, :mm] @ S[:, want[o]]
    Rm = np.triu(T[mm:mm + P, mm - P:mm])
    if purify and nconv >= k and (np.diag(Rm) > 0).all():
        X = X + V[:, mm:mm + P] @ ((Rm @ S[mm - P:mm, want[o]]) / theta[want[o]])
    return {"lam": lam[o], "X": X, "V": V, "BV": BV, "T": T, "Hcols": Hcols, "pks": pks, "mm": mm, "m": m,
            "nconv": nconv, "restarts": restarts, "n_op": n_op, "max_rel_res": worst}


def restart_state(V, Hcols, P, k, m, op, BV=None):
    """What the tests of the state after a restart measure on the basis V (n, >= m + P) and the device's projected columns
    Hcols (ld, ld), ld = m + P, T[i, j] = Hcols[i, j]: a dict with
    pk, mm        the first non-zero column and the columns the last cycle filled;
    structure     names of the exact properties that fail (pk range, a gap in the written columns, an R block not upper
                  triangular with a positive diagonal, a written entry below an R block, a zero in rows 0 .. pk of the
                  first block after the restart);
    orth          max |V^T B V - I| over the mm + P columns;
    relation      || OP V_mm - V_{mm+P} T || / || OP V_mm ||, T completed in the kept columns by symmetry (rows pk .. pk + P)
                  and the Rayleigh quotients v_q^T B OP v_q;
    symmetry      max |T[c0-P:c0, c0:c0+P] - R^T| / max |T| over the blocks after the first;
    outside_band  max |T[:c0-P, c0:c0+P]| / max |T| over the same blocks;
    bv_kept, bv_new  (with BV) the largest |BV - B V| over the live rows in units of 4 GAMMA u |B| |V| + 64 u |B V|, the bound of
                  the first-cycle test, over the kept columns (rotated with V, not recomputed: where a Ritz vector is small
                  next to the basis vectors it was combined from, the rotation's own rounding u |BV| |S| exceeds a bound
                  made of |B| |V| of the result) and over the columns from pk on (products of this and the last cycle)."""
    ld = m + P
    Hc = np.asarray(Hcols, dtype=np.float64)[:ld, :ld]
    nzcol = np.nonzero(np.any(Hc != 0, axis=0))[0]
    bad = []
    pk = int(nzcol[0]) if nzcol.size else 0
    if not (nzcol.size and k <= pk <= m - 2 * P):
        return dict({q: np.inf for q in STATE_KEYS}, pk=pk, mm=0, structure=["pk_range"])
    mm = pk + P * ((m - pk) // P)
    if not np.array_equal(nzcol, np.arange(pk, mm)):
        bad.append("written_columns")
    B = op.B
    Vc = np.asarray(V, dtype=np.float64)[:, :mm + P]
    orth = float(np.abs(Vc.T @ (B @ Vc) - np.eye(mm + P)).max())
    OPV = op(Vc[:, :mm])
    T = Hc[:mm + P, :mm].copy()
    T[pk:pk + P, :pk] = Hc[:pk, pk:pk + P].T
    T[np.arange(pk), np.arange(pk)] = np.einsum("ij,ij->j", Vc[:, :pk], np.asarray(B @ OPV[:, :pk]))
    relation = float(np.linalg.norm(OPV - Vc @ T) / np.linalg.norm(OPV))
    Tn = float(np.abs(T).max())
    if not (Hc[:pk + P, pk:pk + P] != 0).all():
        bad.append("first_block_full")
    sym = out = 0.0
    for c0 in range(pk, mm, P):
        R = Hc[c0 + P:c0 + 2 * P, c0:c0 + P]
        if not (np.array_equal(R, np.triu(R)) and (np.diag(R) > 0).all()):
            bad.append(f"R_upper_positive@{c0}")
        if (Hc[c0 + 2 * P:, c0:c0 + P] != 0).any():
            bad.append(f"below_R@{c0}")
        if c0 > pk:
            sym = max(sym, float(np.abs(Hc[c0 - P:c0, c0:c0 + P] - Hc[c0:c0 + P, c0 - P:c0].T).max()) / Tn)
            out = max(out, float(np.abs(Hc[:c0 - P, c0:c0 + P]).max()) / Tn)
    res = {"pk": pk, "mm": mm, "structure": bad, "orth": orth, "relation": relation, "symmetry": sym, "outside_band": out,
           "bv_kept": 0.0, "bv_new": 0.0}
    if BV is not None:
        ref = np.asarray(B @ Vc)
        bound = 4 * GAMMA * U * np.asarray(abs(B) @ np.abs(Vc)) + 64 * U * np.abs(ref)
        d = np.abs(np.asarray(BV, dtype=np.float64)[:, :mm + P] - ref)[op.live]
        if not np.isfinite(d).all():
            bad.append("BV_finite")
        ratio = np.where(d > 0, d / np.maximum(bound[op.live], 1e-300), 0.0)
        res["bv_kept"], res["bv_new"] = float(ratio[:, :pk].max()), float(ratio[:, pk:].max())
    return res


def state_tolerances(ref_state):
    """STATE_FACTOR times what the restatement shows on the same pencil, never below the first-cycle numbers."""
    return {q: max(STATE_FACTOR * ref_state[q], FIRST_CYCLE_TOL[q]) for q in STATE_KEYS}


def state_vector(st):
    """The measured quantities and the count of failed exact properties as one vector (for margins / assert_margins; the
    count has a zero bound: any failure is an infinite margin)."""
    return np.array([min(st[q], 1e200) for q in STATE_KEYS] + [float(len(st["structure"]))])


# ---- dense references of a converged solve -----------------------------------------------------------------------------
def triple_mesh(p, t, cores, shifts=(0.0, 2.0, 4.0)):
    """Copies of one mesh (p (2, nv), t (3, ne)) shifted in x, node numbers offset, the cores shifted along: a block
    diagonal pencil whose every eigenvalue appears len(shifts) times up to the rounding of the shifted coordinates."""
    p, t, cores = np.asarray(p, dtype=np.float64), np.asarray(t), np.asarray(cores, dtype=np.float64).reshape(-1, 3)
    nv = p.shape[1]
    ps = np.hstack([p + np.array([[s], [0.0]]) for s in shifts])
    ts = np.hstack([t + i * nv for i in range(len(shifts))]).astype(t.dtype)
    cs = np.vstack([cores + np.array([s, 0.0, 0.0]) for s in shifts])
    return ps, ts, cs


def dense_reference(A, B, live, sigma):
    """All eigenpairs of the live rows of the pencil, one scipy.linalg.eigh per connected component of the pattern, sorted
    by decreasing |1 / (lambda - sigma)|: (lam, X (n, nlive), ncomponents); X is B-orthonormal, dead rows 0."""
    import scipy.linalg as sl
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    live = np.nonzero(np.asarray(live, dtype=bool))[0]
    Al = sp.csr_matrix(A)[live][:, live]
    Bl = sp.csr_matrix(B)[live][:, live]
    ncomp, lab = connected_components(abs(Al) + abs(Bl), directed=False)
    lam, X = [], np.zeros((A.shape[0], live.size))
    at = 0
    for cpt in range(ncomp):
        idx = np.nonzero(lab == cpt)[0]
        a = Al[idx][:, idx].toarray()
        b = Bl[idx][:, idx].toarray()
        w, x = sl.eigh((a + a.T) / 2, (b + b.T) / 2)
        lam.append(w)
        X[live[idx], at:at + w.size] = x
        at += w.size
    lam = np.concatenate(lam)
    o = np.argsort(-np.abs(1.0 / (lam - sigma)), kind="stable")
    return lam[o], X[:, o], ncomp


def theta_bound(theta_ref, tol):
    """|theta - theta_ref| <= 2 tol |theta_ref| + 64 u max |theta|: the residual bounds a Ritz value's error for a symmetric
    operator (the driver's contract, factor 2), plus rounding."""
    theta_ref = np.asarray(theta_ref, dtype=np.float64)
    return 2 * tol * np.abs(theta_ref) + 64 * U * np.abs(theta_ref).max()


def wanted_interval(lam_sorted_all, lam_wanted_sorted):
    """First index of the wanted values in the ascending spectrum (they are an interval of it: the nearest to sigma; equal
    copies of a cut cluster at its lower end make the place of the smallest value ambiguous, so every candidate is tried)."""
    lam, w = np.asarray(lam_sorted_all), np.asarray(lam_wanted_sorted)
    for lo in range(int(np.searchsorted(lam, w[0], "left")), int(np.searchsorted(lam, w[0], "right"))):
        if np.array_equal(lam[lo:lo + w.size], w):
            return lo
    raise AssertionError("the wanted values are no interval of the spectrum")


def whole_clusters(lam_sorted_all, lo, hi, rel_gap):
    """Boolean mask over [lo, hi) of an ascending spectrum: True where the cluster of the value (consecutive values closer
    than rel_gap |lambda|, the rule of oracle/compare.py) lies wholly inside [lo, hi)."""
    lam = np.asarray(lam_sorted_all)
    close = np.abs(np.diff(lam)) < rel_gap * np.abs(lam[1:])         # close[i]: lam[i] and lam[i + 1] in one cluster
    cid = np.concatenate([[0], np.cumsum(~close)])
    inside = (cid >= (cid[lo - 1] + 1 if lo > 0 else 0)) & (cid <= (cid[hi] - 1 if hi < lam.size else cid[-1]))
    return inside[lo:hi]
