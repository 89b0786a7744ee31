"""The rule by which assembled CSR blocks of the device are held against the oracle's, shared by test_gpu_parity.py and
test_gpu_topology.py: slot by slot, |difference| <= 1e-13 x the sum over the contributing elements of the element's
largest entry."""
import numpy as np
import scipy.sparse as sp

SLOT_TOL = 1e-13


def abs_assembled(basis, N, name_terms):
    """Sum of |element entries| per CSR slot: the magnitude rounding errors are measured against."""
    ed = basis.element_dofs
    rows = np.broadcast_to(ed.T[:, :, None], (ed.shape[1], 6, 6)).ravel()
    cols = np.broadcast_to(ed.T[:, None, :], (ed.shape[1], 6, 6)).ravel()
    # per-element scale = largest entry of that element's matrices: inside a sliver element an entry
    # can be a cancelling sum of quadrature terms as large as the element's largest entry
    mag = sum(np.abs(t) for t in name_terms)
    mag = np.broadcast_to(mag.max(axis=(1, 2), keepdims=True), mag.shape)
    return sp.coo_matrix((mag.ravel(), (rows, cols)), shape=(N, N)).tocsr()


def check_blocks(ctx, sym, basis, refs):
    """refs: block name -> (reference matrix (N, N), element terms it is the sum of).  Returns the worst ratio
    |difference| / magnitude over all slots of all blocks."""
    N = sym.N
    rowptr, colind = sym.array("rowptr"), sym.array("colind")
    worst = 0.0
    for name, (R, terms) in refs.items():
        G = sp.csr_matrix((ctx.block_values(name), colind, rowptr), shape=(N, N))
        mag = abs_assembled(basis, N, terms)
        D = abs(G - R)
        D.eliminate_zeros()
        # |diff| <= 1e-13 * (sum over contributing elements of the element's largest entry), slot by slot
        viol = D - SLOT_TOL * mag
        assert viol.max() <= 0.0, (name, D.max(), mag.max())
        if D.nnz:
            D = D.tocoo()
            worst = max(worst, float((D.data / np.asarray(mag[D.row, D.col]).ravel()).max()))
    return worst


def vectorial_refs(A, Minv, Dxx, Dxy, Dyy, em, k0sq, N):
    """The eight blocks of the vectorial assembly (hfield.assemble_hfield_system_fused, hfield.element_matrices)."""
    return {
        "Axx": (A[:N, :N], [em["kxx"], em["div_xx"], k0sq * em["mass"]]),
        "Axy": (A[:N, N:], [em["kxy"], em["div_xy"]]),
        "Ayx": (A[N:, :N], [em["kyx"], em["div_xy"]]),
        "Ayy": (A[N:, N:], [em["kyy"], em["div_yy"], k0sq * em["mass"]]),
        "Minv": (Minv, [em["mass_eps_inv"]]), "Dxx": (Dxx, [em["div_xx"]]),
        "Dxy": (Dxy, [em["div_xy"]]), "Dyy": (Dyy, [em["div_yy"]]),
    }


def scalar_refs(K, M, Me, em, k0sq):
    """The two blocks of the scalar assembly (oracle.scalar): K - k0^2 M_eps in the Axx slot, M in the Minv slot."""
    return {"Axx": ((K - k0sq * Me).tocsr(), [em["stiff"], k0sq * em["eps_m"]]), "Minv": (M.tocsr(), [em["mass"]])}
