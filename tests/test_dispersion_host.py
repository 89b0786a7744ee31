"""Group index and k0-derivative coupling, host side (no GPU): the NumPy emulation of the Gram kernel against the oracle's
assembled blocks, Hellmann-Feynman from emulated Grams against finite differences of oracle eigen-solves (vectorial and
scalar, with and without material dispersion), an exactly degenerate toy pencil, and argument checking before any device
call."""
import copy
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import eigsh

from gram_emulation import GramEmulation
from oracle import hfield, scalar
from pl_fem_vectoriel_amd import _native, generate_mesh, mode_dispersion
from pl_fem_vectoriel_amd.dispersion import deps_dk0, dispersion_from_grams


@pytest.fixture(scope="module")
def lantern(c1_geometry, built_library):
    mesh = generate_mesh(c1_geometry, 0.5, 0)
    return mesh, GramEmulation(mesh.p, mesh.t)


def _geom(g, k0=None, n_core=None, n_clad=None):
    h = copy.copy(g)
    if k0 is not None:
        h.k0, h.wavelength = k0, 2 * np.pi / k0
    if n_core is not None:
        h.n_core = n_core
    if n_clad is not None:
        h.n_clad = n_clad
    return h


def _csr(d, ed, N):
    rows = np.broadcast_to(ed.T[:, :, None], (ed.shape[1], 6, 6)).ravel()
    cols = np.broadcast_to(ed.T[:, None, :], (ed.shape[1], 6, 6)).ravel()
    return sp.coo_matrix((d.ravel(), (rows, cols)), shape=(N, N)).tocsr()


def _vec_blocks(g, em):
    """Interior-restricted 2N_s x 2N_s blocks K = [[Kxx, Kxy], [Kyx, Kyy]], D, M and M_(1/eps) of the oracle."""
    e = hfield.element_matrices(g, em.basis)
    ed, N, it = em.basis.element_dofs, em.N, em.interior
    m = {nm: _csr(v, ed, N)[it][:, it] for nm, v in e.items()}
    K = sp.bmat([[m["kxx"], m["kxy"]], [m["kyx"], m["kyy"]]]).tocsr()
    D = sp.bmat([[m["div_xx"], m["div_xy"]], [m["div_xy"].T, m["div_yy"]]]).tocsr()
    M = sp.block_diag([m["mass"], m["mass"]]).tocsr()
    Mi = sp.block_diag([m["mass_eps_inv"], m["mass_eps_inv"]]).tocsr()
    return K, D, M, Mi


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_emulated_grams_reproduce_the_assembled_blocks(lantern, c1_geometry):
    mesh, em = lantern
    g = c1_geometry
    rng = np.random.default_rng(11)
    k = 5
    vals = rng.standard_normal((2, k, em.interior.size))
    G = em.grams(vals, True, g)
    V = np.hstack([vals[0], vals[1]]).T                               # (2 N_s, k)
    ec, el = g.n_core ** 2, g.n_clad ** 2
    # K and M_(1/eps) are linear in 1/eps_r: (eps_core, eps_clad) = (1, inf) and (inf, 1) give each region alone
    Kc, D, M, Mc = _vec_blocks(_geom(g, n_core=1.0, n_clad=np.inf), em)
    Kl, _, _, Ml = _vec_blocks(_geom(g, n_core=np.inf, n_clad=1.0), em)
    for nm, X in (("K_core", Kc), ("K_clad", Kl), ("M_core", Mc), ("M_clad", Ml), ("D", D)):
        assert _rel(G[nm], V.T @ (X @ V)) <= 1e-12, nm
    assert _rel(G["M_core"] + G["M_clad"], V.T @ (M @ V)) <= 1e-12
    # the whole pencil of the solver
    A, B, basis, *_ = hfield.assemble_hfield_system_fused(g, em.mesh)
    A, B, _ = hfield.restrict_interior(A, B, basis)
    a = G["K_core"] / ec + G["K_clad"] / el + G["D"] - g.k0 ** 2 * (G["M_core"] + G["M_clad"])
    assert _rel(a, V.T @ (A @ V)) <= 1e-12
    assert _rel(G["M_core"] / ec + G["M_clad"] / el, V.T @ (B @ V)) <= 1e-12

    u = rng.standard_normal((1, k, em.N))
    Gs = em.grams(u, False, g)
    # M_eps is linear in eps_r: (1, 0) and (0, 1)
    S, Mm, Mcs, _ = scalar.assemble(_geom(g, n_core=1.0, n_clad=0.0), em.mesh)
    _, _, Mls, _ = scalar.assemble(_geom(g, n_core=0.0, n_clad=1.0), em.mesh)
    U = u[0].T
    for nm, X in (("M_core", Mcs), ("M_clad", Mls), ("S", S)):
        assert _rel(Gs[nm], U.T @ (X @ U)) <= 1e-12, nm
    assert _rel(Gs["M_core"] + Gs["M_clad"], U.T @ (Mm @ U)) <= 1e-12


def _vec_solve(g, em, sigma, k):
    A, B, basis, *_ = hfield.assemble_hfield_system_fused(g, em.mesh)
    A, B, _ = hfield.restrict_interior(A, B, basis)
    w, X = eigsh(A, k=k, M=B, sigma=sigma, which="LM", tol=1e-14)
    return w, X


def _scal_solve(g, em, sigma, k):
    S, M, Me, _ = scalar.assemble(g, em.mesh)
    w, X = eigsh((S - g.k0 ** 2 * Me).tocsr(), k=k, M=M, sigma=sigma, which="LM", tol=1e-14)
    return w, X


def _fd_check(kind, g, em, dn, delta=1e-5, k=12):
    """n_g from emulated Grams at k0 against central differences of solves at k0 (1 +- delta); returns the worst
    |n_g(HF) - n_g(FD)| over the modes matched uniquely and well separated, and how many there were."""
    k0 = g.k0
    lam0 = 2 * np.pi / k0

    def at(kk):
        dl = 2 * np.pi / kk - lam0
        return _geom(g, k0=kk, n_core=g.n_core + dn[0] * dl, n_clad=g.n_clad + dn[1] * dl)

    solve = _vec_solve if kind == "vectorial" else _scal_solve
    sigma = hfield.shift_estimate(g) if kind == "vectorial" else scalar.shift(g)
    w0, X0 = solve(g, em, sigma, k)
    wp, Xp = solve(at(k0 * (1 + delta)), em, sigma, k)
    wm, Xm = solve(at(k0 * (1 - delta)), em, sigma, k)
    sgn = 1.0 if kind == "vectorial" else -1.0
    keep = sgn * w0 > 0
    w0, X0 = w0[keep], X0[:, keep]
    beta = np.sqrt(sgn * w0)
    if kind == "vectorial":
        ns = em.interior.size
        vals = np.stack([X0[:ns].T, X0[ns:].T])
    else:
        vals = X0.T[None]
    G = em.grams(vals, kind == "vectorial", g)
    res = dispersion_from_grams(kind, G, beta, k0, (g.n_core ** 2, g.n_clad ** 2),
                                (deps_dk0(g.n_core, k0, dn[0]), deps_dk0(g.n_clad, k0, dn[1])))
    assert res["rayleigh_defect"].max() <= 1e-10
    h = 2 * delta * k0
    x = X0 / np.linalg.norm(X0, axis=0)

    def match(w, X):                                    # eigenvalue of the unique |cos| > 0.999 partner, else nan
        c = np.abs(x.T @ X) / np.linalg.norm(X, axis=0)[None]
        return np.array([w[np.argmax(r)] if (r > 0.999).sum() == 1 else np.nan for r in c])

    mp, mm = match(wp, Xp), match(wm, Xm)
    errs = []
    for i in range(beta.size):
        # separation: the nearest neighbour's gap must exceed 100 x what the shift changes it by (the whole spectrum
        # moves by far more than its spacing; the modes' relative motion is what could mix them)
        j = np.argsort(np.abs(w0 - w0[i]))[1]
        moved = max(abs((mp[i] - mp[j]) - (w0[i] - w0[j])), abs((mm[i] - mm[j]) - (w0[i] - w0[j])))
        if not np.isfinite(moved) or abs(w0[i] - w0[j]) < 100 * moved:
            continue
        fd = (np.sqrt(sgn * mp[i]) - np.sqrt(sgn * mm[i])) / h
        errs.append(abs(res["n_g"][i] - fd))
    return max(errs), len(errs), res


@pytest.mark.parametrize("kind", ["vectorial", "scalar"])
@pytest.mark.parametrize("dn", [(0.0, 0.0), (-0.0118, -0.0102)])
def test_hellmann_feynman_matches_finite_differences(lantern, c1_geometry, kind, dn):
    _, em = lantern
    err, n, res = _fd_check(kind, c1_geometry, em, dn)
    print(f"{kind} dn={dn}: {n} modes compared, worst |n_g(HF) - n_g(FD)| = {err:.2e}, n_g {res['n_g'].min():.6f}.."
          f"{res['n_g'].max():.6f}")
    assert n >= 3
    assert err <= 1e-6
    if dn == (0.0, 0.0):
        c = res["coupling"]
        assert np.array_equal(c, -c.T)                               # B' = 0: exactly antisymmetric


def test_bulk_material_gives_the_textbook_group_index():
    # scalar pencil, one material, a field without transverse variation (S = 0): a plane wave in bulk material
    k0, n, dn = 2 * np.pi / 1.55, 1.444, -0.0118
    eps = n * n
    G = {"M_core": np.zeros((1, 1)), "M_clad": np.ones((1, 1)), "S": np.zeros((1, 1))}
    res = dispersion_from_grams("scalar", G, np.array([k0 * n]), k0, (eps, eps), (0.0, deps_dk0(n, k0, dn)))
    assert res["n_g"][0] == pytest.approx(n - 1.55 * dn, rel=1e-14)
    assert res["group_delay_ps_per_m"][0] == pytest.approx(res["n_g"][0] / 299792458.0 * 1e12, rel=1e-15)


def _toy(seed=5, n=8):
    """A dense vectorial-form pencil with an exact double eigenvalue at k0: the Grams of all its eigenvectors."""
    rng = np.random.default_rng(seed)
    k0, ec, el = 4.0, 2.2, 2.0

    def spd():
        a = rng.standard_normal((n, n))
        return a @ a.T + n * np.eye(n)

    def sym():
        a = rng.standard_normal((n, n))
        return a + a.T

    Mc, Ml, Kc, Kl = spd(), spd(), sym(), sym()
    B = Mc / ec + Ml / el
    L = np.linalg.cholesky(B)
    Wt = np.linalg.qr(rng.standard_normal((n, n)))[0]
    W = np.linalg.solve(L.T, Wt)                                      # W^T B W = I
    lam = np.array([10.0, 12.0, 15.0, 15.0, 18.0, 21.0, 25.0, 30.0])
    A0 = B @ W @ np.diag(lam) @ W.T @ B
    D = A0 - Kc / ec - Kl / el + k0 ** 2 * (Mc + Ml)
    mats = {"M_core": Mc, "M_clad": Ml, "K_core": Kc, "K_clad": Kl, "D": D}

    def pencil(kk):
        return Kc / ec + Kl / el + D - kk ** 2 * (Mc + Ml), B

    c, s = np.cos(0.7), np.sin(0.7)
    W[:, 2:4] = W[:, 2:4] @ np.array([[c, -s], [s, c]])                  # an arbitrary basis of the double eigenspace
    return k0, (ec, el), mats, pencil, W, lam


def _eig(A, B):
    L = np.linalg.cholesky(B)
    Li = np.linalg.inv(L)
    w, Y = np.linalg.eigh(Li @ A @ Li.T)
    return w, Li.T @ Y


def test_degenerate_toy_pencil_cluster_against_finite_differences():
    k0, eps, mats, pencil, W, lam = _toy()
    G = {nm: W.T @ X @ W for nm, X in mats.items()}
    res = dispersion_from_grams("vectorial", G, np.sqrt(lam), k0, eps, cluster_rtol=1e-10, alpha_p=1.0)
    assert res["cluster"].tolist() == [-1, -1, 0, 0, -1, -1, -1, -1]
    assert res["rayleigh_defect"].max() <= 1e-12
    h = 1e-5
    wp, Xp = _eig(*pencil(k0 + h))
    wm, Xm = _eig(*pencil(k0 - h))
    # the split pair: ascending one-sided slopes from each side, averaged (second order)
    sp_ = np.sort((wp[2:4] - 15.0) / h)
    sm_ = np.sort((15.0 - wm[2:4]) / h)
    fd_dmu = 0.5 * (sp_ + sm_)
    beta = np.sqrt(lam)
    assert np.allclose(res["n_g"][2:4], fd_dmu / (2 * beta[2:4]), rtol=0, atol=1e-7)
    for i in (0, 1, 4, 5, 6, 7):
        assert res["n_g"][i] == pytest.approx((np.sqrt(wp[i]) - np.sqrt(wm[i])) / (2 * h), abs=1e-8)
    # the rotation: the adapted vectors are the limits of the split eigenvectors
    Y = res["cluster_rotation"][0]
    adapted = W[:, 2:4] @ Y
    B = pencil(k0)[1]
    ov = np.abs(adapted.T @ B @ Xp[:, 2:4])
    assert np.abs(ov - np.eye(2)).max() <= 1e-4
    # coupling between singletons: h_m^T B dh_n/dk0 from differences of B-normalised, sign-aligned eigenvectors
    c = res["coupling"]
    for n in (0, 1, 4, 5):
        xp = Xp[:, n] * np.sign(Xp[:, n] @ B @ W[:, n])
        xm = Xm[:, n] * np.sign(Xm[:, n] @ B @ W[:, n])
        d = (xp - xm) / (2 * h)
        for m in (0, 1, 4, 5, 6, 7):
            if m != n:
                assert c[m, n] == pytest.approx(W[:, m] @ B @ d, abs=1e-7)
    assert (c[2:4, 2:4] == np.diag(np.diag(c[2:4, 2:4]))).all()       # in-cluster entries 0
    assert np.array_equal(c, -c.T)


def test_argument_errors_before_any_device_call(lantern, c1_geometry):
    mesh, em = lantern
    ns = em.interior.size
    good = [{"Ex_dofs": np.ones(ns), "Ey_dofs": np.ones(ns), "beta": 8.0}]
    scal = [{"field_vector": np.ones(em.N), "beta": 8.0}]
    with pytest.raises(ValueError):
        mode_dispersion(good + scal, mesh, c1_geometry)                  # mixed kinds
    with pytest.raises(ValueError):
        mode_dispersion([{"Ex_dofs": np.ones(ns - 1), "Ey_dofs": np.ones(ns - 1), "beta": 8.0}], mesh, c1_geometry)
    for b in (None, np.nan, np.inf, 0.0, -1.0):
        rec = {"Ex_dofs": np.ones(ns), "Ey_dofs": np.ones(ns)}
        if b is not None:
            rec["beta"] = b
        with pytest.raises(ValueError):
            mode_dispersion([rec], mesh, c1_geometry)
    for dn in ((0.0,), (0.0, 0.0, 0.0), (np.nan, 0.0), "ab", None):
        with pytest.raises(ValueError):
            mode_dispersion(good, mesh, c1_geometry, dn_dlambda=dn)
    many = _geom(c1_geometry)
    many.positions = np.zeros((65, 2))
    many.core_radii = np.ones(65)
    with pytest.raises(ValueError):
        mode_dispersion(good, mesh, many)
    with pytest.raises(ValueError):
        mode_dispersion([], mesh, c1_geometry)


def test_gram_work_bytes_on_the_host(built_library):
    lib = _native.load_library()
    b = ctypes.c_int64(0)
    assert lib.plfem_gram_work_bytes(2, 22, ctypes.byref(b)) == _native.PLFEM_OK
    v22 = b.value
    assert v22 >= 5 * 22 * 22 * 8 and v22 % 8 == 0
    assert lib.plfem_gram_work_bytes(1, 22, ctypes.byref(b)) == _native.PLFEM_OK
    assert 0 < b.value < v22                                           # three outputs instead of five
    assert lib.plfem_gram_work_bytes(2, 33, ctypes.byref(b)) == _native.PLFEM_OK
    assert b.value > 3 * v22                                           # 2 x 2 chunk pairs
    for nc, k in ((2, 0), (2, -1), (0, 5), (3, 5)):
        assert lib.plfem_gram_work_bytes(nc, k, ctypes.byref(b)) == _native.PLFEM_EINVAL
    assert lib.plfem_gram_work_bytes(2, 5, None) == _native.PLFEM_EINVAL
    assert lib.plfem_mode_grams(None, 2, 5, None, 1, None, 0, None, 0, None) == _native.PLFEM_EINVAL
