"""Per-core Grams and what is built from them, host side (no GPU): the NumPy emulation of the per-core Gram call against the
oracle's assembled pencil with unequal core indices, Hellmann-Feynman d n_eff / d n_c against central differences of oracle
eigen-solves, the scalar identity with the power map, the second order of the Rayleigh-Ritz values, an exactly degenerate
toy pencil, ownership on overlapping discs and on core-boundary ties, and argument checking before any device call."""
import copy
import ctypes

import numpy as np
import pytest

from core_gram_emulation import CoreGramEmulation
from core_ties import Ties, jittered_square_mesh, ref_inside
from oracle import hfield, scalar
from pl_fem_vectoriel_amd import (ModeFields, PhotonicLanternGeometry, _native, core_decomposition,
                                  core_quantities_from_grams, generate_mesh)
from test_dispersion_host import _eig, _rel, _scal_solve, _vec_solve

POS = np.array([[0.0, 0.0], [5.0, 0.0], [-2.5, 4.33]])
RAD = np.array([1.5, 1.3, 1.1])
DN = np.array([1e-3, -2e-3, 5e-4])


@pytest.fixture(scope="module")
def three(built_library):
    """Three unequal cores, n = 1.535 / 1.0 at 1.55 um, on generate_mesh(g, 0.5, 0)."""
    g = PhotonicLanternGeometry(3, "triangular_3", POS, RAD, 1.535, 1.0, wavelength=1.55)
    mesh = generate_mesh(g, 0.5, 0)
    em = CoreGramEmulation(mesh.p, mesh.t)
    assert em.N == 8156 and mesh.t.shape[1] == 4055
    return g, mesh, em


def het(g, n_by_core):
    """A duck geometry: g with core c at index n_by_core[c] (later discs overwrite earlier ones, as in g.epsilon)."""
    h = copy.copy(g)
    n = np.asarray(n_by_core, dtype=np.float64)

    def epsilon(x, y):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        eps = np.full_like(x, g.n_clad ** 2, dtype=np.complex128)
        for (cx, cy), r, nc in zip(g.positions, g.core_radii, n):
            eps[(x - cx) ** 2 + (y - cy) ** 2 <= r ** 2] = nc ** 2
        return eps

    h.epsilon = epsilon
    return h


def test_emulated_core_grams_reproduce_the_heterogeneous_pencil(three):
    g, mesh, em = three
    rng = np.random.default_rng(21)
    k = 5
    n = np.array([1.535, 1.50, 1.56])
    e, el, k0 = n ** 2, g.n_clad ** 2, g.k0
    h = het(g, n)

    vals = rng.standard_normal((2, k, em.interior.size))
    G, C = em.grams(vals, True, g), em.core_grams(vals, True, g)
    assert C["points"].sum() == em.core_mask(g).sum() and (C["points"] > 0).all()
    V = np.hstack([vals[0], vals[1]]).T
    A, B, basis, *_ = hfield.assemble_hfield_system_fused(h, em.mesh)
    A, B, _ = hfield.restrict_interior(A, B, basis)
    a = np.tensordot(1 / e, C["K"], 1) + G["K_clad"] / el + G["D"] - k0 ** 2 * (G["M_core"] + G["M_clad"])
    b = np.tensordot(1 / e, C["Mx"] + C["My"], 1) + G["M_clad"] / el
    ea, eb = _rel(a, V.T @ (A @ V)), _rel(b, V.T @ (B @ V))
    print(f"vectorial: V^T A_het V {ea:.1e}, V^T B_het V {eb:.1e}")
    assert ea <= 1e-12 and eb <= 1e-12
    assert _rel((C["Mx"] + C["My"]).sum(0), G["M_core"]) <= 1e-12
    assert _rel(C["K"].sum(0), G["K_core"]) <= 1e-12

    u = rng.standard_normal((1, k, em.N))
    Gs, Cs = em.grams(u, False, g), em.core_grams(u, False, g)
    assert np.array_equal(Cs["points"], C["points"])
    S, Mm, Me, _ = scalar.assemble(h, em.mesh)
    U = u[0].T
    a = Gs["S"] - k0 ** 2 * (np.tensordot(e, Cs["M"], 1) + el * Gs["M_clad"])
    es = _rel(a, U.T @ ((S - k0 ** 2 * Me) @ U))
    print(f"scalar: V^T A_het V {es:.1e}")
    assert es <= 1e-12
    assert _rel(Gs["M_core"] + Gs["M_clad"], U.T @ (Mm @ U)) <= 1e-12
    assert _rel(Cs["M"].sum(0), Gs["M_core"]) <= 1e-12


def _base(kind, g, em, k):
    """Oracle modes of the homogeneous geometry: eigenvalues, vectors, beta, the DOF values as the emulation takes them."""
    solve = _vec_solve if kind == "vectorial" else _scal_solve
    sigma = hfield.shift_estimate(g) if kind == "vectorial" else scalar.shift(g)
    sgn = 1.0 if kind == "vectorial" else -1.0
    w0, X0 = solve(g, em, sigma, k)
    keep = sgn * w0 > 0
    w0, X0 = w0[keep], X0[:, keep]
    if kind == "vectorial":
        ns = em.interior.size
        vals = np.stack([X0[:ns].T, X0[ns:].T])
    else:
        vals = X0.T[None]
    return solve, sigma, sgn, w0, X0, np.sqrt(sgn * w0), vals


def _quantities(kind, g, em, vals, beta, **kw):
    indexed = kind == "vectorial"
    return core_quantities_from_grams(kind, em.core_grams(vals, indexed, g), em.grams(vals, indexed, g), beta, g.k0,
                                      (g.n_core ** 2, g.n_clad ** 2), **kw)


@pytest.fixture(scope="module")
def scalar_base(three):
    g, mesh, em = three
    return _base("scalar", g, em, 10)


@pytest.fixture(scope="module")
def vectorial_base(three):
    g, mesh, em = three
    return _base("vectorial", g, em, 12)


@pytest.fixture(scope="module")
def hellmann_feynman(three, scalar_base, vectorial_base):
    """Per kind: the base solve and the quantities from emulated Grams, computed once for the three cores' cases."""
    g, mesh, em = three
    out = {}
    for kind, base in (("vectorial", vectorial_base), ("scalar", scalar_base)):
        out[kind] = base, _quantities(kind, g, em, base[-1], base[-2])
    return out


@pytest.mark.parametrize("core", [0, 1, 2])
@pytest.mark.parametrize("kind", ["vectorial", "scalar"])
def test_dneff_dn_matches_central_differences_of_oracle_solves(three, hellmann_feynman, kind, core):
    g, mesh, em = three
    delta = 1e-5
    (solve, sigma, sgn, w0, X0, beta, vals), res = hellmann_feynman[kind]
    assert res["rayleigh_defect"].max() <= 1e-10
    x = X0 / np.linalg.norm(X0, axis=0)

    def match(w, X):                                    # eigenvalue of the unique |cos| > 0.999 partner, else nan
        c = np.abs(x.T @ X) / np.linalg.norm(X, axis=0)[None]
        return np.array([w[np.argmax(r)] if (r > 0.999).sum() == 1 else np.nan for r in c])

    n = np.full(3, g.n_core)
    n[core] += delta
    mp = match(*solve(het(g, n), em, sigma, w0.size))
    n[core] -= 2 * delta
    mm = match(*solve(het(g, n), em, sigma, w0.size))
    errs = []
    for i in range(beta.size):
        # separation: the nearest neighbour's gap must exceed 100 x what the shift changes it by
        j = np.argsort(np.abs(w0 - w0[i]))[1]
        moved = max(abs((mp[i] - mp[j]) - (w0[i] - w0[j])), abs((mm[i] - mm[j]) - (w0[i] - w0[j])))
        if not np.isfinite(moved) or abs(w0[i] - w0[j]) < 100 * moved:
            continue
        fd = (np.sqrt(sgn * mp[i]) - np.sqrt(sgn * mm[i])) / (2 * delta * g.k0)
        errs.append(abs(res["dneff_dn"][i, core] - fd))
    print(f"{kind} core {core}: {len(errs)} of {beta.size} modes compared, worst |HF - FD| = {max(errs):.2e}")
    assert len(errs) >= beta.size - 2                   # at most two modes of a core may be left out
    assert max(errs) <= 1e-6


def test_scalar_sensitivity_is_the_power_map(three, scalar_base):
    g, mesh, em = three
    *_, beta, vals = scalar_base
    res = _quantities("scalar", g, em, vals, beta)
    assert (res["cluster"] == -1).all()
    ref = (g.n_core / (beta / g.k0))[:, None] * res["power"]
    assert np.abs(res["dneff_dn"] - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.abs(res["power"].sum(1) + res["power_clad"] - 1).max() <= 1e-12
    assert res["power"].shape == (beta.size, 3) and "pdl_db" not in res


def test_ritz_values_are_second_order_in_the_index_offsets(three, scalar_base):
    g, mesh, em = three
    solve, sigma, sgn, w0, X0, beta, vals = scalar_base
    assert beta.size == 10
    errs = []
    for s in (1.0, 0.5):
        n = g.n_core + s * DN
        res = _quantities("scalar", g, em, vals, beta, n_cores=n)
        w, _ = solve(het(g, n), em, sigma, 10)
        exact = np.sort(np.sqrt(-w) / g.k0)[::-1]
        errs.append(np.abs(res["n_eff_ritz"] - exact).max())
        assert np.all(np.diff(res["n_eff_ritz"]) <= 0) and res["mixing"].shape == (10, 10)
    print(f"worst |n_eff(Ritz) - n_eff(exact)|: {errs[0]:.3e} at dn, {errs[1]:.3e} at dn / 2, ratio {errs[0] / errs[1]:.2f}")
    assert 3.0 <= errs[0] / errs[1] <= 5.0


def _toy(seed=7, n=8, ncore=3):
    """A dense vectorial-form pencil with per-core parts and an exact double eigenvalue at n_c = n_core: the Grams of all
    its eigenvectors, and the pencil as a function of the core indices."""
    rng = np.random.default_rng(seed)
    k0, n_core, el = 4.0, 1.5, 2.0
    ec = n_core ** 2

    def spd():
        a = rng.standard_normal((n, n))
        return a @ a.T + n * np.eye(n)

    def sym():
        a = rng.standard_normal((n, n))
        return a + a.T

    Mx, My = np.array([spd() for _ in range(ncore)]), np.array([spd() for _ in range(ncore)])
    K = np.array([sym() for _ in range(ncore)])
    Ml, Kl = spd(), sym()
    Mc = Mx + My
    M = Mc.sum(0) + Ml
    B = Mc.sum(0) / ec + Ml / el
    L = np.linalg.cholesky(B)
    W = np.linalg.solve(L.T, np.linalg.qr(rng.standard_normal((n, n)))[0])    # W^T B W = I
    lam = np.array([10.0, 12.0, 15.0, 15.0, 18.0, 21.0, 25.0, 30.0])
    D = B @ W @ np.diag(lam) @ W.T @ B - K.sum(0) / ec - Kl / el + k0 ** 2 * M

    def pencil(nc):
        e = np.asarray(nc) ** 2
        return np.tensordot(1 / e, K, 1) + Kl / el + D - k0 ** 2 * M, np.tensordot(1 / e, Mc, 1) + Ml / el

    c, s = np.cos(0.7), np.sin(0.7)
    W[:, 2:4] = W[:, 2:4] @ np.array([[c, -s], [s, c]])                          # an arbitrary basis of the double eigenspace
    P = lambda X: np.einsum("ia,...ij,jb->...ab", W, X, W)
    grams = {"M_core": P(Mc.sum(0)), "M_clad": P(Ml), "K_core": P(K.sum(0)), "K_clad": P(Kl), "D": P(D)}
    cg = {"Mx": P(Mx), "My": P(My), "K": P(K)}
    return k0, n_core, (ec, el), grams, cg, pencil, W, lam


def test_degenerate_toy_pencil_against_finite_differences():
    k0, n_core, eps, grams, cg, pencil, W, lam = _toy()
    beta = np.sqrt(lam)
    d = np.array([0.7, -1.1, 0.4])
    res = core_quantities_from_grams("vectorial", cg, grams, beta, k0, eps, direction=d, alpha_p=1.0)
    assert res["cluster"].tolist() == [-1, -1, 0, 0, -1, -1, -1, -1]
    assert res["rayleigh_defect"].max() <= 1e-12
    h = 1e-5
    single = (0, 1, 4, 5, 6, 7)
    n0 = np.full(3, n_core)

    def fd(direction):
        wp, Xp = _eig(*pencil(n0 + h * direction))
        wm, Xm = _eig(*pencil(n0 - h * direction))
        out = (np.sqrt(wp) - np.sqrt(wm)) / (2 * h) / k0
        # the split pair: ascending one-sided slopes of mu from each side, averaged (second order)
        slope = 0.5 * (np.sort((wp[2:4] - 15.0) / h) + np.sort((15.0 - wm[2:4]) / h))
        out[2:4] = slope / (2 * beta[2:4] * k0)
        return out, (Xp, Xm)

    ref, _ = fd(d)
    assert np.allclose(res["dneff_direction"], ref, rtol=0, atol=1e-7)
    assert np.allclose(res["dneff_direction"][list(single)], (res["dneff_dn"] @ d)[list(single)], rtol=0, atol=1e-13)
    B = pencil(n0)[1]
    for c in range(3):
        ref, (Xp, Xm) = fd(np.eye(3)[c])
        assert np.allclose(res["dneff_dn"][:, c], ref, rtol=0, atol=1e-7), c
        # the diagonal of the sensitivity is d mu_n / d n_c of a singleton
        assert np.allclose(np.diag(res["sensitivity"][c])[list(single)], (ref * 2 * beta * k0)[list(single)], rtol=0, atol=1e-6)
        # off the diagonal: h_m^T B dh_n/dn_c = S_c[m, n] / (mu_n - mu_m), from B-normalised, sign-aligned eigenvectors
        for n in (0, 1, 4, 5):
            xp = Xp[:, n] * np.sign(Xp[:, n] @ B @ W[:, n])
            xm = Xm[:, n] * np.sign(Xm[:, n] @ B @ W[:, n])
            dx = (xp - xm) / (2 * h)
            for m in range(8):
                if m != n:
                    assert res["sensitivity"][c][m, n] / (lam[n] - lam[m]) == pytest.approx(W[:, m] @ B @ dx, abs=1e-7)
    # unequal cores: with every eigenvector in the span the Ritz values are the eigenvalues of the new pencil
    nn = n0 + np.array([0.02, -0.03, 0.01])
    rz = core_quantities_from_grams("vectorial", cg, grams, beta, k0, eps, n_cores=nn, alpha_p=1.0)
    w, _ = _eig(*pencil(nn))
    assert np.allclose(rz["n_eff_ritz"], np.sqrt(w[::-1]) / k0, rtol=1e-12, atol=0)
    # power map and PDL: the reference's per-mode formula, core by core
    dm = np.diag(grams["M_core"] + grams["M_clad"])
    px, py = (cg["Mx"][:, range(8), range(8)] / dm).T, (cg["My"][:, range(8), range(8)] / dm).T
    assert np.allclose(res["power"], px + py, rtol=1e-14) and np.allclose(res["power_x"], px, rtol=1e-14)
    assert np.allclose(res["pdl_db"], np.clip(10 * np.log10(np.maximum(px, py) / np.minimum(px, py)), 0, 50), rtol=1e-12)
    assert np.abs(res["power"].sum(1) + res["power_clad"] - 1).max() <= 1e-14


def test_overlapping_discs_go_to_the_higher_index(three):
    g, mesh, em = three
    h = copy.copy(g)
    h.positions = h.core_positions = np.array([[0.0, 0.0], [1.2, 0.3]])
    h.core_radii = np.array([1.5, 1.0])
    qx, qy = em.basis.qx
    in0 = qx ** 2 + qy ** 2 <= 1.5 ** 2
    in1 = (qx - 1.2) ** 2 + (qy - 0.3) ** 2 <= 1.0 ** 2
    assert (in0 & in1).sum() > 50 and (in0 & ~in1).sum() > 50 and (in1 & ~in0).sum() > 50
    owner = em.core_owner(h)
    assert (owner[in1] == 1).all() and (owner[in0 & ~in1] == 0).all() and (owner[~(in0 | in1)] == -1).all()
    assert np.array_equal(owner >= 0, em.core_mask(h))
    C = em.core_grams(np.ones((1, 1, em.N)), False, h)
    assert C["points"].tolist() == [int((in0 & ~in1).sum()), int(in1.sum())]
    assert C["points"].sum() == (in0 | in1).sum()
    w = em.basis.dx
    assert C["M"][0, 0, 0] == pytest.approx(w[in0 & ~in1].sum(), rel=1e-12)
    assert C["M"][1, 0, 0] == pytest.approx(w[in1].sum(), rel=1e-12)


def test_tie_discs_give_the_counts_of_the_reference_arithmetic():
    T = Ties(jittered_square_mesh(8))
    g = T.geometry()
    em = CoreGramEmulation(T.mesh.p, T.mesh.t)
    owner = em.core_owner(g)
    assert np.array_equal(owner >= 0, T.core(g))
    qx, qy = T.basis.qx
    # every operation rounded on its own, in Python floats, point by point
    ref = [sum(ref_inside(float(X), float(Y), float(cx), float(cy), float(r)) for X, Y in zip(qx.ravel(), qy.ravel()))
           for (cx, cy), r in zip(T.positions, T.radii)]
    pts = em.core_grams(np.ones((1, 1, em.N)), False, g)["points"]
    assert pts.tolist() == ref                                     # (the tie discs are disjoint: no point has two owners)
    assert any(T.flips)
    for i, ((e, q), kind) in enumerate(zip(T.targets, T.kinds)):
        assert owner[e, q] == (i if kind == "on" else -1), (i, kind)


def test_argument_errors_before_any_device_call(three):
    g, mesh, em = three
    ns = em.interior.size
    good = [{"Ex_dofs": np.ones(ns), "Ey_dofs": np.ones(ns), "beta": 8.0}]
    scal = [{"field_vector": np.ones(em.N), "beta": 8.0}]
    mf = ModeFields(mesh)
    many = copy.copy(g)
    many.positions = np.zeros((65, 2))
    many.core_radii = np.ones(65)

    class NoCores:
        n_core, n_clad, k0 = g.n_core, g.n_clad, g.k0

    for bad in (NoCores(), many):
        with pytest.raises(ValueError):
            mf.core_grams(good, bad)
        with pytest.raises(ValueError):
            core_decomposition(good, mesh, bad)
    for recs in ([{"Ex_dofs": np.ones(ns - 1), "Ey_dofs": np.ones(ns - 1), "beta": 8.0}],
                 [{"field_vector": np.ones(em.N + 1), "beta": 8.0}], good + scal):
        with pytest.raises(ValueError):
            mf.core_grams(recs, g)
        with pytest.raises(ValueError):
            core_decomposition(recs, mf, g)
    with pytest.raises(ValueError):
        core_decomposition([], mesh, g)
    for b in (None, np.nan, np.inf, 0.0, -1.0):
        rec = {"Ex_dofs": np.ones(ns), "Ey_dofs": np.ones(ns)}
        if b is not None:
            rec["beta"] = b
        with pytest.raises(ValueError):
            core_decomposition([rec], mesh, g)
    for v in ((1.5, 1.5), (1.5, 1.5, 1.5, 1.5), (1.5, np.nan, 1.5), (1.5, 0.0, 1.5), "abc"):
        with pytest.raises(ValueError):
            core_decomposition(good, mesh, g, n_cores=v)
    for v in ((1.0, 1.0), (1.0, np.inf, 1.0), "abc"):
        with pytest.raises(ValueError):
            core_decomposition(good, mesh, g, direction=v)
    with pytest.raises(ValueError):
        core_decomposition(good, mesh, g, cluster_rtol=-1.0)
    noidx = copy.copy(g)
    del noidx.k0
    with pytest.raises(ValueError):
        core_decomposition(good, mesh, noidx)
    with pytest.raises(ValueError):
        core_quantities_from_grams("tensor", {}, {}, [8.0], g.k0, (2.0, 1.0))


def test_core_gram_entries_refuse_bad_arguments_on_the_host(built_library):
    lib = _native.load_library()
    b = ctypes.c_int64(-1)
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)                                       # never dereferenced: the locator is checked first
    assert lib.plfem_core_gram_work_bytes(null, 2, 22, 7, ctypes.byref(b)) == _native.PLFEM_EINVAL
    assert lib.plfem_core_gram_work_bytes(null, 2, 22, 7, None) == _native.PLFEM_EINVAL
    for ncomp, k, ncore in ((0, 5, 3), (3, 5, 3), (2, 0, 3), (2, -1, 3), (2, 5, 0), (2, 5, 65), (1, 5, -1)):
        assert lib.plfem_core_gram_work_bytes(null, ncomp, k, ncore, ctypes.byref(b)) == _native.PLFEM_EINVAL
        assert lib.plfem_core_grams(null, ncomp, k, one, 0, one, ncore, one, 1 << 30, one, one) == _native.PLFEM_EINVAL
    assert b.value == -1
    assert lib.plfem_core_grams(null, 2, 5, None, 1, None, 3, None, 0, None, None) == _native.PLFEM_EINVAL
