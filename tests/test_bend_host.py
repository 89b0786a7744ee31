"""Coordinate-weighted Grams and the bend quantities built from them, host side (no GPU): the NumPy emulation of the moment
Gram call against the oracle's pencil assembled with the bent permittivity, Hellmann-Feynman d n_eff / d kappa against
central differences of oracle eigen-solves, the scalar identity, the second order of the Rayleigh-Ritz values, an exactly
degenerate toy pencil, centroid and D4-sigma widths of a Gaussian, the origin shift, bend_propagate, and argument checking
before any device call."""
import copy
import ctypes

import numpy as np
import pytest

from moment_gram_emulation import NAMES, MomentGramEmulation
from oracle import hfield, scalar
from pl_fem_vectoriel_amd import (ModeFields, _native, bend_propagate, bend_quantities_from_grams, bend_response)
from quartic_emulation import square_mesh
from test_cores_host import _base, three as _three                # the section and the oracle base solve of the core tests
from test_dispersion_host import _eig, _rel

ANGLE = 0.3


@pytest.fixture(scope="module")
def three(_three):
    g, mesh, _ = _three
    return g, mesh, MomentGramEmulation(mesh.p, mesh.t)


def bent(g, kappa, angle, form, origin=(0.0, 0.0)):
    """A duck geometry: g with the first-order bent permittivity, eps (1 + 2 kappa Xt) for the scalar assembly and
    eps / (1 - 2 kappa Xt) for the vectorial one (whose forms take 1 / eps), Xt = cos(angle) X + sin(angle) Y."""
    h = copy.copy(g)
    c, s = np.cos(angle), np.sin(angle)

    def epsilon(x, y):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        xt = c * (x - origin[0]) + s * (y - origin[1])
        e = g.epsilon(x, y)
        return e * (1 + 2 * kappa * xt) if form == "scalar" else e / (1 - 2 * kappa * xt)

    h.epsilon = epsilon
    return h


def test_emulated_moment_grams_reproduce_the_bent_pencil(three):
    g, mesh, em = three
    rng = np.random.default_rng(31)
    k, kappa, o = 5, 1e-3, (0.4, -0.2)
    c, s = np.cos(ANGLE), np.sin(ANGLE)
    ec, el, k0 = g.n_core ** 2, g.n_clad ** 2, g.k0

    vals = rng.standard_normal((2, k, em.interior.size))
    G, P = em.grams(vals, True, g), em.moment_grams(vals, True, g, o)
    assert tuple(P) == NAMES[2]
    V = np.hstack([vals[0], vals[1]]).T
    A, B, basis, *_ = hfield.assemble_hfield_system_fused(bent(g, kappa, ANGLE, "vectorial", o), em.mesh)
    A, B, _ = hfield.restrict_interior(A, B, basis)
    Kt = sum((c * P[f"K_{r}_X"] + s * P[f"K_{r}_Y"]) / e for r, e in (("core", ec), ("clad", el)))
    Mt = sum((c * P[f"M_{r}_X"] + s * P[f"M_{r}_Y"]) / e for r, e in (("core", ec), ("clad", el)))
    a = G["K_core"] / ec + G["K_clad"] / el + G["D"] - k0 ** 2 * (G["M_core"] + G["M_clad"]) - 2 * kappa * Kt
    b = G["M_core"] / ec + G["M_clad"] / el - 2 * kappa * Mt
    ea, eb = _rel(a, V.T @ (A @ V)), _rel(b, V.T @ (B @ V))
    # the bend's own part, against the difference of the two assembled pencils (what the 1e-12 above leaves of it)
    A0, B0, basis, *_ = hfield.assemble_hfield_system_fused(g, em.mesh)
    A0, B0, _ = hfield.restrict_interior(A0, B0, basis)
    da, db = _rel(-2 * kappa * Kt, V.T @ ((A - A0) @ V)), _rel(-2 * kappa * Mt, V.T @ ((B - B0) @ V))
    print(f"vectorial: V^T A_bent V {ea:.1e}, V^T B_bent V {eb:.1e}; the bend parts alone {da:.1e}, {db:.1e}")
    assert ea <= 1e-12 and eb <= 1e-12
    assert da <= 1e-9 and db <= 1e-9                    # a difference of pencils 1e-3 apart: three digits are lost

    u = rng.standard_normal((1, k, em.N))
    Gs, Ps = em.grams(u, False, g), em.moment_grams(u, False, g, o)
    assert tuple(Ps) == NAMES[1]
    S, Mm, Me, _ = scalar.assemble(bent(g, kappa, ANGLE, "scalar", o), em.mesh)
    U = u[0].T
    Et = sum(e * (c * Ps[f"M_{r}_X"] + s * Ps[f"M_{r}_Y"]) for r, e in (("core", ec), ("clad", el)))
    a = Gs["S"] - k0 ** 2 * (ec * Gs["M_core"] + el * Gs["M_clad"]) - 2 * kappa * k0 ** 2 * Et
    es = _rel(a, U.T @ ((S - k0 ** 2 * Me) @ U))
    _, _, Me0, _ = scalar.assemble(g, em.mesh)
    ds = _rel(2 * kappa * Et, U.T @ ((Me - Me0) @ U))
    print(f"scalar: V^T A_bent V {es:.1e}; the bend part alone {ds:.1e}")
    assert es <= 1e-12 and ds <= 1e-9
    # the second moments: the mass matrix of eps = X^2, XY, Y^2 (a duck geometry again)
    for nm, f in (("M_XX", lambda x, y: (x - o[0]) ** 2), ("M_XY", lambda x, y: (x - o[0]) * (y - o[1])),
                  ("M_YY", lambda x, y: (y - o[1]) ** 2)):
        h = copy.copy(g)
        h.epsilon = lambda x, y, f=f: f(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)) + 0j
        _, _, Mw, _ = scalar.assemble(h, em.mesh)
        assert _rel(Ps[nm], U.T @ (Mw @ U)) <= 1e-12, nm


def test_origin_shift(three):
    g, mesh, em = three
    rng = np.random.default_rng(32)
    o = (0.7, -1.3)
    for vals, indexed in ((rng.standard_normal((2, 4, em.interior.size)), True), (rng.standard_normal((1, 4, em.N)), False)):
        F = em.flat_features(vals, indexed)
        G, P0, P1 = em.grams(vals, indexed, g), em.moment_grams(vals, indexed, g, features=F), em.moment_grams(vals, indexed, g, o, F)
        for r in ("core", "clad"):
            for ax, oo in (("X", o[0]), ("Y", o[1])):
                assert _rel(P1[f"M_{r}_{ax}"], P0[f"M_{r}_{ax}"] - oo * G[f"M_{r}"]) <= 1e-12
        M = G["M_core"] + G["M_clad"]
        MX, MY = P0["M_core_X"] + P0["M_clad_X"], P0["M_core_Y"] + P0["M_clad_Y"]
        assert _rel(P1["M_XX"], P0["M_XX"] - 2 * o[0] * MX + o[0] ** 2 * M) <= 1e-12
        assert _rel(P1["M_XY"], P0["M_XY"] - o[0] * MY - o[1] * MX + o[0] * o[1] * M) <= 1e-12
        assert _rel(P1["M_YY"], P0["M_YY"] - 2 * o[1] * MY + o[1] ** 2 * M) <= 1e-12


@pytest.fixture(scope="module")
def scalar_base(three):
    g, mesh, em = three
    base = _base("scalar", g, em, 10)
    vals, beta = base[-1], base[-2]
    F = em.flat_features(vals, False)
    return base, em.grams(vals, False, g), em.moment_grams(vals, False, g, features=F)


def _quantities(g, scalar_base, **kw):
    base, G, P = scalar_base
    return bend_quantities_from_grams("scalar", P, G, base[-2], g.k0, (g.n_core ** 2, g.n_clad ** 2), **kw)


@pytest.mark.parametrize("angle", [0.0, 0.3, np.pi / 2])
def test_dneff_dkappa_matches_central_differences_of_oracle_solves(three, scalar_base, angle):
    g, mesh, em = three
    delta = 1e-6
    (solve, sigma, sgn, w0, X0, beta, vals), _, _ = scalar_base
    res = _quantities(g, scalar_base, angle=angle)
    assert res["rayleigh_defect"].max() <= 1e-10 and beta.size == 10
    x = X0 / np.linalg.norm(X0, axis=0)

    def match(w, X):                                    # eigenvalue of the unique |cos| > 0.999 partner, else nan
        c = np.abs(x.T @ X) / np.linalg.norm(X, axis=0)[None]
        return np.array([w[np.argmax(r)] if (r > 0.999).sum() == 1 else np.nan for r in c])

    mp = match(*solve(bent(g, delta, angle, "scalar"), em, sigma, w0.size))
    mm = match(*solve(bent(g, -delta, angle, "scalar"), em, sigma, w0.size))
    errs = []
    for i in range(beta.size):
        # separation: the nearest neighbour's gap must exceed 100 x what the bend changes it by
        j = np.argsort(np.abs(w0 - w0[i]))[1]
        moved = max(abs((mp[i] - mp[j]) - (w0[i] - w0[j])), abs((mm[i] - mm[j]) - (w0[i] - w0[j])))
        if not np.isfinite(moved) or abs(w0[i] - w0[j]) < 100 * moved:
            continue
        fd = (np.sqrt(sgn * mp[i]) - np.sqrt(sgn * mm[i])) / (2 * delta * g.k0)
        errs.append(abs(res["dneff_dkappa"][i] - fd))
    scale = np.abs(res["dneff_dkappa"]).max()
    print(f"angle {angle:.2f}: {len(errs)} of {beta.size} modes compared, worst |HF - FD| = {max(errs):.2e} on values up to "
          f"{scale:.2f} um ({max(errs) / scale:.1e} of it)")
    assert len(errs) >= beta.size - 2
    assert max(errs) <= 1e-6 * scale


def test_scalar_dneff_dkappa_is_the_eps_weighted_first_moment(three, scalar_base):
    g, mesh, em = three
    (*_, beta, vals), G, P = scalar_base
    ec, el = g.n_core ** 2, g.n_clad ** 2
    for angle in (0.0, ANGLE, 2.0):
        res = _quantities(g, scalar_base, angle=angle)
        assert (res["cluster"] == -1).all()
        c, s = np.cos(angle), np.sin(angle)
        num = np.diag(ec * (c * P["M_core_X"] + s * P["M_core_Y"]) + el * (c * P["M_clad_X"] + s * P["M_clad_Y"]))
        ref = num / ((beta / g.k0) * np.diag(G["M_core"] + G["M_clad"]))
        assert np.abs(res["dneff_dkappa"] - ref).max() <= 1e-12 * np.abs(ref).max()
        assert np.abs(np.diag(c * res["coupling"][0] + s * res["coupling"][1]) + 2 * beta * g.k0 * ref).max() <= 1e-9
    both = _quantities(g, scalar_base, angle=np.array([0.0, ANGLE]), curvature=np.array([0.0, 0.0]))
    assert both["dneff_dkappa"].shape == (2, beta.size)
    assert np.array_equal(both["dneff_dkappa"][1], _quantities(g, scalar_base, angle=ANGLE)["dneff_dkappa"])


def test_ritz_values_are_second_order_in_the_curvature(three, scalar_base):
    g, mesh, em = three
    (solve, sigma, sgn, w0, X0, beta, vals), _, _ = scalar_base
    kappas = np.array([1 / 4000.0, 1 / 8000.0])         # R = 4 mm and 8 mm
    res = _quantities(g, scalar_base, curvature=kappas, angle=ANGLE)
    assert res["n_eff_ritz"].shape == (2, 10) and res["mixing"].shape == (2, 10, 10) and res["beta_ritz"].shape == (2, 10)
    n0 = np.sort(beta / g.k0)[::-1]
    errs = []
    for i, kp in enumerate(kappas):
        w, _ = solve(bent(g, kp, ANGLE, "scalar"), em, sigma, 10)
        exact = np.sort(np.sqrt(-w) / g.k0)[::-1]
        errs.append(np.abs(res["n_eff_ritz"][i] - exact).max())
        assert np.all(np.diff(res["n_eff_ritz"][i]) <= 0)
        print(f"R = {1e-3 / kp:.0f} mm: shifts up to {np.abs(exact - n0).max():.2e}, worst |n_eff(Ritz) - n_eff(exact)| {errs[-1]:.2e}")
    print(f"ratio {errs[0] / errs[1]:.2f}")
    assert 3.0 <= errs[0] / errs[1] <= 5.0
    # curvature 0: the records' own values
    zero = _quantities(g, scalar_base, curvature=0.0)
    assert zero["n_eff_ritz"].shape == (1, 10) and np.abs(zero["n_eff_ritz"][0] - n0).max() <= 1e-10


def _toy(seed=9, n=8):
    """A dense vectorial-form pencil with first-moment parts and an exact double eigenvalue at kappa = 0: the Grams of
    all its eigenvectors, and the pencil as a function of the curvature vector (kappa cos, kappa sin)."""
    rng = np.random.default_rng(seed)
    k0, ec, el = 4.0, 2.25, 2.0

    def spd():
        a = rng.standard_normal((n, n))
        return a @ a.T + n * np.eye(n)

    def sym():
        a = rng.standard_normal((n, n))
        return a + a.T

    Mc, Ml, Kc, Kl = spd(), spd(), sym(), sym()
    first = {f"{f}_{r}_{ax}": sym() for f in "MK" for r in ("core", "clad") for ax in "XY"}
    M = Mc + Ml
    B = Mc / ec + Ml / el
    L = np.linalg.cholesky(B)
    W = np.linalg.solve(L.T, np.linalg.qr(rng.standard_normal((n, n)))[0])    # W^T B W = I
    lam = np.array([10.0, 12.0, 15.0, 15.0, 18.0, 21.0, 25.0, 30.0])
    D = B @ W @ np.diag(lam) @ W.T @ B - Kc / ec - Kl / el + k0 ** 2 * M
    eps = {"core": ec, "clad": el}

    def pencil(kv):
        A = Kc / ec + Kl / el + D - k0 ** 2 * M
        Bk = B.copy()
        for ax, kp in zip("XY", kv):
            A = A - 2 * kp * sum(first[f"K_{r}_{ax}"] / eps[r] for r in eps)
            Bk = Bk - 2 * kp * sum(first[f"M_{r}_{ax}"] / eps[r] for r in eps)
        return A, Bk

    c, s = np.cos(0.7), np.sin(0.7)
    W[:, 2:4] = W[:, 2:4] @ np.array([[c, -s], [s, c]])                          # an arbitrary basis of the double eigenspace
    proj = lambda X: W.T @ X @ W
    grams = {"M_core": proj(Mc), "M_clad": proj(Ml), "K_core": proj(Kc), "K_clad": proj(Kl), "D": proj(D)}
    mg = {nm: proj(X) for nm, X in first.items()}
    mg.update(M_XX=proj(spd()), M_XY=proj(sym()), M_YY=proj(spd()))
    return k0, (ec, el), grams, mg, pencil, W, lam, B


def test_degenerate_toy_pencil_against_finite_differences():
    k0, eps, grams, mg, pencil, W, lam, B = _toy()
    beta = np.sqrt(lam)
    h = 1e-5
    single = [0, 1, 4, 5, 6, 7]
    for angle in (0.0, np.pi / 2, 0.9):
        res = bend_quantities_from_grams("vectorial", mg, grams, beta, k0, eps, angle=angle, alpha_p=1.0)
        assert res["cluster"].tolist() == [-1, -1, 0, 0, -1, -1, -1, -1]
        assert res["rayleigh_defect"].max() <= 1e-12
        d = np.array([np.cos(angle), np.sin(angle)])
        wp, Xp = _eig(*pencil(h * d))
        wm, Xm = _eig(*pencil(-h * d))
        ref = (np.sqrt(wp) - np.sqrt(wm)) / (2 * h) / k0
        # the split pair: ascending one-sided slopes of mu from each side, averaged (second order)
        slope = 0.5 * (np.sort((wp[2:4] - 15.0) / h) + np.sort((15.0 - wm[2:4]) / h))
        ref[2:4] = slope / (2 * beta[2:4] * k0)
        assert np.allclose(res["dneff_dkappa"], ref, rtol=0, atol=1e-7), angle
        C = d[0] * res["coupling"][0] + d[1] * res["coupling"][1]
        # the diagonal of the coupling is d mu_n / d kappa of a singleton
        assert np.allclose(np.diag(C)[single], (ref * 2 * beta * k0)[single], rtol=0, atol=1e-6)
        # off the diagonal: h_m^T B dh_n/dkappa = C[m, n] / (mu_n - mu_m), from B-normalised, sign-aligned eigenvectors
        for n in (0, 1, 4, 5):
            xp = Xp[:, n] * np.sign(Xp[:, n] @ B @ W[:, n])
            xm = Xm[:, n] * np.sign(Xm[:, n] @ B @ W[:, n])
            dx = (xp - xm) / (2 * h)
            for m in range(8):
                if m != n:
                    assert C[m, n] / (lam[n] - lam[m]) == pytest.approx(W[:, m] @ B @ dx, abs=1e-7)
    # with every eigenvector in the span the Ritz values are the eigenvalues of the bent pencil
    kv = np.array([0.02, -0.03])
    rz = bend_quantities_from_grams("vectorial", mg, grams, beta, k0, eps, curvature=np.hypot(*kv), angle=np.arctan2(kv[1], kv[0]),
                                    alpha_p=1.0)
    w, _ = _eig(*pencil(kv))
    assert np.allclose(rz["n_eff_ritz"][0], np.sqrt(w[::-1]) / k0, rtol=1e-12, atol=0)
    Y = rz["mixing"][0]
    A2, B2 = pencil(kv)
    assert np.abs(Y.T @ (W.T @ B2 @ W) @ Y - np.eye(8)).max() <= 1e-12
    # a bent B that is no longer positive definite
    with pytest.raises(ValueError):
        bend_quantities_from_grams("vectorial", mg, grams, beta, k0, eps, curvature=50.0, alpha_p=1.0)


def test_centroid_and_widths_of_a_gaussian():
    """A nodal (P2-interpolated) rotated elliptical Gaussian exp(-(a / wa)^2 - (b / wb)^2) centred at (x0, y0): centroid
    (x0, y0), D4-sigma widths (2 wa, 2 wb) along its axes.

    Against the closed form the error is that of the interpolant: in one dimension a quadratic interpolant on an element
    of width h misses f by at most h^3 max|f'''| / (72 sqrt 3), max|f'''| < 4 / w^3 for exp(-t^2 / w^2), so 0.032 (h / w)^3;
    a product of two factors and the moments' sensitivity leave the bound 0.5 (h / w)^3 relative to w, with h the longest
    edge (here 0.117, w = 0.22: 1.6e-2).  Measured: centroid off by 6.4e-7, widths by 4.3e-5.

    The six-point rule (degree 4) against the 16-point rule (degree 8, exact for X^2 u^2): measured 1.7e-9 (centroid) and
    1.1e-7 (widths); asserted with a factor 10."""
    p, t = square_mesh(32)
    em = MomentGramEmulation(p, t)
    x0, y0, wa, wb, rot = 0.1, -0.05, 0.3, 0.22, 0.4
    xy = em.basis.doflocs
    a = np.cos(rot) * (xy[0] - x0) + np.sin(rot) * (xy[1] - y0)
    b = -np.sin(rot) * (xy[0] - x0) + np.cos(rot) * (xy[1] - y0)
    vals = np.exp(-(a / wa) ** 2 - (b / wb) ** 2)[None, None]

    class NoCores:
        positions, core_radii = np.zeros((0, 2)), np.zeros(0)

    o = (0.3, 0.2)
    G, P = em.grams(vals, False, NoCores), em.moment_grams(vals, False, NoCores, o)
    res = bend_quantities_from_grams("scalar", P, G, [5.0], 4.0, (2.0, 1.0))
    edges = np.concatenate([np.hypot(*(p[:, t[i]] - p[:, t[j]])) for i, j in ((0, 1), (1, 2), (2, 0))])
    tol = 0.5 * (edges.max() / wb) ** 3 * wb
    cen = res["centroid"][0] + np.array(o)
    e_c, e_w = np.abs(cen - (x0, y0)).max(), np.abs(res["width_d4sigma"][0] - (2 * wa, 2 * wb)).max()
    print(f"h = {edges.max():.3f}: centroid off by {e_c:.2e}, widths by {e_w:.2e} (bound {tol:.2e})")
    assert e_c <= tol and e_w <= tol
    sm = res["second_moment"][0]
    R = np.array([[np.cos(rot), -np.sin(rot)], [np.sin(rot), np.cos(rot)]])
    assert np.abs(sm - R @ np.diag([wa ** 2 / 4, wb ** 2 / 4]) @ R.T).max() <= tol * wa
    # the six-point rule against the 16-point rule, on the same interpolant
    Q = em.moment_grams16(vals, False, o)
    m = Q["M"][0, 0]
    c16 = np.array([Q["M_X"][0, 0], Q["M_Y"][0, 0]]) / m
    s16 = np.array([[Q["M_XX"][0, 0], Q["M_XY"][0, 0]], [Q["M_XY"][0, 0], Q["M_YY"][0, 0]]]) / m - np.outer(c16, c16)
    w16 = 4 * np.sqrt(np.linalg.eigvalsh(s16)[::-1])
    q_c, q_w = np.abs(res["centroid"][0] - c16).max(), np.abs(res["width_d4sigma"][0] - w16).max()
    print(f"six-point against 16-point rule: centroid {q_c:.2e}, widths {q_w:.2e}")
    assert q_c <= 10 * 1.7e-9 and q_w <= 10 * 1.1e-7


def test_bend_propagate(three, scalar_base):
    g, mesh, em = three
    (*_, beta, vals), G, P = scalar_base
    res = _quantities(g, scalar_base)
    B = res["pencil"]["B"]
    k = beta.size
    L = 100.0
    # straight: the records are eigenvectors to the Rayleigh defect (<= 1e-10 of mu, so a phase error <= 1e-10 beta L / 2 =
    # 3e-8 at beta = 6 / um) and B-orthogonal to the eigensolver's tolerance
    T = bend_propagate(res, [[L, 0.0, 0.0]])
    assert T["transfer"].shape == (k, k) and T["beta"].shape == (1, k) and T["segment_transfer"].shape == (1, k, k)
    assert np.abs(T["transfer"] - np.diag(np.exp(-1j * beta * L))).max() <= 1e-7
    assert np.abs(T["beta"][0] - np.sort(beta)[::-1]).max() <= 1e-9
    kappa = 1 / 3000.0
    one = bend_propagate(res, [[L, kappa, ANGLE]])["transfer"]
    two = bend_propagate(res, [[L / 2, kappa, ANGLE], [L / 2, kappa, ANGLE]])["transfer"]
    assert np.abs(one - two).max() <= 1e-11
    assert np.abs(one - np.diag(np.exp(-1j * beta * L))).max() > 1e-3          # the bend does something
    path = [[L, kappa, ANGLE], [30.0, 0.0, 0.0], [50.0, 2 * kappa, 2.0]]
    T = bend_propagate(res, path)
    U = T["transfer"]
    assert np.abs(U.conj().T @ B @ U - B).max() <= 1e-12
    assert np.abs(U - T["segment_transfer"][2] @ T["segment_transfer"][1] @ T["segment_transfer"][0]).max() <= 1e-12
    # phase conjugation: back through the reversed path
    a = np.random.default_rng(3).standard_normal(k) + 1j * np.random.default_rng(4).standard_normal(k)
    back = bend_propagate(res, path[::-1])["transfer"]
    assert np.abs(np.conj(back @ np.conj(U @ a)) - a).max() <= 1e-11
    assert np.array_equal(bend_propagate(res, np.zeros((0, 3)))["transfer"], np.eye(k))
    # cut-off, named; vectorial; malformed
    with pytest.raises(ValueError, match="segment 1"):
        bend_propagate(res, [[L, 0.0, 0.0], [L, 1.0, 0.0]])
    _, _, grams, mg, *_ = _toy()
    vec = bend_quantities_from_grams("vectorial", mg, grams, np.sqrt(_toy()[6]), 4.0, (2.25, 2.0), alpha_p=1.0)
    with pytest.raises(ValueError, match="scalar"):
        bend_propagate(vec, [[L, 0.0, 0.0]])
    for bad in ([L, 0.0, 0.0], [[L, 0.0]], [[-1.0, 0.0, 0.0]], [[L, np.nan, 0.0]], [[L, 0.0, np.inf]], "abc"):
        with pytest.raises(ValueError):
            bend_propagate(res, bad)
    for bad in ({}, {"pencil": {}}, None, G):
        with pytest.raises(ValueError):
            bend_propagate(bad, [[L, 0.0, 0.0]])


def test_argument_errors_before_any_device_call(three, scalar_base):
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
            mf.moment_grams(good, bad)
        with pytest.raises(ValueError):
            bend_response(good, mesh, bad)
    for recs in ([{"Ex_dofs": np.ones(ns - 1), "Ey_dofs": np.ones(ns - 1), "beta": 8.0}],
                 [{"field_vector": np.ones(em.N + 1), "beta": 8.0}], good + scal):
        with pytest.raises(ValueError):
            mf.moment_grams(recs, g)
        with pytest.raises(ValueError):
            bend_response(recs, mf, g)
    with pytest.raises(ValueError):
        bend_response([], mesh, g)
    for b in (None, np.nan, np.inf, 0.0, -1.0):
        rec = {"Ex_dofs": np.ones(ns), "Ey_dofs": np.ones(ns)}
        if b is not None:
            rec["beta"] = b
        with pytest.raises(ValueError):
            bend_response([rec], mesh, g)
    for o in ((0.0,), (0.0, 0.0, 0.0), (0.0, np.nan), (np.inf, 0.0), "ab", None):
        with pytest.raises(ValueError):
            mf.moment_grams(good, g, origin=o)
        with pytest.raises(ValueError):
            bend_response(good, mesh, g, origin=o)
    for r in (0.0, np.nan, (1e4, 0.0), np.zeros((2, 2)) + 1e4, (), "abc"):
        with pytest.raises(ValueError):
            bend_response(good, mesh, g, radius=r)
    for a in (np.nan, np.inf, "abc", (0.0, 0.1)):                  # (two angles need curvatures to go with)
        with pytest.raises(ValueError):
            bend_response(good, mesh, g, angle=a)
    with pytest.raises(ValueError):
        bend_response(good, mesh, g, radius=(1e4, 2e4, 3e4), angle=(0.0, 0.1))
    with pytest.raises(ValueError):
        bend_response(good, mesh, g, cluster_rtol=-1.0)
    # 2 |x| / R reaches 1 on the mesh's bounding box: the bent permittivity would change sign
    xmax = max(abs(v) for v in mf.bbox)
    with pytest.raises(ValueError, match="change sign"):
        bend_response(good, mesh, g, radius=2 * xmax)
    with pytest.raises(ValueError, match="change sign"):
        bend_response(good, mesh, g, radius=(1e4, -1.9 * xmax))
    with pytest.raises(ValueError, match="change sign"):
        bend_response(good, mesh, g, radius=1e3, origin=(600.0, 0.0))
    noidx = copy.copy(g)
    del noidx.k0
    with pytest.raises(ValueError):
        bend_response(good, mesh, noidx)
    (*_, beta, vals), G, P = scalar_base
    eps = (g.n_core ** 2, g.n_clad ** 2)
    with pytest.raises(ValueError):
        bend_quantities_from_grams("tensor", P, G, beta, g.k0, eps)
    with pytest.raises(ValueError):
        bend_quantities_from_grams("vectorial", P, G, beta, g.k0, eps)       # no K_r_X among scalar moment Grams
    with pytest.raises(ValueError):
        bend_quantities_from_grams("scalar", P, G, beta[:-1], g.k0, eps)
    with pytest.raises(ValueError):
        bend_quantities_from_grams("scalar", P, G, beta, g.k0, eps, curvature=np.nan)
    with pytest.raises(ValueError):
        bend_quantities_from_grams("scalar", P, G, beta, g.k0, eps, cluster_rtol=np.nan)


def test_moment_gram_entries_refuse_bad_arguments_on_the_host(built_library):
    lib = _native.load_library()
    b = ctypes.c_int64(-1)
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)                                       # never dereferenced: the locator is checked first
    assert lib.plfem_moment_gram_work_bytes(2, 22, None) == _native.PLFEM_EINVAL
    for ncomp, k in ((0, 5), (3, 5), (2, 0), (1, -1)):
        assert lib.plfem_moment_gram_work_bytes(ncomp, k, ctypes.byref(b)) == _native.PLFEM_EINVAL
        assert lib.plfem_moment_grams(null, ncomp, k, one, 0, one, 3, one, one, 1 << 30, one) == _native.PLFEM_EINVAL
    assert b.value == -1
    assert lib.plfem_moment_grams(null, 2, 5, None, 1, None, 3, None, None, 0, None) == _native.PLFEM_EINVAL
    # the bound of the header: nout k^2 doubles, then nout ceil(k / 32)^2 x 768 blocks of 8 KiB
    for ncomp, nout in ((1, 7), (2, 11)):
        for k in (1, 22, 32, 33, 70):
            assert lib.plfem_moment_gram_work_bytes(ncomp, k, ctypes.byref(b)) == _native.PLFEM_OK
            nc = (k + 31) // 32
            assert b.value == (nout * k * k * 8 + 255) // 256 * 256 + nout * nc * nc * 768 * 8192
