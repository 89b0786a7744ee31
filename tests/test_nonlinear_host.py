"""Nonlinear overlap tensor, host side (no GPU): the 16-point degree-8 rule, the NumPy emulation of the quartic kernel
against exact barycentric integration, the symmetries of the expanded tensor, Gaussian records against closed-form A_eff
and MFD, gamma against n2 k0 / A_eff, and argument checking before any device call."""
import ctypes
from math import factorial

import numpy as np
import pytest

from quartic_emulation import QuarticEmulation, exact_quartic, square_mesh
from pl_fem_vectoriel_amd import MCFGeometry, _native, generate_mesh, mode_nonlinearity
from pl_fem_vectoriel_amd.nonlinear import (QUAD16_W, QUAD16_X, expand_pairs, nonlinearity_from_pairs, pair_index)


def test_rule_integrates_degree_8_monomials():
    x, y = QUAD16_X
    assert QUAD16_X.shape == (2, 16) and QUAD16_W.shape == (16,)
    assert np.all(QUAD16_W > 0)
    assert np.all(x > 0) and np.all(y > 0) and np.all(x + y < 1)
    assert abs(QUAD16_W.sum() - 0.5) <= 1e-15
    for a in range(9):
        for b in range(9 - a):
            exact = factorial(a) * factorial(b) / factorial(a + b + 2)
            assert abs((QUAD16_W * x ** a * y ** b).sum() - exact) <= 1e-14 * exact, (a, b)


def test_pair_numbering():
    k = 7
    P = pair_index(k)
    I, J = np.triu_indices(k)
    assert np.array_equal(P[I, J], np.arange(I.size))
    assert np.array_equal(P, P.T)
    for i in range(k):
        for j in range(i, k):
            assert P[i, j] == i * k - i * (i - 1) // 2 + (j - i)


@pytest.mark.parametrize("ncomp", [1, 2])
def test_emulation_matches_exact_integration(ncomp):
    p, t = square_mesh(10, seed=3)
    em = QuarticEmulation(p, t)
    indexed = ncomp == 2
    n = em.interior.size if indexed else em.N
    vals = np.random.default_rng(5).standard_normal((ncomp, 6, n))
    Q = em.quartic(vals, indexed)
    E = exact_quartic(em, vals, indexed)
    assert Q.shape == (21, 21)
    assert np.abs(Q - E).max() <= 1e-13 * np.abs(E).max()
    ent = np.array([[0, 5], [3, 20], [7, 7]])
    assert np.allclose(exact_quartic(em, vals, indexed, entries=ent), E[ent[:, 0], ent[:, 1]], rtol=1e-14, atol=0)


def _grams(rng, k, kind):
    A = rng.standard_normal((k, k))
    M = A @ A.T + k * np.eye(k)
    if kind == "scalar":
        return {"M_core": 0.3 * M, "M_clad": 0.7 * M, "S": 2.0 * M}
    return {"M_core": 0.3 * M, "M_clad": 0.7 * M, "K_core": M, "K_clad": 0.5 * M, "D": 0.5 * M}


def test_expanded_tensor_symmetries():
    rng = np.random.default_rng(7)
    p, t = square_mesh(6, seed=1)
    em = QuarticEmulation(p, t)
    k = 4
    for ncomp, kind in ((1, "scalar"), (2, "vectorial")):
        n = em.interior.size if ncomp == 2 else em.N
        vals = rng.standard_normal((ncomp, k, n))
        pairs = em.quartic(vals, ncomp == 2)
        pairs = 0.5 * (pairs + pairs.T)
        res = nonlinearity_from_pairs(kind, pairs, _grams(rng, k, kind))
        Q = res["Q"]
        assert Q.shape == (k,) * 4
        assert np.array_equal(Q, Q.transpose(1, 0, 2, 3))       # ij
        assert np.array_equal(Q, Q.transpose(0, 1, 3, 2))       # lm
        assert np.array_equal(Q, Q.transpose(2, 3, 0, 1))       # (ij) <-> (lm)
        perm13 = np.abs(Q - Q.transpose(0, 2, 1, 3)).max() / np.abs(Q).max()
        if kind == "scalar":                                     # full permutation symmetry
            assert perm13 <= 1e-13
        else:                                                    # (hx_i hx_j + hy_i hy_j)(...): not i <-> l
            assert perm13 > 1e-3
        N = res["norm"]
        assert np.allclose(res["f"], Q / np.sqrt(np.einsum("i,j,l,m->ijlm", N, N, N, N)), rtol=1e-14)
        ii = np.arange(k)
        assert np.allclose(res["a_eff"], 1.0 / res["f"][ii, ii, ii, ii], rtol=1e-15)
        assert np.allclose(res["a_eff_pair"][1, 3], 1.0 / res["f"][1, 1, 3, 3], rtol=1e-15)
    with pytest.raises(ValueError):
        expand_pairs(np.zeros((5, 5)))


@pytest.fixture(scope="module")
def fibre():
    g = MCFGeometry(1, 8.0, 2.5, 1.46, 1.444, wavelength_um=1.55)
    mesh = generate_mesh(g, 1.0, 1)                              # refined towards the core
    return g, mesh, QuarticEmulation(mesh.p, mesh.t)


@pytest.mark.parametrize("kind", ["scalar", "vectorial"])
def test_gaussian_effective_area_and_mfd(fibre, kind):
    g, _, em = fibre
    w = 2.5
    x, y = em.basis.doflocs
    f = np.exp(-(x * x + y * y) / w ** 2)
    if kind == "scalar":
        vals, indexed = f[None, None], False
    else:                                                        # Hx = Gaussian, Hy = 0 on the interior DOFs
        vals, indexed = np.stack([f[em.interior][None], np.zeros((1, em.interior.size))]), True
    res = nonlinearity_from_pairs(kind, em.quartic(vals, indexed), em.grams(vals, indexed, g))
    assert abs(res["a_eff"][0] / (np.pi * w * w) - 1) <= 1e-3
    assert abs(res["mfd_petermann"][0] / (2 * w) - 1) <= 1e-3


def test_gamma_is_n2_k0_over_a_eff(fibre):
    g, _, em = fibre
    x, y = em.basis.doflocs
    vals = np.stack([np.exp(-(x * x + y * y) / 2.0 ** 2), np.exp(-((x - 0.5) ** 2 + y * y) / 3.0 ** 2) * x])[None]
    n2 = 2.6e-20
    pairs = em.quartic(vals, False)
    pairs_n2 = em.quartic(vals, False, g, (n2, n2))
    res = nonlinearity_from_pairs("scalar", pairs, em.grams(vals, False, g), k0=g.k0, pairs_n2=pairs_n2)
    want = 1e21 * g.k0 * n2 / res["a_eff"]
    assert np.allclose(res["gamma_self"], want, rtol=1e-13)
    assert res["gamma"].shape == (2,) * 4
    # n2_clad = 0: only the core contributes, so less than with the same n2 everywhere
    core_only = nonlinearity_from_pairs("scalar", pairs, em.grams(vals, False, g), k0=g.k0,
                                        pairs_n2=em.quartic(vals, False, g, (n2, 0.0)))
    assert np.all(core_only["gamma_self"] < res["gamma_self"])


def test_argument_errors_before_any_device_call(fibre):
    g, mesh, em = fibre
    ns, N = em.interior.size, em.N
    vec = [{"Ex_dofs": np.ones(ns), "Ey_dofs": np.ones(ns), "beta": 8.0}]
    scal = [{"field_vector": np.ones(N), "beta": 8.0}]
    bad = (([], {}), (vec + scal, {}),                                            # no records, mixed kinds
           ([{"Ex_dofs": np.ones(ns - 1), "Ey_dofs": np.ones(ns - 1)}], {}),    # wrong lengths
           ([{"field_vector": np.ones(N + 1)}], {}),
           (scal * 65, {}),                                                      # k > 64
           (scal, {"n2": (2.6e-20, 0.0)}),                                       # n2 without a geometry
           (scal, {"geometry": g, "n2": (np.nan, 0.0)}), (scal, {"geometry": g, "n2": (1e-20,)}),
           (scal, {"geometry": g, "n2": "ab"}), (scal, {"geometry": object()}))
    for modes, kw in bad:
        with pytest.raises(ValueError):
            mode_nonlinearity(modes, mesh, **kw)


def test_quartic_work_bytes_on_the_host(built_library):
    lib = _native.load_library()
    b = ctypes.c_int64(0)
    sizes = {}
    for k in range(1, 65):
        for nc in (1, 2):
            assert lib.plfem_quartic_work_bytes(nc, k, ctypes.byref(b)) == _native.PLFEM_OK
            npair = k * (k + 1) // 2
            assert b.value >= npair * npair * 8 and b.value % 8 == 0
            assert b.value <= npair * npair * 8 + 256 + 2048 * 64 * 64 * 8         # the bound of include/plfem.h
            sizes[nc, k] = b.value
    assert sizes[1, 22] == sizes[2, 22]
    for nc, k in ((2, 0), (2, 65), (0, 5), (3, 5), (1, -1)):
        assert lib.plfem_quartic_work_bytes(nc, k, ctypes.byref(b)) == _native.PLFEM_EINVAL
    assert lib.plfem_quartic_work_bytes(2, 5, None) == _native.PLFEM_EINVAL
    assert lib.plfem_mode_quartic(None, 2, 5, None, 1, None, 0, 1.0, 1.0, None, 0, None) == _native.PLFEM_EINVAL
