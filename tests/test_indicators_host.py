"""The NumPy restatement of the error indicators (tests/indicator_emulation.py) against the oracle's assembled pencils and
against what the definition implies: the signed pieces reproduce (A - lambda B) h of both pencils, a field that is one
global quadratic has no jumps, and eta2 scales with the square of the field."""
import numpy as np
import pytest

from core_ties import jittered_square_mesh
from indicator_emulation import IndicatorEmulation, eps_of
from oracle import hfield, scalar
from oracle.p2 import MeshTriLite

K0 = 2 * np.pi / 1.55
EPS = 2.25


class Uniform:
    """No cores, one permittivity != 1 everywhere."""
    k0, n_core, n_clad = K0, 1.535, 1.5
    positions, core_radii = np.zeros((0, 2)), np.zeros(0)

    def epsilon(self, x, y):
        return np.full(np.shape(x), EPS) + 0j


@pytest.fixture(scope="module")
def square():
    mesh = jittered_square_mesh(5)
    return mesh, IndicatorEmulation(mesh.p, mesh.t)


def uniform_eps(x, y):
    return np.full(np.shape(x), EPS)


@pytest.mark.parametrize("kind", ["scalar", "vectorial"])
def test_signed_pieces_reproduce_the_assembled_pencil(square, kind):
    mesh, emu = square
    om = MeshTriLite(mesh.p, mesh.t)
    rng = np.random.default_rng(3)
    lam = np.array([30.0, -7.5])
    if kind == "scalar":
        Kc, M, Me, basis = scalar.assemble(Uniform(), om)
        A, B, ncomp = (Kc - K0 ** 2 * Me).tocsr(), M, 1
    else:
        A, B, basis = hfield.assemble_hfield_system_fused(Uniform(), om)[:3]
        ncomp = 2
    N = basis.N
    assert N == emu.N
    h = rng.standard_normal((ncomp, 2, N))
    got = emu.signed_residual(h, lam, K0, 1.0, uniform_eps)
    for m in range(2):
        x = h[:, m].reshape(-1)
        want = A @ x - lam[m] * (B @ x)
        err = np.abs(got[:, m].reshape(-1) - want).max() / np.abs(want).max()
        print(f"{kind} lambda {lam[m]}: max error {err:.1e} of the largest entry")
        assert err <= 1e-11


@pytest.mark.parametrize("kind", ["scalar", "vectorial"])
def test_a_global_quadratic_has_no_jumps(square, kind):
    mesh, emu = square
    x, y = emu.basis.doflocs
    rng = np.random.default_rng(5)
    ncomp = 1 if kind == "scalar" else 2
    c = rng.standard_normal((ncomp, 2, 6))
    h = (c[..., 0, None] + c[..., 1, None] * x + c[..., 2, None] * y + c[..., 3, None] * x * x + c[..., 4, None] * x * y
         + c[..., 5, None] * y * y)                              # P2 interpolates a quadratic exactly
    lam = np.array([30.0, -7.5])
    res, jmp = emu.eta2_parts(h, False, lam, K0, 1.0, uniform_eps)
    if kind == "scalar":                                         # the natural-boundary flux is no jump: interior edges only
        P = emu.pieces(h, False, lam, K0, 1.0, uniform_eps)
        interior = (emu.nbr >= 0)[None, None, :, :, None]
        worst = np.abs((P["flux"][0] - P["flux"][1]) * interior).max() / np.abs(P["flux"][0]).max()
        print(f"scalar: largest interior jump {worst:.1e} of the largest flux")
        assert worst <= 1e-12
        inner = np.all(emu.nbr >= 0, axis=0)
        assert np.all(jmp[:, inner] <= 1e-12 * res[:, inner])
    else:
        print(f"vectorial: jump terms at most {np.max(jmp / res):.1e} of the residual terms")
        assert np.all(jmp <= 1e-12 * res)
    assert np.all(res > 0)


@pytest.mark.parametrize("kind", ["scalar", "vectorial"])
def test_eta2_scales_with_the_square_of_the_field(square, kind):
    mesh, emu = square
    ncomp = 1 if kind == "scalar" else 2
    rng = np.random.default_rng(7)
    h = rng.standard_normal((ncomp, 3, emu.N))
    lam = np.array([30.0, -7.5, 2.0])

    class Disc(Uniform):
        positions, core_radii = np.array([[0.4, 0.55]]), np.array([0.23])
        n_core, n_clad = 1.535, 1.2

    eps = eps_of(Disc())
    a = emu.eta2(h, False, lam, K0, 1.0, eps)
    b = emu.eta2(-3.0 * h, False, lam, K0, 1.0, eps)
    assert a.shape == (3, mesh.t.shape[1]) and np.all(a > 0)
    assert np.abs(b - 9.0 * a).max() <= 1e-13 * a.max()
    # an indexed record is the full one with zeros on the boundary
    hi = h[:, :, emu.interior]
    full = np.zeros_like(h)
    full[:, :, emu.interior] = hi
    assert np.array_equal(emu.eta2(hi, True, lam, K0, 1.0, eps), emu.eta2(full, False, lam, K0, 1.0, eps))
