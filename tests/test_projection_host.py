"""Projection of modes on plane waves and Gaussian beams, host side (no GPU): the exact identities of the NumPy emulation
(kappa = 0 against the oracle's mass matrix, Hermitian symmetry, translation), the same P2 function on the red-refined
mesh (exact at kappa = 0; the printed difference at |kappa| <= k0 is the quadrature error of DESIGN.md section 15),
``encircled_na`` on an analytic far field, argument checking before any device call, and the two exported symbols."""
import ctypes

import numpy as np
import pytest
from scipy.sparse.linalg import eigsh

from oracle import scalar
from pl_fem_vectoriel_amd import ModeFields, _native, encircled_na, far_field, gaussian_coupling, generate_mesh
from projection_emulation import ProjectionEmulation


@pytest.fixture(scope="module")
def lantern(c1_geometry, built_library):
    """C1 at L = 0, six scalar modes of the oracle and five random interior-indexed vectorial fields."""
    g = c1_geometry
    mesh = generate_mesh(g, 0.5, 0)
    em = ProjectionEmulation(mesh.p, mesh.t)
    S, M, Me, _ = scalar.assemble(g, em.mesh)
    _, X = eigsh((S - g.k0 ** 2 * Me).tocsr(), k=6, M=M, sigma=scalar.shift(g), which="LM", tol=1e-12)
    scal = np.ascontiguousarray(X.T)[None]                                         # (1, 6, N)
    vec = np.random.default_rng(21).standard_normal((2, 5, em.interior.size))
    return {"mesh": mesh, "em": em, "M": M, "scal": scal, "vec": vec}


def _factors(g):
    """Plane waves up to k0 with +-kappa pairs and kappa = 0, and w = 1.5 beams on three cores with a tilt."""
    k0 = g.k0
    pos = np.atleast_2d(np.asarray(g.positions, dtype=np.float64))
    xf = [(0.0, 0.0, 0.0), (0.0, 0.0, k0), (0.0, 0.0, -k0), (0.0, 0.0, 0.37 * k0), (0.0, 0.0, -0.37 * k0)]
    yf = [(0.0, 0.0, 0.0), (0.0, 0.0, 0.81 * k0), (0.0, 0.0, -0.81 * k0)]
    s = 1.0 / 1.5 ** 2
    for (cx, cy), kap in zip(pos[:3], (0.0, 0.5, -0.5)):
        xf.append((cx, s, kap))
        yf.append((cy, s, -kap))
    return np.array(xf), np.array(yf)


def _negated(fac):
    out = fac.copy()
    out[:, 2] = -out[:, 2]
    return out


def _excess(got, ref, tol):
    """Largest |got - ref| / tol over the entries."""
    return float((np.abs(got - ref) / tol).max())


def test_kappa_zero_is_the_row_sum_of_the_mass_matrix(lantern):
    em, M = lantern["em"], lantern["M"]
    one = np.array([[0.0, 0.0, 0.0]])
    ones = np.ones(em.N)
    for vals, indexed in ((lantern["scal"], False), (lantern["vec"], True)):
        P = em.project(vals, indexed, one, one)
        assert P.shape == (vals.shape[0], vals.shape[1], 1, 1)
        assert np.all(P.imag == 0.0)
        full = np.zeros(vals.shape[:2] + (em.N,))
        full[:, :, em.interior if indexed else slice(None)] = vals
        ref = np.einsum("n,ckn->ck", M.T @ ones, full)[:, :, None, None]
        ex = _excess(P, ref, em.tolerance(vals, indexed, one, one))
        print(f"kappa = 0 against (M 1)^T u, indexed {indexed}: {ex:.2e} of the tolerance")
        assert ex <= 1.0


def test_hermitian_identity(lantern, c1_geometry):
    em = lantern["em"]
    xf, yf = _factors(c1_geometry)
    for vals, indexed in ((lantern["scal"], False), (lantern["vec"], True)):
        P = em.project(vals, indexed, xf, yf)
        Pn = em.project(vals, indexed, _negated(xf), _negated(yf))
        ex = _excess(Pn, np.conj(P), em.tolerance(vals, indexed, xf, yf))
        print(f"P(-kappa) = conj P(kappa), indexed {indexed}: {ex:.2e} of the tolerance")
        assert ex <= 1.0


def test_translation_identity(lantern, c1_geometry):
    em, mesh = lantern["em"], lantern["mesh"]
    d = np.array([0.5, -0.25])
    moved = ProjectionEmulation(mesh.p + d[:, None], mesh.t)
    xf, yf = _factors(c1_geometry)
    xm, ym = xf.copy(), yf.copy()
    xm[:, 0] += d[0]                                             # the Gaussian centres move along
    ym[:, 0] += d[1]
    shift = np.exp(-1j * (xf[None, :, 2] * d[0] + yf[:, None, 2] * d[1]))[None, None]
    for vals, indexed in ((lantern["scal"], False), (lantern["vec"], True)):
        P = em.project(vals, indexed, xf, yf)
        Pm = moved.project(vals, indexed, xm, ym)
        ex = _excess(Pm, P * shift, moved.tolerance(vals, indexed, xm, ym))
        print(f"translation by {tuple(d)}, indexed {indexed}: {ex:.2e} of the tolerance")
        assert ex <= 1.0


def test_same_function_on_the_refined_mesh(lantern, c1_geometry):
    em, vals = lantern["em"], lantern["scal"]
    fine_mesh = em.mesh.refined(1)
    fine = ProjectionEmulation(fine_mesh.p, fine_mesh.t)
    fv, elem = em.sample(vals, fine.basis.doflocs, False)       # the same piecewise-P2 function, exactly
    assert np.all(elem >= 0)
    one = np.array([[0.0, 0.0, 0.0]])
    ex = _excess(fine.project(fv, False, one, one), em.project(vals, False, one, one), fine.tolerance(fv, False, one, one))
    print(f"kappa = 0 on refined(1): {ex:.2e} of the tolerance")
    assert ex <= 1.0
    # the quadrature error proper: |kappa| up to k0 (and up to sqrt(2) k0 in the corners of the grid)
    k0 = c1_geometry.k0
    kap = np.linspace(-k0, k0, 9)
    fac = np.stack([np.zeros(9), np.zeros(9), kap], 1)
    S = em.scale(vals, False)[:, :, None, None]
    diff = np.abs(fine.project(fv, False, fac, fac) - em.project(vals, False, fac, fac)) / S
    radius = np.hypot(kap[None, :], kap[:, None])
    print(f"16-point rule against the same function on refined(1), {em.mesh.t.shape[1]} elements: "
          f"{diff[:, :, radius <= k0 * (1 + 1e-12)].max():.2e} S for |kappa| <= k0, {diff.max():.2e} S for |kappa| <= sqrt(2) k0")
    assert diff.max() < 0.05                                      # (an error of order S would be a wrong integrand)


def test_encircled_na_on_an_analytic_far_field():
    a, k0 = 3.0, 2 * np.pi / 1.55
    kx = np.linspace(-2.0, 2.0, 161)
    ky = np.linspace(-2.0, 2.0, 121)
    step = max(kx[1] - kx[0], ky[1] - ky[0])
    r2 = kx[None, :] ** 2 + ky[:, None] ** 2
    intensity = np.exp(-r2 * a * a / 4) ** 2                      # |F|^2 of F = exp(-kappa^2 a^2 / 4)
    for fraction in (0.5, 0.95, 0.99):
        want = np.sqrt(-2.0 * np.log(1.0 - fraction)) / a         # 1 - exp(-kappa_r^2 a^2 / 2) = fraction
        got = encircled_na(intensity, kx, ky, k0, fraction)
        assert abs(got * k0 - want) <= step, (fraction, got * k0, want)
    both = encircled_na(np.stack([intensity, intensity ** 4]), kx, ky, k0)
    assert both.shape == (2,) and both[1] < both[0]
    assert encircled_na(np.ones_like(intensity), kx, ky, k0, 1.0) * k0 == pytest.approx(np.hypot(2.0, 2.0))   # the corners
    for bad in (dict(fraction=0.0), dict(fraction=1.5), dict(k0=0.0), dict(k0=np.nan)):
        kw = dict(k0=k0, fraction=0.95)
        kw.update(bad)
        with pytest.raises(ValueError):
            encircled_na(intensity, kx, ky, **kw)
    with pytest.raises(ValueError):
        encircled_na(intensity[:, :-1], kx, ky, k0)
    with pytest.raises(ValueError):
        encircled_na(-intensity, kx, ky, k0)
    with pytest.raises(ValueError):
        encircled_na(np.zeros_like(intensity), kx, ky, k0)


def test_argument_errors_before_any_device_call(lantern, monkeypatch):
    mesh, em = lantern["mesh"], lantern["em"]
    ns, N = em.interior.size, em.N

    def no_device(self):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(ModeFields, "_ensure_locator", no_device)
    mf = ModeFields(mesh)
    vec = [{"Ex_dofs": np.ones(ns), "Ey_dofs": np.ones(ns), "beta": 8.0}]
    scal = [{"field_vector": np.ones(N), "beta": 8.0}]
    ok = np.array([[0.0, 0.0, 1.0]])
    bad_tables = (np.zeros((0, 3)), np.zeros((4097, 3)), np.zeros((3, 2)), np.zeros(3), [[0.0, -1.0, 0.0]],
                  [[np.nan, 0.0, 0.0]], [[0.0, np.inf, 0.0]], [[0.0, 0.0, -np.inf]], "ab", None)
    for bad in bad_tables:
        with pytest.raises(ValueError):
            mf.project(scal, bad, ok)
        with pytest.raises(ValueError):
            mf.project(scal, ok, bad)
    bad_modes = (vec + scal, [{"Ex_dofs": np.ones(ns - 1), "Ey_dofs": np.ones(ns - 1)}], [{"field_vector": np.ones(N + 1)}],
                 scal * 65, scal[0], [{"beta": 1.0}], [np.ones(N)])
    for modes in bad_modes:
        with pytest.raises(ValueError):
            mf.project(modes, ok, ok)
        with pytest.raises(ValueError):
            far_field(modes, mf, [0.0], [0.0])
        with pytest.raises(ValueError):
            gaussian_coupling(modes, mesh, 1.5, [0.0], [0.0])
    with pytest.raises(NotImplementedError):                      # complex records, as in the other ModeFields methods
        mf.project([{"field_vector": np.ones(N) + 0j}], ok, ok)
    empty = mf.project([], np.zeros((5, 3)), np.zeros((3, 3)))     # an empty mode list: an empty array, no device
    assert empty.shape == (0, 0, 3, 5) and empty.dtype == np.complex128
    for fn in (far_field, lambda m, msh, x, y: gaussian_coupling(m, msh, 1.5, x, y)):
        for x, y in (([], [0.0]), ([0.0], [np.nan]), ([[0.0]], [0.0]), (np.zeros(4097), [0.0]), ("ab", [0.0])):
            with pytest.raises(ValueError):
                fn(scal, mf, x, y)
        with pytest.raises(ValueError):
            fn([], mf, [0.0], [0.0])
        with pytest.raises(ValueError):
            fn(scal, object(), [0.0], [0.0])
    for kw in (dict(waist=0.0), dict(waist=-1.0), dict(waist=np.nan), dict(waist=np.inf), dict(waist="ab"), dict(waist=1e-200),
               dict(tilt=(0.0,)), dict(tilt=(np.nan, 0.0)), dict(tilt="ab"), dict(polarization=(0.0, 0.0)),
               dict(polarization=(1.0, 0.0, 0.0)), dict(polarization=(np.inf, 0.0))):
        args = dict(waist=1.5)
        args.update(kw)
        with pytest.raises(ValueError):
            gaussian_coupling(vec, mf, args.pop("waist"), [0.0], [0.0], **args)


def test_symbols_and_work_bytes_on_the_host(built_library):
    lib = ctypes.CDLL(_native.LIB_PATH)                           # the cross-compiled library itself
    for name in ("plfem_project_work_bytes", "plfem_mode_project"):
        assert name in _native.EXPORTS and hasattr(lib, name), name
    lib = _native.load_library()
    b = ctypes.c_int64(0)
    assert lib.plfem_project_work_bytes(2, 22, 64, 64, ctypes.byref(b)) == _native.PLFEM_OK
    result, tiles = 16 * 44 * 64 * 64, 64
    assert b.value >= result + 8 * 256 * 44 * tiles and b.value % 256 == 0
    assert b.value <= result + 2048 * 44 * 1024 + 4 * 256 + 2 * 24 * 64      # the bound of include/plfem.h
    assert lib.plfem_project_work_bytes(1, 64, 4096, 4096, ctypes.byref(b)) == _native.PLFEM_OK
    assert b.value >= 16 * 64 * 4096 * 4096                                 # (past 2^31: an int64)
    for nc, k, la, lb in ((0, 5, 4, 4), (3, 5, 4, 4), (1, 0, 4, 4), (1, 65, 4, 4), (1, 5, 0, 4), (1, 5, 4, 0), (1, 5, 4097, 4),
                          (1, 5, 4, 4097), (1, -1, 4, 4)):
        assert lib.plfem_project_work_bytes(nc, k, la, lb, ctypes.byref(b)) == _native.PLFEM_EINVAL
    assert lib.plfem_project_work_bytes(1, 5, 4, 4, None) == _native.PLFEM_EINVAL
    assert lib.plfem_mode_project(None, 1, 5, None, 0, 4, None, 4, None, None, 0, None) == _native.PLFEM_EINVAL
