"""Sampled index maps on the host: IndexProfile.epsilon with a map against a scalar loop of the model (cell, clamping,
closed extent, interpolation order, layers over the map) bit for bit, the premises of the edge sections, a bilinear
function reproduced to rounding, the emulated profile Grams against the oracle's pencils assembled with the same
geometry, every Python guard, the C entries without a device, copy / pickle / hash, and the oracle's record counts on
M3 and M3L."""
import copy
import ctypes
import math
import pickle

import numpy as np
import pytest

from map_cases import (M3_X, M3_Y, SQUARE_BG, SquareMaps, layers_only_profile, m3, m3_index, m3_profile, m3l, m3l_profile,
                       outside_profile)
from oracle import hfield, scalar
from oracle.p2 import MeshTriLite
from pl_fem_vectoriel_amd import IndexProfile, ModeFields, ProfiledGeometry, _native, core_decomposition, mode_dispersion
from profile_cases import three_core
from profile_gram_emulation import NAMES, ProfileGramEmulation
from test_dispersion_host import _rel


@pytest.fixture(scope="module")
def three(built_library):
    g, mesh = three_core()
    return g, mesh, ProfileGramEmulation(mesh.p, mesh.t)


@pytest.fixture(scope="module")
def square():
    return SquareMaps()


def loop_epsilon(profile, xs, ys):
    """The model one point at a time, in Python floats: the map (or the background), then the layers in their order."""
    m = profile.index_map
    if m is not None:
        E, x0, y0, dx, dy = m
        ny, nx = E.shape
        E = E.tolist()
        inv_dx, inv_dy = 1.0 / dx, 1.0 / dy
    layers = profile.table().tolist()
    out = []
    for x, y in zip(xs, ys):
        eps = profile.eps_background
        if m is not None:
            tx, ty = (x - x0) * inv_dx, (y - y0) * inv_dy
            if 0.0 <= tx <= nx - 1 and 0.0 <= ty <= ny - 1:
                i0, j0 = min(math.floor(tx), nx - 2), min(math.floor(ty), ny - 2)
                a, b = tx - i0, ty - j0
                a1, b1 = 1.0 - a, 1.0 - b
                lo = a1 * E[j0][i0] + a * E[j0][i0 + 1]
                hi = a1 * E[j0 + 1][i0] + a * E[j0 + 1][i0 + 1]
                eps = lo * b1 + hi * b
        for cx, cy, r_in, r_out, eps_a, eps_b, g, _ in layers:
            ddx, ddy = x - cx, y - cy
            d2 = ddx * ddx + ddy * ddy
            if r_in * r_in <= d2 <= r_out * r_out:
                eps = eps_a + (eps_b - eps_a) * math.pow(min(max((math.sqrt(d2) - r_in) / (r_out - r_in), 0.0), 1.0), g) if g > 0 else eps_a
        out.append(eps)
    return np.array(out)


def probe_points(profile, qx, qy):
    """The quadrature points, then the map's nodes, points on its four edges, points around its corners one ulp either
    way, points well outside, and a NaN."""
    E, x0, y0, dx, dy = profile.index_map
    ny, nx = E.shape
    gx, gy = x0 + dx * np.arange(nx), y0 + dy * np.arange(ny)
    NX, NY = np.meshgrid(gx, gy)
    t = np.random.default_rng(3).uniform(0, 1, 40)
    x1, y1 = x0 + dx * (nx - 1), y0 + dy * (ny - 1)
    ex = np.concatenate([x0 + (x1 - x0) * t, x0 + (x1 - x0) * t, np.full(40, x0), np.full(40, x1)])
    ey = np.concatenate([np.full(40, y0), np.full(40, y1), y0 + (y1 - y0) * t, y0 + (y1 - y0) * t])
    cx, cy = [], []
    for X in (x0, x1):
        for Y in (y0, y1):
            for sx in (-np.inf, 0, np.inf):
                for sy in (-np.inf, 0, np.inf):
                    cx.append(np.nextafter(X, sx) if sx else X)
                    cy.append(np.nextafter(Y, sy) if sy else Y)
    far = np.array([x0 - 3 * dx, x1 + 3 * dx, x0 - 1e6, 0.5 * (x0 + x1), np.nan, 0.5 * (x0 + x1)])
    fary = np.array([0.5 * (y0 + y1), 0.5 * (y0 + y1), y0, y1 + dy, y0, np.nan])
    xs = np.concatenate([np.ravel(qx), NX.ravel(), ex, cx, far])
    ys = np.concatenate([np.ravel(qy), NY.ravel(), ey, cy, fary])
    return xs, ys


def test_epsilon_matches_the_scalar_loop(three, square):
    g, mesh, em = three
    qx, qy = em.basis.qx
    for name, prof in (("M3", m3_profile()), ("M3L", m3l_profile()), ("outside", outside_profile())):
        xs, ys = probe_points(prof, qx, qy)
        got = prof.epsilon(xs, ys)
        assert got.shape == xs.shape and np.array_equal(got, loop_epsilon(prof, xs, ys)), name
    assert np.array_equal(outside_profile().epsilon(qx, qy), layers_only_profile().epsilon(qx, qy))
    for name, prof in square.profiles.items():
        xs, ys = probe_points(prof, square.qx, square.qy)
        assert np.array_equal(prof.epsilon(xs, ys), loop_epsilon(prof, xs, ys)), name
    # M3: the extent ends inside the mesh and cuts elements; n is up to 1.08 at its edge against the background of 1.0
    prof = m3_profile()
    E = prof.index_map[0]
    rim = np.sqrt(np.concatenate([E[0], E[-1], E[:, 0], E[:, -1]]).max())
    assert 1.07 < rim < 1.09 and prof.n_min == 1.0 and abs(prof.n_max - 1.533) < 1e-3
    eps = prof.epsilon(qx, qy)
    inside = (qx >= M3_X[0]) & (qx <= M3_X[-1]) & (qy >= M3_Y[0]) & (qy <= M3_Y[-1])
    cut = inside.any(axis=1) & ~inside.all(axis=1)
    assert cut.sum() > 50 and np.all(eps[~inside] == 1.0) and (~inside).sum() > 1000
    # the layers of M3L are painted over the map
    epsl = m3l_profile().epsilon(qx, qy)
    assert {1.530 ** 2, 1.40 ** 2} <= set(np.unique(epsl).tolist()) and (epsl != eps).sum() > 500
    # shapes and scalars, as for a profile without a map
    assert prof.epsilon(0.0, 0.0).shape == () and float(prof.epsilon(0.0, 0.0)) == loop_epsilon(prof, [0.0], [0.0])[0] > 2.0
    assert prof.epsilon(qx[:3], qy[:3]).shape == (3, 6)


def test_premises_of_the_edge_sections(square):
    S = square
    (e, q), (ef, qf) = S.left_target, S.far_target
    X, Y = float(S.qx[e, q]), float(S.qy[e, q])
    bare = IndexProfile(SQUARE_BG)
    for name in ("left", "left_out"):
        E, x0, y0, dx, dy = S.profiles[name].index_map
        assert E.shape == (5, 4) and x0 == S.left_x0[name] and abs(dx - 0.2) < 1e-15
        tx, ty = (X - x0) * (1.0 / dx), (Y - y0) * (1.0 / dy)
        assert 0.0 < ty < 4.0
        got = float(S.profiles[name].epsilon(X, Y))
        if name == "left":
            assert x0 == X and tx == 0.0
            j0 = math.floor(ty)
            b = ty - j0
            assert got == E[j0, 0] * (1.0 - b) + E[j0 + 1, 0] * b and got != SQUARE_BG ** 2
        else:
            assert x0 == np.nextafter(X, np.inf) and tx < 0.0 and got == SQUARE_BG ** 2
    assert float(bare.epsilon(X, Y)) == SQUARE_BG ** 2
    # far edge: x0 = X - 0.375 and X - x0 = 0.375, both exact; tx = 3 = nx - 1: the clamped cell with a = 1
    X, Y = float(S.qx[ef, qf]), float(S.qy[ef, qf])
    E, x0, y0, dx, dy = S.profiles["far"].index_map
    assert 0.1875 <= X <= 0.75 and dx == 0.125 and x0 == S.far_x0 and x0 + 0.375 == X and X - x0 == 0.375
    tx, ty = (X - x0) * (1.0 / dx), (Y - y0) * (1.0 / dy)
    assert tx == 3.0 and min(math.floor(tx), 4 - 2) == 2 and tx - 2 == 1.0
    j0 = math.floor(ty)
    b = ty - j0
    got = float(S.profiles["far"].epsilon(X, Y))
    assert got == E[j0, 3] * (1.0 - b) + E[j0 + 1, 3] * b and got != SQUARE_BG ** 2
    # past the edge the point is outside (2^-40 further: X - x0 itself rounds away single ulps of X)
    assert float(S.profiles["far"].epsilon(X + 2.0 ** -40, Y)) == SQUARE_BG ** 2
    # the 2 x 2 map: one cell, and it owns quadrature points
    two = S.profiles["two"].epsilon(S.qx, S.qy)
    assert S.profiles["two"].index_map[0].shape == (2, 2) and (two != SQUARE_BG ** 2).sum() > 300


def test_a_bilinear_function_is_reproduced_to_rounding():
    f = lambda x, y: 2.0 + 0.3 * x - 0.2 * y + 0.05 * x * y
    x, y = np.linspace(-1.0, 2.0, 7), np.linspace(0.5, 3.0, 11)
    X, Y = np.meshgrid(x, y)
    prof = IndexProfile(1.0).sampled(x, y, np.sqrt(f(X, Y)))
    rng = np.random.default_rng(11)
    px, py = rng.uniform(-1.0, 2.0, 5000), rng.uniform(0.5, 3.0, 5000)
    got = prof.epsilon(px, py)
    # n * n of sqrt(f) is within an ulp of f at the nodes, the weights carry an ulp of tx <= 6 each, four products and
    # three sums: 1e-14 of the largest value (3.6) is a dozen ulps
    assert np.abs(got - f(px, py)).max() <= 1e-14 * 3.6
    assert np.array_equal(prof.epsilon(X, Y), prof.index_map[0])       # at the nodes: the samples themselves
    assert float(prof.epsilon(2.5, 1.0)) == 1.0 and float(prof.epsilon(0.0, 0.25)) == 1.0


def test_emulated_profile_grams_reproduce_the_mapped_pencils(three, square):
    g, mesh, em = three
    cases = [("M3L", m3l(g), em), ("far", square.geometry("far"), ProfileGramEmulation(square.mesh.p, square.mesh.t))]
    for name, pg, em in cases:
        prof = pg.index_profile
        rng = np.random.default_rng(41)
        k, k0 = 5, pg.k0
        vals = rng.standard_normal((2, k, em.interior.size))
        G = em.profile_grams(vals, True, prof)
        assert tuple(G) == NAMES[2]
        V = np.hstack([vals[0], vals[1]]).T
        A, B, basis, *_ = hfield.assemble_hfield_system_fused(pg, em.mesh)
        A, B, _ = hfield.restrict_interior(A, B, basis)
        ea, eb = _rel(G["K_w"] + G["D"] - k0 ** 2 * G["M"], V.T @ (A @ V)), _rel(G["M_w"], V.T @ (B @ V))
        u = rng.standard_normal((1, k, em.N))
        Gs = em.profile_grams(u, False, prof)
        S, Mm, Me, _ = scalar.assemble(pg, em.mesh)
        U = u[0].T
        es, em_ = _rel(Gs["S"] - k0 ** 2 * Gs["M_w"], U.T @ ((S - k0 ** 2 * Me) @ U)), _rel(Gs["M"], U.T @ (Mm @ U))
        print(f"{name}: vectorial V^T A V {ea:.1e}, V^T B V {eb:.1e}; scalar V^T A V {es:.1e}, V^T B V {em_:.1e}")
        assert ea <= 1e-12 and eb <= 1e-12 and es <= 1e-12 and em_ <= 1e-12


def test_python_guards():
    x, y, n = np.linspace(0, 1, 4), np.linspace(0, 2, 5), np.full((5, 4), 1.4)
    p = IndexProfile(1.0)
    bad_n = [np.full((4, 5), 1.4), np.full((5, 4, 1), 1.4), np.full(20, 1.4), 1.4, "x", np.where(np.eye(5, 4) > 0, np.nan, 1.4),
             np.where(np.eye(5, 4) > 0, np.inf, 1.4), np.where(np.eye(5, 4) > 0, 0.0, 1.4), np.where(np.eye(5, 4) > 0, -1.4, 1.4),
             np.full((5, 4), 1e200)]
    for v in bad_n:
        with pytest.raises(ValueError):
            p.sampled(x, y, v)
    bad_axes = [np.array([0.0]), np.array([0.0, 1.0, 3.0]), np.array([1.0, 0.0]), np.array([0.0, 0.0]), np.array([0.0, np.nan]),
                np.array([0.0, np.inf]), np.zeros((2, 2)), "x", np.arange(8193.0), np.array([0.0, 1e-320])]
    for a in bad_axes:
        with pytest.raises(ValueError):
            p.sampled(a, y, np.full((5, np.size(a)), 1.4))
        with pytest.raises(ValueError):
            p.sampled(x, a, np.full((np.size(a), 4), 1.4))
    with pytest.raises(ValueError, match="2\\^24"):
        p.sampled(np.arange(8192.0), np.arange(4096.0), np.broadcast_to(1.4, (4096, 8192)))
    assert p.index_map is None and len(p) == 0                      # a refused map leaves the profile as it was
    assert p.sampled(x, y, n) is p and p.index_map[0].shape == (5, 4) and p.index_map[1:] == (0.0, 0.0, 1.0 / 3.0, 0.5)
    assert np.array_equal(p.index_map[0], n * n) and not p.index_map[0].flags.writeable
    n[0, 0] = 9.0                                                    # the profile keeps its own copy
    assert p.index_map[0][0, 0] == 1.4 * 1.4
    assert p.sampled([0.0, 2.0], [1.0, 2.0, 3.0], [[1.3, 1.2], [1.1, 1.6], [1.25, 1.0]]) is p       # a second call replaces
    assert p.index_map[0].shape == (3, 2) and (p.n_max, p.n_min) == (1.6, 1.0) and len(p) == 0
    q = IndexProfile(1.45).sampled([0.0, 2.0], [1.0, 2.0], [[1.3, 1.2], [1.1, 1.25]]).disc((0, 0), 1.0, 1.5)
    assert (q.n_max, q.n_min) == (1.5, 1.1) and q.table().shape == (1, 8)


def test_profiled_geometry_with_a_map(three, monkeypatch):
    g, mesh, em = three
    qx, qy = em.basis.qx
    with pytest.raises(ValueError, match="no layers"):               # neither layers nor a map: still no section
        ProfiledGeometry(g, IndexProfile(1.0))
    pg = m3(g, 1.40)                                                 # a map without layers is one
    assert isinstance(pg, ProfiledGeometry) and isinstance(pg, type(g)) and len(pg.index_profile) == 0
    assert (pg.n_core, pg.n_clad) == (pg.index_profile.n_max, 1.40) and m3(g).n_clad == 1.0
    e = pg.epsilon(qx, qy)
    assert e.dtype == np.complex128 and not e.imag.any() and np.array_equal(e.real, pg.index_profile.epsilon(qx, qy))
    for q in (copy.copy(pg), copy.deepcopy(pg), pickle.loads(pickle.dumps(pg))):
        assert type(q) is type(pg) and q.hash == pg.hash and (q.n_core, q.n_clad) == (pg.n_core, pg.n_clad)
        assert np.array_equal(q.index_profile.index_map[0], pg.index_profile.index_map[0])
        assert q.index_profile.index_map[1:] == pg.index_profile.index_map[1:]
        assert np.array_equal(q.epsilon(qx, qy), e)
    assert copy.deepcopy(pg).index_profile is not pg.index_profile and copy.copy(pg).index_profile is pg.index_profile
    # the hash covers the map's bytes and its grid, and is that of an equal map
    X, Y = np.meshgrid(M3_X, M3_Y)
    n = m3_index(X, Y)
    same = ProfiledGeometry(g, IndexProfile(1.0).sampled(M3_X, M3_Y, n), n_clad=1.40)
    n2 = n.copy()
    n2[7, 9] = np.nextafter(n2[7, 9], 2.0)
    other = ProfiledGeometry(g, IndexProfile(1.0).sampled(M3_X, M3_Y, n2), n_core=pg.n_core, n_clad=1.40)
    moved = ProfiledGeometry(g, IndexProfile(1.0).sampled(M3_X + 0.5, M3_Y, n), n_clad=1.40)
    scaled = ProfiledGeometry(g, IndexProfile(1.0).sampled(M3_X, M3_Y[0] + 1.01 * (M3_Y - M3_Y[0]), n), n_clad=1.40)
    hashes = [pg.hash, other.hash, moved.hash, scaled.hash, m3l(g, 1.40).hash, g.hash,
              ProfiledGeometry(g, layers_only_profile(), n_core=pg.n_core, n_clad=1.40).hash,
              ProfiledGeometry(g, outside_profile(), n_core=pg.n_core, n_clad=1.40).hash]
    assert same.hash == pg.hash and len(set(hashes)) == len(hashes)
    # the two-region entries refuse the geometry before anything reaches the device
    mf = ModeFields(mesh)
    monkeypatch.setattr(ModeFields, "_ensure_locator", lambda self: pytest.fail("the device was touched"))
    rng = np.random.default_rng(2)
    modes = [{"field_vector": rng.standard_normal(em.N), "beta": 6.0 + i, "n_eff": 1.48 + 0.01 * i} for i in range(3)]
    for call in (lambda: mf.grams(modes, pg), lambda: mf.core_grams(modes, pg), lambda: mf.moment_grams(modes, pg),
                 lambda: mf.quartic(modes, pg), lambda: mode_dispersion(modes, mf, pg), lambda: core_decomposition(modes, mf, pg)):
        with pytest.raises(ValueError, match="profile_grams"):
            call()
    assert set(mf.profile_grams([], pg)) == set()


def test_map_entries_refuse_a_null_handle(built_library):
    lib = _native.load_library()
    E = np.full((5, 4), 2.0)
    ptr = E.ctypes.data_as(ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    for entry in (lib.plfem_set_index_map, lib.plfem_locator_set_index_map):
        assert entry(null, ptr, 4, 5, 0.0, 0.0, 0.25, 0.25) == _native.PLFEM_EINVAL
        assert entry(null, None, 0, 0, 0.0, 0.0, 0.0, 0.0) == _native.PLFEM_EINVAL
        assert entry(null, None, 4, 5, 0.0, 0.0, 0.25, 0.25) == _native.PLFEM_EINVAL
    assert {"plfem_set_index_map", "plfem_locator_set_index_map"} <= set(_native.EXPORTS)


def test_the_oracle_counts_on_m3_and_m3l(three):
    """The condition of the GPU parity tests: the reference's own filters keep these records, and at n_clad = 1.40 its
    shift lands at n = 1.45, where exactly one vectorial record is confined; the rest are box modes of the air region in
    exact pairs, whose x / y split is not defined."""
    g, mesh, em = three
    om = MeshTriLite(mesh.p, mesh.t)
    for make in (m3, m3l):
        pg = make(g)
        assert len(scalar.solve(pg, om, 10)) == 18
        assert len(hfield.solve_vectorial_modes(pg, om, n_modes_target=10, fused=True)) == 22
    pg = m3(g, 1.40)
    assert len(scalar.solve(pg, om, 10)) == 13
    vec = hfield.solve_vectorial_modes(pg, om, n_modes_target=10, fused=True)
    assert len(vec) == 22
    confined = [m for m in vec if m["confinement"] > 0.5]
    assert len(confined) == 1 and round(confined[0]["confinement"], 2) == 0.75 and round(confined[0]["n_eff"], 5) == 1.45022
    assert all(abs(m["n_eff"] - 1.45) < 0.005 for m in vec)
