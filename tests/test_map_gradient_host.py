"""Pixel gradients of sampled index maps on the host: the point-order emulation of plfem_index_map_gradients against the
tangent-Gram emulation (linearity in the map), its support against a direct count, the edge points of the square maps,
the host math of index_map_gradient against central differences of the oracle's dense eigenproblem, and the Python
argument errors."""
import copy
import ctypes
import math

import numpy as np
import pytest
import scipy.linalg

from map_cases import SquareMaps, m3, m3l
from map_gradient_emulation import NAMES, MapGradientEmulation
from oracle import hfield, scalar
from pl_fem_vectoriel_amd import ModeFields, ProfiledGeometry, _native, index_map_gradient, index_map_gradient_from_densities
from profile_cases import p5, three_core
from tangent_gram_emulation import TangentGramEmulation

KINDS = ("vectorial", "scalar")
# worst |HF - FD| of d n_eff / d n over the modes and pixels of test_gradient_against_central_differences_of_the_oracle_
# eigenproblem, measured on the CPU with the oracle's pencils and this file's emulation (3.10e-09 on "two", 5.52e-09 on
# "left"): central-difference truncation plus the roundoff of eigh over 2e-5.  The test asserts ten
# times this.
FD_WORST = 5.52e-9


@pytest.fixture(scope="module")
def square():
    return SquareMaps()


@pytest.fixture(scope="module")
def three():
    g, mesh = three_core()
    return g, mesh


def _sections(square, three):
    g, mesh = three
    out = [(nm, square.profiles[nm], square.mesh) for nm in ("two", "left", "left_out", "far")]
    return out + [("m3", m3(g).index_profile, mesh), ("m3l", m3l(g).index_profile, mesh)]


def _random_vals(em, ncomp, k, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((ncomp, k, em.interior.size if ncomp == 2 else em.N))


def test_emulation_contracted_with_a_tangent_map_is_the_tangent_gram_diagonal(square, three):
    for name, prof, mesh in _sections(square, three):
        em, tem = MapGradientEmulation(mesh.p, mesh.t), TangentGramEmulation(mesh.p, mesh.t)
        D = np.random.default_rng(11).uniform(-1.0, 1.0, prof.index_map[0].shape)
        tangent = prof.tangent_eps(0.0, 0.0, D)
        for ncomp in (2, 1):
            vals = _random_vals(em, ncomp, 3, seed=50 + ncomp)
            out, support = em.map_gradients(vals, ncomp == 2, prof)
            ref = tem.tangent_grams(vals, ncomp == 2, prof, [tangent])[0]            # (nout, k, k)
            assert out.shape == (3, len(NAMES[ncomp])) + D.shape and support.dtype == np.int32
            for o, nm in enumerate(NAMES[ncomp]):
                for r in range(3):
                    got, scale = float((D * out[r, o]).sum()), float((np.abs(D) * np.abs(out[r, o])).sum())
                    assert abs(got - ref[o][r, r]) <= 1e-12 * scale, (name, ncomp, nm, r)
                    assert scale > 0
            assert np.all(out[:, :, support == 0] == 0.0)


def test_support_is_a_direct_count(square, three):
    """One point at a time, in Python floats: the extent test and the cell of the model, the layers' closed rims."""
    for name, prof, mesh in _sections(square, three):
        em = MapGradientEmulation(mesh.p, mesh.t)
        _, support = em.map_gradients(_random_vals(em, 1, 1, 3), False, prof)
        E, x0, y0, dx, dy = prof.index_map
        ny, nx = E.shape
        inv_dx, inv_dy = 1.0 / dx, 1.0 / dy
        layers = prof.table().tolist()
        qx, qy = em.basis.qx
        count = np.zeros((ny, nx), dtype=np.int64)
        for X, Y in zip(qx.ravel().tolist(), qy.ravel().tolist()):
            tx, ty = (X - x0) * inv_dx, (Y - y0) * inv_dy
            if not (0.0 <= tx <= nx - 1 and 0.0 <= ty <= ny - 1):
                continue
            if any(r_in * r_in <= (X - cx) * (X - cx) + (Y - cy) * (Y - cy) <= r_out * r_out for cx, cy, r_in, r_out, *_ in layers):
                continue
            i0, j0 = min(math.floor(tx), nx - 2), min(math.floor(ty), ny - 2)
            count[j0:j0 + 2, i0:i0 + 2] += 1
        assert np.array_equal(support, count), name
        assert support.sum() > 0 and support.sum() % 4 == 0


def test_edge_points_of_the_square_maps(square):
    em = MapGradientEmulation(square.mesh.p, square.mesh.t)
    e, q = square.left_target
    f_left = {nm: em.contributions(square.profiles[nm], 1)[0] for nm in ("left", "left_out")}
    assert 6 * e + q in f_left["left"] and 6 * e + q not in f_left["left_out"]
    # far_target: tx = nx - 1 exactly, the clamped cell i0 = nx - 2 with a = 1: its whole weight is on column nx - 1
    e, q = square.far_target
    prof = square.profiles["far"]
    f, i0, j0, a, b, c = em.contributions(prof, 1)
    at = int(np.nonzero(f == 6 * e + q)[0][0])
    nx = prof.index_map[0].shape[1]
    assert i0[at] == nx - 2 and a[at] == 1.0 and c[at] != 0.0
    # alone on the mesh it feeds column nx - 1 only: one field that is 1 everywhere, every other point's c removed
    one = np.ones((1, 1, em.N))
    dens = em.point_densities(one, False)[0, 0]
    plane = np.zeros(prof.index_map[0].shape)
    a1, b1 = 1.0 - a[at], 1.0 - b[at]
    for dj, di, beta in ((0, 0, a1 * b1), (0, 1, a[at] * b1), (1, 0, a1 * b[at]), (1, 1, a[at] * b[at])):
        plane[j0[at] + dj, i0[at] + di] += c[at] * beta * dens[f[at]]
    assert np.all(plane[:, :nx - 1] == 0.0) and plane[:, nx - 1].sum() != 0.0


# ---- the host math against central differences of the oracle's dense eigenproblem ------------------------------------
def _with_pixel(profile, j, i, dn):
    """A copy of ``profile`` whose pixel (j, i) has its index moved by ``dn``."""
    q = copy.deepcopy(profile)
    E, *grid = profile.index_map
    E2 = E.copy()
    E2[j, i] = (np.sqrt(E[j, i]) + dn) ** 2
    E2.setflags(write=False)
    q._map = (E2, *grid)
    return q


def _dense_modes(kind, pg, mesh):
    """Every eigenpair of the oracle's dense pencil: ``(mu ascending, vectors as columns)``."""
    if kind == "vectorial":
        A, B, basis, *_ = hfield.assemble_hfield_system_fused(pg, mesh)
        A, B, _ = hfield.restrict_interior(A, B, basis)
    else:
        S, B, Me, _ = scalar.assemble(pg, mesh)
        A = S - pg.k0 ** 2 * Me
    A, B = A.toarray(), B.toarray()
    return scipy.linalg.eigh(0.5 * (A + A.T), 0.5 * (B + B.T))


def _isolated(kind, mu, rgap=1e-6, most=4):
    """Indices of guided-side eigenvalues (beta^2 > 0) whose relative gap to both neighbours exceeds ``rgap``, the ``most``
    with the largest n_eff."""
    b2 = mu if kind == "vectorial" else -mu
    order = np.argsort(-b2)
    picked = []
    for pos, m in enumerate(order):
        if b2[m] <= 0:
            break
        near = [abs(b2[m] - b2[order[p]]) for p in (pos - 1, pos + 1) if 0 <= p < order.size]
        if min(near) > rgap * abs(b2[m]):
            picked.append(int(m))
    return picked[:most]


@pytest.mark.parametrize("name", ["two", "left"])
def test_gradient_against_central_differences_of_the_oracle_eigenproblem(square, name):
    """Measured with the oracle alone (worst |HF - FD| of d n_eff / d n over modes and pixels): DESIGN.md section 32."""
    pg = square.geometry(name)
    prof = pg.index_profile
    em = MapGradientEmulation(square.mesh.p, square.mesh.t)
    mesh, k0, h = em.mesh, pg.k0, 1e-5
    n_map = np.sqrt(prof.index_map[0])
    support = em.map_gradients(np.zeros((1, 1, em.N)), False, prof)[1]
    seen = np.argwhere(support > 0)
    pixels = list(dict.fromkeys([tuple(seen[0]), tuple(seen[len(seen) // 2]), tuple(seen[-1]),
                                 tuple(np.unravel_index(np.argmax(support), support.shape))]))
    assert len(pixels) >= 3
    worst = 0.0
    for kind in KINDS:
        mu, X = _dense_modes(kind, pg, mesh)
        pick = _isolated(kind, mu)
        assert len(pick) >= 3, (kind, len(pick))
        beta = np.sqrt(np.abs(mu[pick]))
        if kind == "vectorial":
            n = em.interior.size
            vals = np.stack([X[:n, pick].T, X[n:, pick].T])
        else:
            vals = X[:, pick].T[None]
        vals = np.ascontiguousarray(vals)
        out, sup = em.map_gradients(vals, kind == "vectorial", prof)
        dens = em.named(out, sup)
        grams = em.profile_grams(vals, kind == "vectorial", prof)
        res = index_map_gradient_from_densities(kind, grams, dens, beta, k0, n_map)
        assert np.all(res["cluster"] == -1) and np.array_equal(res["dneff_dn"], res["dneff_dn_cluster"])
        for j, i in pixels:
            neff = []
            for s in (1.0, -1.0):
                moved = ProfiledGeometry(square.base, _with_pixel(prof, j, i, s * h), n_core=1.535, n_clad=pg.n_clad)
                mu_s, _ = _dense_modes(kind, moved, mesh)
                neff.append(np.sqrt(np.abs(mu_s[pick])) / k0)
            fd = (neff[0] - neff[1]) / (2 * h)
            err = np.abs(res["dneff_dn"][:, j, i] - fd)
            print(f"{name} {kind} pixel ({j}, {i}): dn_eff/dn = {res['dneff_dn'][:, j, i]}, |HF - FD| = {err}")
            assert np.abs(fd).max() > 1e-6
            worst = max(worst, float(err.max()))
    print(f"{name}: worst |HF - FD| = {worst:.2e}")
    assert worst <= 10 * FD_WORST


def test_from_densities_cluster_means_and_argument_errors():
    rng = np.random.default_rng(2)
    k, shape = 4, (3, 5)
    beta = np.array([5.0, 5.0, 4.5, 4.0])
    dens = {"M_px": rng.standard_normal((k,) + shape), "K_px": rng.standard_normal((k,) + shape), "support": np.ones(shape, dtype=np.int32)}
    grams = {"M_w": np.diag([1.0, 2.0, 3.0, 4.0]), "M": np.diag([1.0, 2.0, 3.0, 4.0])}
    n_map = rng.uniform(1.3, 1.5, shape)
    for kind in KINDS:
        res = index_map_gradient_from_densities(kind, grams, dens, beta, 4.0, n_map)
        assert list(res["cluster"]) == [0, 0, -1, -1] and np.array_equal(res["norm"], [1.0, 2.0, 3.0, 4.0])
        mean = res["dneff_deps"][:2].mean(axis=0)
        assert np.array_equal(res["dneff_deps_cluster"][0], mean) and np.array_equal(res["dneff_deps_cluster"][1], mean)
        assert np.array_equal(res["dneff_deps_cluster"][2:], res["dneff_deps"][2:])
        assert np.array_equal(res["dneff_dn"], 2.0 * n_map[None] * res["dneff_deps"])
        if kind == "scalar":                                             # -(-k0^2 M_px / N) / (2 beta k0)
            assert np.allclose(res["dneff_deps"], 16.0 * dens["M_px"] / np.diag(grams["M"])[:, None, None] / (8.0 * beta)[:, None, None],
                               rtol=1e-15)
        else:
            want = (dens["K_px"] - (beta ** 2)[:, None, None] * dens["M_px"]) / np.diag(grams["M_w"])[:, None, None] / (8.0 * beta)[:, None, None]
            assert np.allclose(res["dneff_deps"], want, rtol=1e-15)
    for bad in (dict(kind="other"), dict(beta=beta[:3]), dict(beta=-beta), dict(k0=0.0), dict(n_map=n_map[0]), dict(cluster_rtol=-1.0),
                dict(densities={"M_px": dens["M_px"]}), dict(grams={}), dict(grams={"M_w": -np.eye(4), "M": -np.eye(4)})):
        kw = dict(kind="vectorial", grams=grams, densities=dens, beta=beta, k0=4.0, n_map=n_map, cluster_rtol=1e-10)
        kw.update(bad)
        with pytest.raises(ValueError):
            index_map_gradient_from_densities(**kw)


def test_python_argument_errors(built_library, three, square):
    g, mesh = three
    mf = ModeFields(mesh)
    modes = [{"field_vector": np.zeros(mf.N), "beta": 5.0} for _ in range(3)]
    with pytest.raises(ValueError, match="index profile"):
        mf.index_map_densities(modes, g)
    with pytest.raises(ValueError, match="sampled map"):
        mf.index_map_densities(modes, p5(g))
    for basis in (np.zeros((2, 4)), np.zeros(3), np.full((2, 3), np.nan), "x"):
        with pytest.raises(ValueError, match="basis"):
            mf.index_map_densities(modes, m3(g), basis=basis)
    with pytest.raises(ValueError, match="index profile"):
        index_map_gradient(modes, mf, g)
    with pytest.raises(ValueError, match="sampled map"):
        index_map_gradient(modes, mf, p5(g))
    with pytest.raises(ValueError, match="no mode records"):
        index_map_gradient([], mf, m3(g))
    # no fields: empty arrays of the right shapes, nothing touches the device
    for kind_modes, names in (([], ("M_px", "K_px", "support")), (modes, ("M_px", "support"))):
        res = mf.index_map_densities(kind_modes, m3(g), basis=None if not kind_modes else np.zeros((0, 3)))
        assert tuple(res) == names and res["M_px"].shape == (0, 33, 41) and res["support"].shape == (33, 41)
        assert res["support"].dtype == np.int32 and mf._loc is None


def test_entries_are_exported_and_refuse_a_null_locator(built_library):
    lib = _native.load_library()
    assert {"plfem_index_map_gradient_work_bytes", "plfem_index_map_gradients"} <= set(_native.EXPORTS)
    b = ctypes.c_int64(-7)
    assert lib.plfem_index_map_gradient_work_bytes(None, 2, 3, ctypes.byref(b)) == _native.PLFEM_EINVAL and b.value == -7
    one = np.zeros(8).ctypes.data_as(ctypes.c_void_p)
    assert lib.plfem_index_map_gradients(None, 2, 3, one, 1, one, 0, 1.0, one, 0, one, one) == _native.PLFEM_EINVAL
