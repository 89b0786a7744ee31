"""Posed flux overlap, host side (no GPU): the NumPy emulation (tests/flux_overlap_emulation.py) against the power emulation
at the identity pose, against itself on a mesh moved by the pose on the host, and against the closed forms of quadratic
fields; the k x k host math of ``flux_transfer_from_grams``; every Python argument error with no device present; and what
the sizer rejects without a locator."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import power_cases
from flux_overlap_emulation import (NAMES, OUTSIDE, centred_profile, ka_closed_form, moved_discs, posed_flux, profiled,
                                    rim_disc_geometry, uniform_geometry)
from pose_overlap_emulation import COVERING, IDENTITY, moved_mesh, moved_records, small_meshes
from power_emulation import PowerEmulation
from pl_fem_vectoriel_amd import (ModeFields, flux_overlap_poses, flux_transfer_from_grams, splice_power_map,
                                  taper_transfer_vectorial)

SHIFT = (0.15, -0.1, 1.0, 0.0, 1.0)
QUARTER = (0.05, 0.1, 0.0, 1.0, 0.9)                     # an exact quarter turn


def rel(a, ref):
    return np.abs(a - ref).max() / np.abs(ref).max()


@pytest.fixture(scope="module")
def pair():
    mesh_a, mesh_b = small_meshes()
    S = SimpleNamespace(mesh_a=mesh_a, mesh_b=mesh_b, em_a=PowerEmulation(mesh_a.p, mesh_a.t), em_b=PowerEmulation(mesh_b.p, mesh_b.t))
    rng = np.random.default_rng(41)
    S.ra = power_cases.records(rng, S.em_a.interior.size, 5)
    S.rb = power_cases.records(rng, S.em_b.interior.size, 4)
    S.discs, S.rim_point = rim_disc_geometry(S.em_b)
    return S


@pytest.mark.parametrize("material", ["discs", "profile"])
def test_identity_pose_of_a_set_on_itself_is_the_flux_grams(pair, material):
    g = pair.discs if material == "discs" else profiled(centred_profile(), pair.discs)
    v = power_cases.vals_of(pair.rb)
    out, elem = posed_flux(pair.em_b, v, g, pair.em_b, v, g, True, IDENTITY)
    assert (elem >= 0).all()
    ref = pair.em_b.flux_grams(v, True, g)
    M, G = ref["M_w_core"] + ref["M_w_rest"], ref["G_w_core"] + ref["G_w_rest"]
    errs = {"MA": rel(out["MA"], M), "MB": rel(out["MB"], M), "GA": rel(out["GA"], G), "GB": rel(out["GB"], G.T)}
    print(material, {nm: f"{e:.2e}" for nm, e in errs.items()})
    assert max(errs.values()) <= 1e-12, errs


@pytest.mark.parametrize("pose", [SHIFT, QUARTER, COVERING], ids=["shift", "quarter turn", "covering magnification"])
def test_emulation_against_a_host_moved_mesh(pair, pose):
    """A posed by the kernel's arithmetic against A moved on the host (mesh, records and discs) under the identity pose.
    g is made of second derivatives, so on the mesh magnified by m it is A's own turned and divided by m^2."""
    va, vb = power_cases.vals_of(pair.ra), power_cases.vals_of(pair.rb)
    ga = power_cases.discs([[0.3, -0.2], [-0.6, 0.5]], [0.45, 0.3], n_core=1.535, n_clad=1.0)
    out, elem = posed_flux(pair.em_a, va, ga, pair.em_b, vb, pair.discs, True, pose)
    assert (elem >= 0).all()
    mm = moved_mesh(pair.mesh_a, pose)
    ref, _ = posed_flux(PowerEmulation(mm.p, mm.t), power_cases.vals_of(moved_records(pair.ra, pose)), moved_discs(ga, pose),
                        pair.em_b, vb, pair.discs, True, IDENTITY)
    ref["GA"] = ref["GA"] * pose[4] ** 2
    errs = {nm: rel(out[nm], ref[nm]) for nm in NAMES}
    print(pose, {nm: f"{e:.2e}" for nm, e in errs.items()})
    assert max(errs.values()) <= 1e-12, errs
    if pose is QUARTER:
        # the turn matters: the unturned records on the moved mesh give other matrices
        bad, _ = posed_flux(PowerEmulation(mm.p, mm.t), va, moved_discs(ga, pose), pair.em_b, vb, pair.discs, True, IDENTITY)
        assert rel(bad["MA"], ref["MA"]) > 1e-3


def test_closed_form_of_quadratic_fields(pair):
    """A global quadratic is exact in P2 on any mesh, its g is constant, and the integrand on each element of B has
    degree 4: the six-point rule is exact."""
    g = uniform_geometry()
    va = power_cases.ka_all_dof_vectors(pair.em_a.basis.doflocs)
    vb = power_cases.ka_all_dof_vectors(pair.em_b.basis.doflocs)
    for pose in (COVERING, IDENTITY):
        out, elem = posed_flux(pair.em_a, va, g, pair.em_b, vb, g, False, pose)
        assert (elem >= 0).all()
        ref = ka_closed_form(pose)
        errs = {nm: rel(out[nm], ref[nm]) for nm in NAMES}
        print(pose, {nm: f"{e:.2e}" for nm, e in errs.items()})
        assert max(errs.values()) <= 1e-12, errs


def test_the_outside_pose_and_the_rim_point(pair):
    va, vb = power_cases.vals_of(pair.ra), power_cases.vals_of(pair.rb)
    out, elem = posed_flux(pair.em_a, va, pair.discs, pair.em_b, vb, pair.discs, True, OUTSIDE)
    share = float(np.mean(elem < 0))
    assert 1 / 3 <= share <= 2 / 3, share
    assert all(np.abs(out[nm]).max() > 0 for nm in NAMES)
    # the rim point counts as core: moving the disc's radius one ulp down changes the weights of that point alone
    qx = pair.em_b.basis.qx.reshape(2, -1)
    X, Y = qx[:, pair.rim_point]
    cx, cy, r = pair.discs.positions[0][0], pair.discs.positions[0][1], pair.discs.core_radii[0]
    assert (X - cx) ** 2 + (Y - cy) ** 2 == r * r


# -- flux_transfer_from_grams ------------------------------------------------------------------------------------------
def _self_grams(rng, k):
    """M (symmetric positive definite) and G of a made-up set, with its betas."""
    Q = rng.standard_normal((k, k))
    return Q @ Q.T + k * np.eye(k), 0.1 * rng.standard_normal((k, k)), rng.uniform(5, 10, k)


def test_a_set_onto_itself_is_the_identity_when_power_orthogonal():
    k, k0 = 4, 4.0
    beta = np.array([9.0, 8.0, 7.5, 6.0])
    M, G = np.diag([1.0, 2.0, 0.5, 3.0]), np.diag([0.3, -0.2, 0.1, 0.4])
    P = (beta * np.diag(M) + np.diag(G) / beta) / (2 * k0)
    r = flux_transfer_from_grams(M, G, M, G.T, beta, k0, beta, k0, P, P, 1.0)
    assert np.abs(r["transfer"] - np.eye(k)).max() <= 1e-15
    assert abs(r["IL_dB"]) <= 1e-14 and abs(r["MDL_dB"]) <= 1e-14
    assert np.abs(r["singular_values"] - 1).max() <= 1e-15 and np.array_equal(r["power"], r["transfer"] ** 2)
    # the diagonal is 1 for any set: X_ab[i, i] = X_ba[i, i] = 2 P_i
    M, G, beta = _self_grams(np.random.default_rng(5), 3)
    P = np.diag((beta[:, None] * M + G / beta[:, None]) / (2 * k0))
    r = flux_transfer_from_grams(M, G, M, G.T, beta, k0, beta, k0, P, P)
    assert np.abs(np.diag(r["transfer"]) - 1).max() <= 1e-14


def test_a_hand_made_two_by_two_case():
    MA = np.array([[2.0, 1.0], [0.0, 4.0]])
    GA = np.array([[1.0, 0.0], [2.0, -2.0]])
    MB = np.array([[1.0, 3.0], [2.0, 0.0]])
    GB = np.array([[0.0, 4.0], [4.0, 2.0]])
    ba, bb, k0 = np.array([2.0, 4.0]), np.array([1.0, 2.0]), 2.0
    pa, pb = np.array([4.0, -1.0]), np.array([1.0, 4.0])
    X_ab = np.array([[(2 * 2.0 + 1.0 / 2) / 2, (2 * 1.0 + 0.0) / 2], [(4 * 0.0 + 2.0 / 4) / 2, (4 * 4.0 - 2.0 / 4) / 2]])
    X_ba = np.array([[(1 * 1.0 + 0.0) / 2, (2 * 3.0 + 4.0 / 2) / 2], [(1 * 2.0 + 4.0) / 2, (2 * 0.0 + 2.0 / 2) / 2]])
    norm = np.array([[np.sqrt(4.0 * 1.0), np.sqrt(4.0 * 4.0)], [np.sqrt(1.0 * 1.0), np.sqrt(1.0 * 4.0)]])
    T = ((X_ab + X_ba) / (4 * norm)).T
    r = flux_transfer_from_grams(MA, GA, MB, GB, ba, k0, bb, k0, pa, pb)
    assert np.abs(r["transfer"] - T).max() <= 1e-15
    sv = np.linalg.svd(T, compute_uv=False)
    assert np.abs(r["singular_values"] - sv).max() <= 1e-15
    assert abs(r["IL_dB"] + 10 * np.log10(np.mean(sv ** 2))) <= 1e-13
    assert abs(r["MDL_dB"] - 10 * np.log10(sv[0] ** 2 / sv[1] ** 2)) <= 1e-12
    # a stack of poses is pose by pose
    r3 = flux_transfer_from_grams(np.stack([MA, 2 * MA]), np.stack([GA, 2 * GA]), np.stack([MB, 2 * MB]), np.stack([GB, 2 * GB]),
                                  ba, k0, bb, k0, pa, pb, [1.0, 1.0])
    assert r3["transfer"].shape == (2, 2, 2) and np.array_equal(r3["transfer"][0], r["transfer"])
    assert np.abs(r3["transfer"][1] - 2 * r["transfer"]).max() <= 1e-15


def test_the_bookkeeping_of_the_magnification():
    """Set B is set A magnified by m = 0.9, described in its own frame: h_B(x) = h_A(x / m), so beta_B = beta_A / m, k0_B =
    k0_A / m, g_B = g_A / m^2, and over B's frame (area m^2) MA = MB = m^2 M, GA = m^2 G (the kernel leaves A's g alone)
    and GB = m^2 G^T / m^2 = G^T.  The transfer must be what the set gives onto itself."""
    m, k0 = 0.9, 4.0
    M, G, beta = _self_grams(np.random.default_rng(6), 3)
    P = np.diag((beta[:, None] * M + G / beta[:, None]) / (2 * k0))
    same = flux_transfer_from_grams(M, G, M, G.T, beta, k0, beta, k0, P, P)
    # B's own power: (beta_B M_B + G_B / beta_B) / (2 k0_B) with M_B = m^2 M, G_B = m^2 G / m^2 = G
    bB, kB = beta / m, k0 / m
    PB = np.diag((bB[:, None] * (m * m * M) + G / bB[:, None]) / (2 * kB))
    assert np.abs(PB - m * m * P).max() <= 1e-14 * np.abs(P).max()
    r = flux_transfer_from_grams(m * m * M, m * m * G, m * m * M, G.T, beta, k0, bB, kB, P, PB, m)
    assert np.abs(r["transfer"] - same["transfer"]).max() <= 1e-14


def test_cross_power_matrices_orthonormalise_the_sets():
    """With the symmetrised cross-power matrix of a set in place of its power vector the set is Loewdin-orthonormalised
    under it: a set onto itself is the identity whatever its cross powers, a diagonal matrix is the vector formula, and a
    change of basis inside a set leaves the singular values alone."""
    rng = np.random.default_rng(8)
    k, k0 = 4, 4.0
    M, G, beta = _self_grams(rng, k)
    X = (beta[:, None] * M + G / beta[:, None]) / k0                     # X_ab of the set onto itself; X_ba is its transpose
    Psym = (X + X.T) / 4                                                 # cross_sym: P = X / 2
    assert np.abs(Psym - np.diag(np.diag(Psym))).max() > 1e-2 * np.abs(Psym).max()      # far from power-orthogonal
    r = flux_transfer_from_grams(M, G, M, G.T, beta, k0, beta, k0, Psym, Psym)
    assert np.abs(r["transfer"] - np.eye(k)).max() <= 1e-13
    assert abs(r["IL_dB"]) <= 1e-12 and abs(r["MDL_dB"]) <= 1e-12
    vec = flux_transfer_from_grams(M, G, M, G.T, beta, k0, beta, k0, np.diag(Psym), np.diag(Psym))
    assert np.abs(vec["transfer"] - np.eye(k)).max() > 1e-3                # the modes as they are do not give it
    dia = flux_transfer_from_grams(M, G, M, G.T, beta, k0, beta, k0, np.diag(np.diag(Psym)), np.diag(Psym))
    assert np.abs(dia["transfer"] - vec["transfer"]).max() <= 1e-14
    # another set B of three modes: made-up cross sums, its own cross powers
    MA, GA, MB, GB = (rng.standard_normal((2, k, 3)) for _ in range(4))
    bb = rng.uniform(5, 10, 3)
    Q = rng.standard_normal((3, 3))
    Pb = Q @ Q.T + 3 * np.eye(3)
    full = flux_transfer_from_grams(MA, GA, MB, GB, beta, k0, bb, k0, Psym, Pb)
    Xs = (beta[None, :, None] * MA + GA / beta[None, :, None]) / k0 + (bb[None, None, :] * MB + GB / bb[None, None, :]) / k0
    wa, Va = np.linalg.eigh(Psym)
    wb, Vb = np.linalg.eigh(Pb)
    ref = (Vb / np.sqrt(wb)) @ Vb.T @ Xs.transpose(0, 2, 1) @ (Va / np.sqrt(wa)) @ Va.T / 4
    assert full["transfer"].shape == (2, 3, k) and np.abs(full["transfer"] - ref).max() <= 1e-13 * np.abs(ref).max()
    for bad in (np.diag([1.0, 1.0, 1.0, -1.0]), np.zeros((k, k)), Psym + np.triu(np.ones((k, k)), 1), np.full((k, k), np.nan)):
        with pytest.raises(ValueError):
            flux_transfer_from_grams(M, G, M, G.T, beta, k0, beta, k0, bad, Psym)


def test_k0_mismatch_and_the_other_argument_errors():
    M = np.eye(2)
    b, p = np.array([5.0, 6.0]), np.array([1.0, 1.0])
    good = dict(MA=M, GA=M, MB=M, GB=M, beta_a=b, k0_a=4.0, beta_b=b, k0_b=4.0, power_a=p, power_b=p, scale=1.0)
    flux_transfer_from_grams(**good)
    flux_transfer_from_grams(**dict(good, k0_b=4.0 * (1 + 5e-10)))
    flux_transfer_from_grams(**dict(good, k0_b=4.0 / 0.9, scale=0.9))
    bad = [dict(k0_b=4.0 * (1 + 1e-8)), dict(scale=0.9), dict(k0_a=0.0), dict(k0_b=np.nan), dict(scale=0.0), dict(scale=[1.0, 1.0]),
           dict(MA=np.eye(3)), dict(GB=np.full((2, 2), np.nan)), dict(MA="x"), dict(beta_a=[5.0, 0.0]), dict(beta_b=[5.0]),
           dict(power_a=[1.0, np.inf]), dict(power_b=[1.0, 1.0, 1.0]), dict(MA=np.zeros((0, 2)), GA=np.zeros((0, 2)),
                                                                           MB=np.zeros((0, 2)), GB=np.zeros((0, 2)))]
    for kw in bad:
        with pytest.raises(ValueError):
            flux_transfer_from_grams(**dict(good, **kw))


def test_zero_power_guard():
    M = np.array([[1.0, 0.5], [0.5, 2.0]])
    b = np.array([5.0, 6.0])
    r = flux_transfer_from_grams(M, 0 * M, M, 0 * M, b, 4.0, b, 4.0, [0.0, 1.0], [1.0, 1.0])
    assert np.all(np.isfinite(r["transfer"])) and (r["transfer"][:, 0] == 0).all() and (r["transfer"][:, 1] != 0).all()
    r = flux_transfer_from_grams(M, 0 * M, M, 0 * M, b, 4.0, b, 4.0, [1.0, 1.0], [1.0, 0.0])
    assert np.all(np.isfinite(r["transfer"])) and (r["transfer"][1] == 0).all() and np.isinf(r["MDL_dB"])


# -- Python argument errors, no device ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fields(pair):
    fa, fb = ModeFields(pair.mesh_a), ModeFields(pair.mesh_b)
    yield fa, fb
    assert fa._loc is None and fb._loc is None              # nothing below touched the device


def test_python_argument_errors_of_flux_overlap_poses(pair, fields, monkeypatch):
    fa, fb = fields
    monkeypatch.setattr(ModeFields, "_ensure_locator", lambda self: pytest.fail("the device was touched"))
    ga = gb = pair.discs
    rng = np.random.default_rng(7)
    scalar_a = [{"field_vector": rng.standard_normal(fa.N)}]
    mapped = profiled(power_cases.map_profile(), pair.discs)
    P = [IDENTITY]
    bad = {
        "scalar A": (scalar_a, fa, ga, pair.rb, fb, gb, P),
        "scalar B": (pair.ra, fa, ga, [{"field_vector": rng.standard_normal(fb.N)}], fb, gb, P),
        "one record": (pair.ra[0], fa, ga, pair.rb, fb, gb, P),
        "pose shape": (pair.ra, fa, ga, pair.rb, fb, gb, [[0.0, 0.0, 1.0, 0.0]]),
        "no poses": (pair.ra, fa, ga, pair.rb, fb, gb, np.zeros((0, 5))),
        "m = 0": (pair.ra, fa, ga, pair.rb, fb, gb, [(0.0, 0.0, 1.0, 0.0, 0.0)]),
        "nan": (pair.ra, fa, ga, pair.rb, fb, gb, [(np.nan, 0.0, 1.0, 0.0, 1.0)]),
        "no rotation": (pair.ra, fa, ga, pair.rb, fb, gb, [(0.0, 0.0, 1.0, 1e-5, 1.0)]),
        "map A": (pair.ra, fa, mapped, pair.rb, fb, gb, P),
        "map B": (pair.ra, fa, ga, pair.rb, fb, mapped, P),
        "geometry A": (pair.ra, fa, SimpleNamespace(k0=4.0), pair.rb, fb, gb, P),
        "geometry B": (pair.ra, fa, ga, pair.rb, fb, None, P),
        "length A": (pair.rb, fa, ga, pair.rb, fb, gb, P),
        "length B": (pair.ra, fa, ga, pair.ra, fb, gb, P),
        "mesh": (pair.ra, None, ga, pair.rb, fb, gb, P),
        "too many chunk pairs": (pair.ra * 52, fa, ga, pair.rb * 66, fb, gb, P),      # 9 x 9 chunks
    }
    for name, args in bad.items():
        with pytest.raises(ValueError):
            flux_overlap_poses(*args)
            pytest.fail(name)
    # no modes on a side: empty results, still no device
    out = flux_overlap_poses([], fa, ga, pair.rb, fb, gb, [IDENTITY, COVERING])
    assert set(out) == set(NAMES) and all(v.shape == (2, 0, 4) for v in out.values())


def test_python_argument_errors_of_the_splice_functions(pair, fields, monkeypatch):
    fa, fb = fields
    monkeypatch.setattr(ModeFields, "_ensure_locator", lambda self: pytest.fail("the device was touched"))
    g = pair.discs
    k0 = g.k0
    other = SimpleNamespace(positions=g.positions, core_radii=g.core_radii, n_core=g.n_core, n_clad=g.n_clad, k0=1.1 * k0)
    scalar_b = [{"field_vector": np.zeros(fb.N), "beta": 5.0, "n_eff": 1.2}]
    nobeta = [{k: v for k, v in m.items() if k != "beta"} for m in pair.rb]
    good = dict(modes_a=pair.ra, mesh_a=fa, geometry_a=g, modes_b=pair.rb, mesh_b=fb, geometry_b=g, dx=[0.0], dy=[0.0])
    bad = [dict(dx=[]), dict(dy=[np.nan]), dict(angle="x"), dict(scale=0.0), dict(modes_a=[]), dict(modes_b=scalar_b),
           dict(modes_b=nobeta), dict(geometry_b=other), dict(scale=0.9), dict(geometry_a=SimpleNamespace(k0=k0)),
           dict(geometry_a=profiled(power_cases.map_profile(), g)), dict(modes_a=pair.rb)]
    for kw in bad:
        with pytest.raises(ValueError):
            splice_power_map(**dict(good, **kw))
            pytest.fail(str(kw))
    good = dict(modes_list=[pair.rb, pair.rb], mesh=fb, geometry=g, scales=(1.0, 0.9), lengths=(10.0, 10.0), k0=k0)
    bad = [dict(scales=(1.0,)), dict(scales=(1.0, 0.0)), dict(lengths=(1.0, -1.0)), dict(k0=0.0), dict(modes_list=[pair.rb, []]),
           dict(modes_list=[pair.rb, scalar_b]), dict(modes_list=[pair.rb, nobeta]), dict(modes_list=[pair.rb, pair.ra]),
           dict(geometry=profiled(power_cases.map_profile(), g)), dict(geometry=None), dict(modes_list=7)]
    for kw in bad:
        with pytest.raises(ValueError):
            taper_transfer_vectorial(**dict(good, **kw))
            pytest.fail(str(kw))


def test_the_sizer_without_a_locator(built_library):
    from pl_fem_vectoriel_amd import _native
    lib = _native.load_library()
    assert {"plfem_flux_overlap_posed_work_bytes", "plfem_flux_overlap_posed"} <= set(_native.EXPORTS)
    need = ctypes.c_int64(-7)
    assert lib.plfem_flux_overlap_posed_work_bytes(None, 3, 3, 2, ctypes.byref(need)) == _native.PLFEM_EINVAL
    assert need.value == -7
    # the entry point without a locator: the status alone
    assert lib.plfem_flux_overlap_posed(None, None, 1, 1, None, 0, 1.0, 1.0, None, 0, 1.0, 0, None, None, 1, 1, None, 0, 1.0, 1.0,
                                        None, 0, 1.0, 0, 1, None, None, 0, None) == _native.PLFEM_EINVAL


def layout_of_the_header(ka, kb, nposes, ne_b):
    """(batch, bytes) by the layout include/plfem.h documents for plfem_flux_overlap_posed."""
    pairs = ((ka + 31) // 32) * ((kb + 31) // 32)
    slices = max(1, min(128, (6 * ne_b + 31) // 32))
    batch = max(1, min(nposes, 4096, ((512 << 20) - 768) // (8 * (4 * ka * kb + 4096 * pairs * slices + 5))))
    up = lambda n: (n + 255) & ~255
    return batch, up(8 * batch * 4 * ka * kb) + up(8 * batch * 4 * pairs * slices * 1024) + up(8 * batch * 5)


def test_the_layout_formula_stays_under_its_bound():
    for ka, kb, n, ne in ((1, 1, 1, 1), (70, 70, 1681, 32), (256, 256, 100000, 10 ** 6), (2048, 1, 2 ** 31 - 1, 10 ** 6), (3, 3, 2, 32)):
        batch, nbytes = layout_of_the_header(ka, kb, n, ne)
        assert batch >= 1 and 0 < nbytes <= 512 << 20, (ka, kb, n, ne, batch, nbytes)
