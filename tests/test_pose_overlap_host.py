"""Host side of the posed overlaps: the NumPy emulation of k_field_overlap_posed (tests/pose_overlap_emulation.py) against
the emulation of the merged kernel on a mesh moved by the pose on the host and against a closed form; the k x k host
math of the splice and taper functions; and every argument error, raised with no device present."""
import numpy as np
import pytest

from fields_emulation import Emulation, overlap as em_overlap
from pose_overlap_emulation import (COVERING, HALF_OUT, IDENTITY, closed_form, moved_mesh, moved_records, posed_overlap,
                                    quadratic_records, records, small_meshes, vals)
from pl_fem_vectoriel_amd import (MCFGeometry, mode_overlap_poses, pose_table, splice_map, splice_quantities_from_overlaps,
                                  taper_from_interfaces, taper_transfer)

QUARTER = (0.05, 0.1, 0.0, 1.0, 0.9)


@pytest.fixture(scope="module")
def pair():
    mesh_a, mesh_b = small_meshes()
    em_a, em_b = Emulation(mesh_a.p, mesh_a.t), Emulation(mesh_b.p, mesh_b.t)
    assert em_a.quadrature()[0].shape[1] == 300 and em_b.quadrature()[0].shape[1] == 192
    rng = np.random.default_rng(21)
    recs = {kind: (records(rng, kind, em_a.interior.size if kind == "vectorial" else em_a.N, 5),
                   records(rng, kind, em_b.interior.size if kind == "vectorial" else em_b.N, 4))
            for kind in ("vectorial", "scalar")}
    return mesh_a, mesh_b, em_a, em_b, recs


@pytest.mark.parametrize("kind", ["vectorial", "scalar"])
def test_emulation_matches_the_overlap_on_a_host_moved_mesh(pair, kind):
    mesh_a, mesh_b, em_a, em_b, recs = pair
    ra, rb = recs[kind]
    indexed = kind == "vectorial"
    for pose in (IDENTITY, COVERING, HALF_OUT, QUARTER):
        O, elem = posed_overlap(em_a, vals(ra), em_b, vals(rb), indexed, pose)
        moved = moved_mesh(mesh_a, pose)
        ref = em_overlap(Emulation(moved.p, moved.t), vals(moved_records(ra, pose)), em_b, vals(rb), indexed)
        err = np.abs(O - ref).max() / np.abs(ref).max()
        print(kind, pose, f"{err:.2e}", f"outside {np.mean(elem < 0):.2f}")
        assert err <= 1e-12, (kind, pose, err)
    out = np.mean(posed_overlap(em_a, vals(ra), em_b, vals(rb), indexed, HALF_OUT)[1] < 0)
    assert 0.25 <= out <= 0.75, out


@pytest.mark.parametrize("kind", ["vectorial", "scalar"])
def test_identity_pose_is_bit_equal_to_the_overlap(pair, kind):
    _, _, em_a, em_b, recs = pair
    ra, rb = recs[kind]
    O, _ = posed_overlap(em_a, vals(ra), em_b, vals(rb), kind == "vectorial", IDENTITY)
    assert np.array_equal(O, em_overlap(em_a, vals(ra), em_b, vals(rb), kind == "vectorial"))


def test_closed_form_of_quadratics_under_the_covering_pose(pair):
    _, _, em_a, em_b, _ = pair
    rng = np.random.default_rng(22)
    Ca, Cb = rng.standard_normal((5, 6)), rng.standard_normal((4, 6))
    O, elem = posed_overlap(em_a, vals(quadratic_records(em_a, Ca)), em_b, vals(quadratic_records(em_b, Cb)), False, COVERING)
    assert (elem >= 0).all()
    ref = closed_form(Ca, Cb, COVERING)
    err = np.abs(O - ref).max() / np.abs(ref).max()
    print(f"closed form {err:.2e}")
    assert err <= 1e-12, err


# -- splice_quantities_from_overlaps ----------------------------------------------------------------------------------
def test_splice_quantities():
    rng = np.random.default_rng(23)
    Q = np.linalg.qr(rng.standard_normal((4, 4)))[0]
    r = splice_quantities_from_overlaps(Q, np.eye(4), np.eye(4), 1.0)
    assert abs(r["IL_dB"]) <= 1e-12 and abs(r["MDL_dB"]) <= 1e-12
    assert np.abs(r["transfer"] - Q.T).max() <= 1e-14 and r["transfer"].shape == (4, 4)
    # a diagonal O with known entries, rectangular: ka = 3, kb = 2
    O = np.zeros((3, 2))
    O[0, 0], O[1, 1] = 0.8, 0.4
    r = splice_quantities_from_overlaps(O, np.eye(3), np.eye(2), 1.0)
    assert r["transfer"].shape == (2, 3) and r["power"].shape == (2, 3)
    assert np.allclose(r["singular_values"], [0.8, 0.4], rtol=0, atol=1e-15)
    assert abs(r["IL_dB"] + 10 * np.log10((0.64 + 0.16) / 2)) <= 1e-12
    assert abs(r["MDL_dB"] - 10 * np.log10(4.0)) <= 1e-12
    assert np.allclose(r["power"], (O * O).T, rtol=0, atol=1e-15)
    # the scale: the posed A has the self-overlap m^2 Gaa, so O = m Q is a perfect splice at magnification m
    r = splice_quantities_from_overlaps(np.stack([1.25 * Q, 0.5 * Q]), np.eye(4), np.eye(4), [1.25, 0.5])
    assert r["transfer"].shape == (2, 4, 4) and np.abs(r["IL_dB"]).max() <= 1e-12 and np.abs(r["MDL_dB"]).max() <= 1e-12
    # Loewdin: non-orthonormal sets A = X Sa, B = X Sb of one orthonormal X give a unitary transfer
    Sa, Sb = rng.standard_normal((4, 4)), rng.standard_normal((4, 4))
    r = splice_quantities_from_overlaps(Sa.T @ Sb, Sa.T @ Sa, Sb.T @ Sb)
    assert np.abs(r["transfer"] @ r["transfer"].T - np.eye(4)).max() <= 1e-10
    # a dark splice
    r = splice_quantities_from_overlaps(np.zeros((1, 3, 2)), np.eye(3), np.eye(2))
    assert np.isinf(r["IL_dB"][0]) and np.isinf(r["MDL_dB"][0]) and (r["transfer"] == 0).all()
    for bad in ((np.zeros(3), np.eye(3), np.eye(3), 1.0), (Q, np.eye(3), np.eye(4), 1.0), (Q, np.eye(4), -np.eye(4), 1.0),
                (Q, np.eye(4), np.eye(4), 0.0), (Q, np.eye(4), np.eye(4), [1.0, 2.0]), (Q * np.nan, np.eye(4), np.eye(4), 1.0)):
        with pytest.raises(ValueError):
            splice_quantities_from_overlaps(*bad)


# -- taper_from_interfaces --------------------------------------------------------------------------------------------
def test_taper_from_interfaces():
    rng = np.random.default_rng(24)
    b = [rng.uniform(5, 6, 3), rng.uniform(5, 6, 2), rng.uniform(5, 6, 4)]
    L = np.array([10.0, 20.0, 5.0])
    T0, T1 = rng.standard_normal((2, 3)), rng.standard_normal((4, 2))          # rectangular, and no product commutes
    r = taper_from_interfaces([T0, T1], b, L)
    P = [np.diag(np.exp(-1j * bi * li)) for bi, li in zip(b, L)]
    ref = P[2] @ T1 @ P[1] @ T0 @ P[0]
    assert r["transfer"].shape == (4, 3) and np.abs(r["transfer"] - ref).max() <= 1e-13
    assert np.abs(r["power"] - np.abs(ref) ** 2).max() <= 1e-13
    assert np.abs(r["transmitted"] - (np.abs(ref) ** 2).sum(0)).max() <= 1e-13
    # one section: the diagonal of phases
    r = taper_from_interfaces([], [b[0]], [7.0])
    assert np.abs(r["transfer"] - np.diag(np.exp(-7j * b[0]))).max() <= 1e-15
    assert abs(r["IL_dB"]) <= 1e-12 and abs(r["MDL_dB"]) <= 1e-12
    # unitary interfaces give a unitary total
    U = [np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in range(2)]
    r = taper_from_interfaces(U, [b[0]] * 3, L)
    tot = r["transfer"]
    assert np.abs(tot.conj().T @ tot - np.eye(3)).max() <= 1e-13
    assert np.abs(r["transmitted"] - 1).max() <= 1e-13 and abs(r["IL_dB"]) <= 1e-12 and abs(r["MDL_dB"]) <= 1e-11
    # known loss
    r = taper_from_interfaces([np.diag([0.8, 0.4])], [b[1], b[1]], [1.0, 1.0])
    assert abs(r["IL_dB"] + 10 * np.log10(0.4)) <= 1e-12 and abs(r["MDL_dB"] - 10 * np.log10(4.0)) <= 1e-12
    for bad in (([T0], b, L), ([T1, T0], b, L), ([T0, T1], b, L[:2]), ([T0, T1], b, -L), ([], [], []),
                ([T0 * np.nan, T1], b, L), ([T0, T1], [b[0], b[1], b[2] * np.inf], L)):
        with pytest.raises(ValueError):
            taper_from_interfaces(*bad)


# -- argument errors, with no device present --------------------------------------------------------------------------
def test_pose_table():
    t = pose_table()
    assert t.shape == (1, 5) and np.array_equal(t[0], IDENTITY)
    t = pose_table(np.arange(3.0)[None, :], np.arange(2.0)[:, None], 0.3, 1.2)
    assert t.shape == (6, 5) and np.array_equal(t[4], (1.0, 1.0, np.cos(0.3), np.sin(0.3), 1.2))
    for bad in (dict(dx=np.nan), dict(dy=np.inf), dict(angle=np.nan), dict(scale=0.0), dict(scale=-1.0), dict(dx="abc"),
                dict(dx=np.zeros(2), dy=np.zeros(3)), dict(scale=np.array([]))):
        with pytest.raises(ValueError):
            pose_table(**bad)


def test_argument_errors_before_any_device_call(pair):
    mesh_a, mesh_b, em_a, em_b, recs = pair
    va, vb = recs["vectorial"]
    sa, sb = recs["scalar"]
    good = pose_table(0.1, 0.0, 0.2, 1.1)
    g = MCFGeometry(7, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55)
    for poses in (np.zeros((0, 5)), np.zeros(5), np.zeros((2, 4)), [[0, 0, 1, 0, 0]], [[0, 0, 1, 0, -1]], [[0, 0, 1, 1e-5, 1]],
                  [[np.nan, 0, 1, 0, 1]], [[0, np.inf, 1, 0, 1]], [[0, 0, 2, 0, 1]], "abc", None):
        with pytest.raises(ValueError):
            mode_overlap_poses(va, mesh_a, vb, mesh_b, poses)
    for a, b in ((va, sb), (sa, vb), ([{"Ex_dofs": np.ones(3), "Ey_dofs": np.ones(3)}], vb), (sa, [{"field_vector": np.ones(7)}]),
                 (sa[0], sb), ([{"x": 1}], sb)):
        with pytest.raises(ValueError):
            mode_overlap_poses(a, mesh_a, b, mesh_b, good)
        with pytest.raises(ValueError):
            splice_map(a, mesh_a, b, mesh_b, [0.0], [0.0])
    with pytest.raises(ValueError):
        mode_overlap_poses(sa, None, sb, mesh_b, good)
    with pytest.raises(ValueError, match="weight=None"):
        mode_overlap_poses(sa, mesh_a, sb, mesh_b, good, weight=g, normalize=True)
    with pytest.raises(ValueError):
        mode_overlap_poses(sa, mesh_a, sb, mesh_b, good, weight=object())
    many = [sa[0]] * 520                                               # 17 x 17 chunk pairs
    with pytest.raises(ValueError, match="chunk"):
        mode_overlap_poses(many, mesh_a, many, mesh_a, good)
    assert mode_overlap_poses([], mesh_a, sb, mesh_b, good).shape == (1, 0, 4)

    for kw in (dict(dx=[np.nan], dy=[0.0]), dict(dx=[], dy=[0.0]), dict(dx=np.zeros((2, 2)), dy=[0.0]), dict(dx=[0.0], dy="abc"),
               dict(dx=[0.0], dy=[0.0], angle=np.nan), dict(dx=[0.0], dy=[0.0], angle=[0.0, 0.1]),
               dict(dx=[0.0], dy=[0.0], scale=0.0), dict(dx=[0.0], dy=[0.0], scale=np.inf)):
        with pytest.raises(ValueError):
            splice_map(sa, mesh_a, sb, mesh_b, **kw)
    with pytest.raises(ValueError):
        splice_map([], mesh_a, sb, mesh_b, [0.0], [0.0])

    def section(n, k=2, n_eff=1.5):
        return [{"field_vector": np.ones(n), "n_eff": n_eff} for _ in range(k)]

    N = em_b.N
    ok = [section(N), section(N, 3)]
    vec = [{"Ex_dofs": np.ones(em_b.interior.size), "Ey_dofs": np.ones(em_b.interior.size), "n_eff": 1.5}]
    for args in ((ok, mesh_b, (1.0,), (1.0, 1.0), 4.0), (ok, mesh_b, (1.0, 0.9), (1.0,), 4.0), (ok, mesh_b, (1.0, 0.0), (1.0, 1.0), 4.0),
                 (ok, mesh_b, (1.0, -0.9), (1.0, 1.0), 4.0), (ok, mesh_b, (1.0, 0.9), (1.0, -1.0), 4.0),
                 (ok, mesh_b, (1.0, np.nan), (1.0, 1.0), 4.0), (ok, mesh_b, (1.0, 0.9), (1.0, 1.0), 0.0),
                 (ok, mesh_b, (1.0, 0.9), (1.0, 1.0), np.nan), (ok, mesh_b, (1.0, 0.9), (1.0, 1.0), "k"),
                 ([], mesh_b, (), (), 4.0), ([ok[0], []], mesh_b, (1.0, 0.9), (1.0, 1.0), 4.0),
                 ([ok[0], section(N + 1)], mesh_b, (1.0, 0.9), (1.0, 1.0), 4.0),
                 ([ok[0], section(N, n_eff=np.nan)], mesh_b, (1.0, 0.9), (1.0, 1.0), 4.0),
                 ([ok[0], [{"field_vector": np.ones(N)}]], mesh_b, (1.0, 0.9), (1.0, 1.0), 4.0),
                 (ok, None, (1.0, 0.9), (1.0, 1.0), 4.0)):
        with pytest.raises(ValueError):
            taper_transfer(*args)
    with pytest.raises(ValueError, match="scalar"):
        taper_transfer([vec, vec], mesh_b, (1.0, 0.9), (1.0, 1.0), 4.0)
