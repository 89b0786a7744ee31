"""Index profiles on the host: IndexProfile.epsilon against a scalar loop over points and layers (overwrite order, closed
rims, points exactly on a rim, the graded formula), the step model written as a profile, the NumPy emulation of the
profile Gram kernel against the oracle's pencils assembled with the profiled geometry, the guards of every two-region
entry, the argument checks that need no device, and the condition of the P5 section: the oracle keeps every record."""
import copy
import ctypes
import math
import pickle

import numpy as np
import pytest

from oracle import hfield, scalar
from oracle.p2 import MeshTriLite, P2Basis
from pl_fem_vectoriel_amd import (IndexProfile, ModeFields, ProfiledGeometry, _native, bend_response, core_decomposition,
                                  mode_dispersion, mode_nonlinearity)
from pl_fem_vectoriel_amd.cmt import CoupledModeTheory
from profile_cases import TIE_RING_N, own_discs, p5, p5_profile, three_core, tie_square
from profile_gram_emulation import NAMES, ProfileGramEmulation
from test_dispersion_host import _rel


@pytest.fixture(scope="module")
def three(built_library):
    g, mesh = three_core()
    return g, mesh, ProfileGramEmulation(mesh.p, mesh.t)


def loop_epsilon(profile, xs, ys):
    """Section 1 of the model, one point and one layer at a time, in Python floats."""
    out = []
    for x, y in zip(xs, ys):
        eps = profile.eps_background
        for cx, cy, r_in, r_out, eps_a, eps_b, g, _ in profile.table().tolist():
            dx, dy = x - cx, y - cy
            d2 = dx * dx + dy * dy
            if r_in * r_in <= d2 <= r_out * r_out:
                if g > 0:
                    t = min(max((math.sqrt(d2) - r_in) / (r_out - r_in), 0.0), 1.0)
                    eps = eps_a + (eps_b - eps_a) * math.pow(t, g)
                else:
                    eps = eps_a
        out.append(eps)
    return np.array(out)


def test_epsilon_matches_the_scalar_loop():
    rng = np.random.default_rng(5)
    # overwrite order: a disc, a ring across it, a smaller disc on top of both, and the same discs the other way round
    a = IndexProfile(1.0).disc((0, 0), 2.0, 1.45).ring((0.5, 0), 1.0, 1.75, 1.40).disc((1.5, 0), 0.5, 1.53)
    b = IndexProfile(1.0).disc((1.5, 0), 0.5, 1.53).ring((0.5, 0), 1.0, 1.75, 1.40).disc((0, 0), 2.0, 1.45)
    pts = rng.uniform(-2.5, 2.5, (2, 4000))
    for prof in (a, b):
        assert np.array_equal(prof.epsilon(pts[0], pts[1]), loop_epsilon(prof, pts[0], pts[1]))
    assert a.epsilon(1.5, 0.0) == 1.53 ** 2 and b.epsilon(1.5, 0.0) == 1.45 ** 2       # the later layer wins
    assert a.epsilon(0.0, 1.9) == 1.45 ** 2 and a.epsilon(3.0, 0.0) == 1.0
    assert (a.n_max, a.n_min, len(a)) == (1.53, 1.0, 3)
    # both rims of a ring are closed: points exactly on them (dyadic, so every product is exact), and one ulp off
    ring = IndexProfile(1.0).ring((0.25, -0.5), 1.5, 2.5, 1.40)
    up, dn = (lambda v: np.nextafter(v, np.inf)), (lambda v: np.nextafter(v, -np.inf))
    xs = np.array([1.75, dn(1.75), 0.25, 0.25, 2.75, up(2.75), -1.25, up(-1.25)])
    ys = np.array([-0.5, -0.5, 2.0, up(2.0), -0.5, -0.5, -0.5, -0.5])
    want = np.where([True, False, True, False, True, False, True, False], 1.40 ** 2, 1.0)
    assert np.array_equal(ring.epsilon(xs, ys), want) and np.array_equal(loop_epsilon(ring, xs, ys), want)


def test_epsilon_on_the_tie_discs_of_the_jittered_square():
    """Quadrature points exactly on a disc's boundary, or one ulp outside it, land where the reference's arithmetic puts
    them: the profile of the tie discs at n_core equals the reference's epsilon on every quadrature point."""
    ties, g, pgt, _ = tie_square()
    qx, qy = ties.basis.qx
    # the section of the GPU tests: a point exactly on the INNER rim of a ring is in the ring, as is one an ulp outside it
    epst = pgt.index_profile.epsilon(qx, qy)
    assert np.array_equal(epst.reshape(-1), loop_epsilon(pgt.index_profile, qx.reshape(-1), qy.reshape(-1)))
    for kind in ("on", "ulp_out"):
        i = ties.kinds.index(kind)
        (e, q), (cx, cy), r = ties.targets[i], ties.positions[i], ties.radii[i]
        d2 = (qx[e, q] - cx) * (qx[e, q] - cx) + (qy[e, q] - cy) * (qy[e, q] - cy)
        assert (d2 == r * r) if kind == "on" else (d2 == np.nextafter(r * r, np.inf))
        assert epst[e, q] == TIE_RING_N ** 2
    prof = own_discs(g).index_profile
    eps = prof.epsilon(qx, qy)
    assert np.array_equal(eps, np.real(g.epsilon(qx, qy)))
    assert np.array_equal(eps.reshape(-1), loop_epsilon(prof, qx.reshape(-1), qy.reshape(-1)))
    for (e, q), kind in zip(ties.targets, ties.kinds):
        assert (eps[e, q] == g.n_core ** 2) == (kind == "on")


@pytest.mark.parametrize("alpha", [1, 2, 8])
def test_graded_formula(alpha):
    n0, n1, a = 1.535, 1.50, 1.5
    prof = IndexProfile(1.0).graded((0.3, -0.2), a, n0, n1, alpha)
    rho = np.concatenate([[0.0], np.random.default_rng(alpha).uniform(0, a, 500)])
    th = np.random.default_rng(alpha + 1).uniform(0, 2 * np.pi, rho.size)
    x, y = 0.3 + rho * np.cos(th), -0.2 + rho * np.sin(th)
    got = prof.epsilon(x, y)
    rr = np.hypot(x - 0.3, y + 0.2)
    inside = got != 1.0
    assert inside.sum() >= 495 and got[0] == n0 ** 2
    # n^2(rho) = n0^2 + (n_edge^2 - n0^2) (rho / a)^alpha.  rho / a carries the 2 ulp of hypot and the rotation, raised to
    # alpha: alpha x 2 ulp of the graded part, which is 0.1 of the value; 1e-14 relative covers alpha = 8
    want = n0 ** 2 + (n1 ** 2 - n0 ** 2) * (rr / a) ** alpha
    assert np.abs(got[inside] - want[inside]).max() <= 1e-14 * n0 ** 2
    # against the scalar loop: the same operations; NumPy's vector pow may differ from libm's by an ulp of t^g
    loop = loop_epsilon(prof, x, y)
    assert np.abs(got - loop).max() <= 2 ** -52 * abs(n1 ** 2 - n0 ** 2)
    assert prof.epsilon(0.3 + a, -0.2) in (n1 ** 2, 1.0)              # the rim: the edge value, or outside by rounding
    assert (prof.n_max, prof.n_min) == (n0, 1.0)


def test_discs_of_a_geometry_equal_its_epsilon_bit_for_bit(three):
    g, mesh, em = three
    qx, qy = em.basis.qx
    pg = own_discs(g)
    assert pg.index_profile.table().shape == (3, 8)
    assert np.array_equal(pg.index_profile.epsilon(qx, qy), np.real(g.epsilon(qx, qy)))
    e = pg.epsilon(qx, qy)
    assert e.dtype == np.complex128 and not e.imag.any() and np.array_equal(e.real, np.real(g.epsilon(qx, qy)))


def test_profiled_geometry_keeps_the_base(three):
    g, _, _ = three
    pg = p5(g)
    assert isinstance(pg, ProfiledGeometry) and isinstance(pg, type(g)) and pg.index_profile.table().shape == (5, 8)
    assert (pg.n_core, pg.n_clad) == (1.540, 1.0) and pg.k0 == g.k0 and pg.domain_radius == g.domain_radius
    assert np.array_equal(pg.positions, g.positions) and np.array_equal(pg.core_radii, g.core_radii)
    assert pg.hash != g.hash and g.n_core == 1.535 and not hasattr(g, "index_profile")
    d = ProfiledGeometry(g, p5_profile())
    assert (d.n_core, d.n_clad) == (1.540, 1.0)
    with pytest.raises(ValueError):
        ProfiledGeometry(g, "no profile")
    with pytest.raises(ValueError, match="no layers"):               # a homogeneous background is no section to solve
        ProfiledGeometry(g, IndexProfile(1.0))


def test_profiled_geometry_copies_pickles_and_rewraps(three):
    g, _, em = three
    pg = p5(g)
    qx, qy = em.basis.qx
    eps = pg.epsilon(qx, qy)
    for q in (copy.copy(pg), copy.deepcopy(pg), pickle.loads(pickle.dumps(pg))):
        assert type(q) is type(pg) and isinstance(q, ProfiledGeometry) and isinstance(q, type(g))
        assert q.hash == pg.hash and (q.n_core, q.n_clad, q.k0, q.domain_radius) == (pg.n_core, pg.n_clad, pg.k0, pg.domain_radius)
        assert np.array_equal(q.index_profile.table(), pg.index_profile.table())
        assert q.index_profile.eps_background == pg.index_profile.eps_background
        assert np.array_equal(q.epsilon(qx, qy), eps) and np.array_equal(q.positions, pg.positions)
    deep = copy.deepcopy(pg)
    assert deep.index_profile is not pg.index_profile and deep.positions is not pg.positions
    assert copy.copy(pg).index_profile is pg.index_profile
    # a second profile on a profiled geometry replaces the first; the first object is left as it was
    other = IndexProfile(1.2).disc((0.0, 0.0), 3.0, 1.46)
    again = ProfiledGeometry(pg, other)
    assert type(again) is type(pg) and again.index_profile is other and pg.index_profile is not other
    assert (again.n_core, again.n_clad) == (1.46, 1.2) and again.hash not in (pg.hash, g.hash)
    assert np.array_equal(again.epsilon(qx, qy).real, other.epsilon(qx, qy)) and np.array_equal(pg.epsilon(qx, qy), eps)
    assert np.array_equal(again.positions, g.positions) and again.domain_radius == g.domain_radius
    assert copy.deepcopy(again).hash == again.hash


def test_emulated_profile_grams_reproduce_the_profiled_pencils(three):
    g, mesh, em = three
    pg = p5(g)
    prof = pg.index_profile
    rng = np.random.default_rng(41)
    k, k0 = 5, g.k0
    vals = rng.standard_normal((2, k, em.interior.size))
    G = em.profile_grams(vals, True, prof)
    assert tuple(G) == NAMES[2]
    V = np.hstack([vals[0], vals[1]]).T
    A, B, basis, *_ = hfield.assemble_hfield_system_fused(pg, em.mesh)
    A, B, _ = hfield.restrict_interior(A, B, basis)
    ea, eb = _rel(G["K_w"] + G["D"] - k0 ** 2 * G["M"], V.T @ (A @ V)), _rel(G["M_w"], V.T @ (B @ V))
    u = rng.standard_normal((1, k, em.N))
    Gs = em.profile_grams(u, False, prof)
    assert tuple(Gs) == NAMES[1]
    S, Mm, Me, _ = scalar.assemble(pg, em.mesh)
    U = u[0].T
    es, em_ = _rel(Gs["S"] - k0 ** 2 * Gs["M_w"], U.T @ ((S - k0 ** 2 * Me) @ U)), _rel(Gs["M"], U.T @ (Mm @ U))
    print(f"vectorial V^T A V {ea:.1e}, V^T B V {eb:.1e}; scalar V^T A V {es:.1e}, V^T B V {em_:.1e}")
    assert ea <= 1e-12 and eb <= 1e-12 and es <= 1e-12 and em_ <= 1e-12
    # the five layers all weigh in: each one owns quadrature points of this mesh
    qx, qy = em.basis.qx
    eps = prof.epsilon(qx, qy)
    assert {1.0, 1.45 ** 2, 1.40 ** 2, 1.530 ** 2, 1.540 ** 2} <= set(np.unique(eps).tolist())
    assert ((eps > 1.50 ** 2) & (eps < 1.535 ** 2)).sum() > 100       # the graded core


def _records(kind, em, k=3):
    rng = np.random.default_rng(2)
    if kind == "vectorial":
        return [{"Ex_dofs": rng.standard_normal(em.interior.size), "Ey_dofs": rng.standard_normal(em.interior.size),
                 "beta": 6.0 + i, "n_eff": 1.48 + 0.01 * i} for i in range(k)]
    return [{"field_vector": rng.standard_normal(em.N), "beta": 6.0 + i, "n_eff": 1.48 + 0.01 * i} for i in range(k)]


def test_two_region_entries_refuse_a_profiled_geometry(three, monkeypatch):
    g, mesh, em = three
    pg = p5(g)
    mf = ModeFields(mesh)
    # nothing may reach the device: the locator is never built
    monkeypatch.setattr(ModeFields, "_ensure_locator", lambda self: pytest.fail("the device was touched"))
    monkeypatch.setattr(_native, "Context", lambda *a, **kw: pytest.fail("the device was touched"))
    for kind in ("vectorial", "scalar"):
        modes = _records(kind, em)
        calls = {"grams": lambda: mf.grams(modes, pg), "core_grams": lambda: mf.core_grams(modes, pg),
                 "moment_grams": lambda: mf.moment_grams(modes, pg), "quartic": lambda: mf.quartic(modes, pg),
                 "mode_dispersion": lambda: mode_dispersion(modes, mf, pg),
                 "core_decomposition": lambda: core_decomposition(modes, mf, pg),
                 "bend_response": lambda: bend_response(modes, mf, pg, radius=4000.0),
                 "mode_nonlinearity": lambda: mode_nonlinearity(modes, mf, pg, n2=(2.6e-20, 2.6e-20))}
        for name, call in calls.items():
            with pytest.raises(ValueError, match="profile_grams"):
                call()
    scal = _records("scalar", em)
    with pytest.raises(ValueError, match="profile_grams"):
        CoupledModeTheory(1.0, "rigorous")._compute_rigorous_coupling(scal, scal, pg, mesh)
    # and the entry for such a geometry refuses one without a profile
    with pytest.raises(ValueError, match="index profile"):
        mf.profile_grams(scal, g)
    assert set(mf.profile_grams([], pg)) == set()


def test_profile_table_validation():
    p = IndexProfile(1.0)
    bad = [lambda: IndexProfile(0.0), lambda: IndexProfile(np.nan), lambda: IndexProfile("x"),
           lambda: p.disc((0, 0), 0.0, 1.5), lambda: p.disc((0, 0), -1.0, 1.5), lambda: p.disc((0, 0), 1.0, 0.0),
           lambda: p.disc((0, 0), 1.0, -1.5), lambda: p.disc((0, np.inf), 1.0, 1.5), lambda: p.disc((0, 0, 0), 1.0, 1.5),
           lambda: p.disc((0, 0), np.nan, 1.5), lambda: p.ring((0, 0), -0.1, 1.0, 1.5), lambda: p.ring((0, 0), 1.0, 1.0, 1.5),
           lambda: p.ring((0, 0), 2.0, 1.0, 1.5), lambda: p.graded((0, 0), 1.0, 1.5, 1.4, 0.0),
           lambda: p.graded((0, 0), 1.0, 1.5, 1.4, -2.0), lambda: p.graded((0, 0), 1.0, 1.5, np.inf, 2.0),
           lambda: p.graded((0, 0), 1.0, 0.0, 1.4, 2.0)]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    assert len(p) == 0 and p.table().shape == (0, 8)
    full = IndexProfile(1.0)
    for i in range(64):
        full.disc((i, 0), 0.4, 1.5)
    with pytest.raises(ValueError, match="64"):
        full.disc((0, 0), 0.4, 1.5)
    assert full.table().shape == (64, 8)
    t = p5_profile().table()
    assert t.dtype == np.float64 and t.flags.c_contiguous and (t[:, 7] == 0).all()
    assert t[2].tolist() == [0.0, 0.0, 0.0, 1.5, 1.535 ** 2, 1.50 ** 2, 2.0, 0.0] and t[1][2:4].tolist() == [1.3, 2.2]


def test_profile_entries_refuse_bad_arguments_on_the_host(built_library):
    lib = _native.load_library()
    b = ctypes.c_int64(-1)
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)                                       # never dereferenced: the handle is checked first
    assert lib.plfem_profile_gram_work_bytes(2, 22, None) == _native.PLFEM_EINVAL
    for ncomp, k in ((0, 5), (3, 5), (2, 0), (1, -1)):
        assert lib.plfem_profile_gram_work_bytes(ncomp, k, ctypes.byref(b)) == _native.PLFEM_EINVAL
        assert lib.plfem_profile_grams(null, ncomp, k, one, 0, one, 3, 1.0, one, 1 << 30, one) == _native.PLFEM_EINVAL
    assert b.value == -1
    assert lib.plfem_profile_grams(null, 2, 5, None, 1, None, 3, 1.0, None, 0, None) == _native.PLFEM_EINVAL
    t = p5_profile().table()
    assert lib.plfem_set_index_profile(null, t.ctypes.data_as(ctypes.c_void_p), 5, 1.0) == _native.PLFEM_EINVAL
    # the bound of the header: nout k^2 doubles, then nout ceil(k / 32)^2 x 768 blocks of 8 KiB
    for ncomp, nout in ((1, 3), (2, 4)):
        for k in (1, 22, 32, 33, 70):
            assert lib.plfem_profile_gram_work_bytes(ncomp, k, ctypes.byref(b)) == _native.PLFEM_OK
            nc = (k + 31) // 32
            assert b.value == (nout * k * k * 8 + 255) // 256 * 256 + nout * nc * nc * 768 * 8192


def test_solver_arguments():
    from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver
    g, _ = three_core()
    for cls in (TrueVectorialMaxwellSolver, ScalarHelmholtzSolver):
        assert cls(g).n_eff_shift is None and cls(g, n_eff_shift=1.49).n_eff_shift == 1.49
        for bad in (0.0, -1.0, np.nan, "x"):
            with pytest.raises(ValueError):
                cls(g, n_eff_shift=bad)


def test_the_oracle_keeps_every_record_of_p5(three):
    """The condition of the GPU parity tests on this section: the reference's own n_eff and field filters drop nothing,
    so a comparison record by record leaves out no mode."""
    g, mesh, em = three
    pg = p5(g)
    om = MeshTriLite(mesh.p, mesh.t)
    sc = scalar.solve(pg, om, 10)
    assert len(sc) == 18
    assert [round(m["n_eff"], 5) for m in sc[:3]] == [1.49592, 1.49560, 1.49050]
    vec = hfield.solve_vectorial_modes(pg, om, n_modes_target=10, fused=True)
    assert len(vec) == 22
