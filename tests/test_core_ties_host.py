"""Core-boundary ties, host side (no GPU): the tie set of tests/core_ties.py puts quadrature points exactly on a core
circle, or one ulp outside it, under the reference's arithmetic, and the contracted order (fused point, fused squared
distance) decides several of them the other way, checked in exact arithmetic; the oracle's quadrature point and core
test are the separately rounded order the device follows; 65 cores are refused before any device call."""
from fractions import Fraction

import numpy as np
import pytest

from core_ties import Ties, fused_inside, fused_point, jittered_square_mesh, maps, ref_inside, ref_point
from oracle.p2 import MeshTriLite, P2Basis, QUAD_X
from pl_fem_vectoriel_amd import ModeFields, generate_mesh, mode_overlap


@pytest.fixture(scope="module")
def ties():
    return Ties(jittered_square_mesh(8))


def test_oracle_quadrature_point_is_the_separately_rounded_order(c1_geometry):
    for mesh in (jittered_square_mesh(8), generate_mesh(c1_geometry, 0.5, 0)):
        m = MeshTriLite(mesh.p, mesh.t)
        qx, qy = P2Basis(m).qx
        x0, y0, j00, j01, j10, j11 = maps(m)
        for q in range(6):
            xi, eta = QUAD_X[:, q]
            assert np.array_equal(qx[:, q], ref_point(x0, j00, j01, xi, eta))
            assert np.array_equal(qy[:, q], ref_point(y0, j10, j11, xi, eta))


def test_tie_set_sits_on_the_boundary_and_discriminates(ties):
    g = ties.geometry()
    core = ties.core(g)
    qx, qy = ties.basis.qx
    x0, y0, j00, j01, j10, j11 = maps(ties.mesh)
    assert len(ties.radii) == 12
    nflip = {"on": 0, "ulp_out": 0}
    for (e, q), (cx, cy), r, kind, flip in zip(ties.targets, ties.positions, ties.radii, ties.kinds, ties.flips):
        X, Y = float(qx[e, q]), float(qy[e, q])
        dx, dy = X - cx, Y - cy
        d2, r2 = dx * dx + dy * dy, r * r
        if kind == "on":
            assert d2 == r2 and core[e, q]                                # on the circle: inside (closed disc)
        else:
            assert d2 == np.nextafter(r2, np.inf) and not core[e, q]      # one ulp outside
        # the squared distance in exact arithmetic is not on the circle: the decision is a rounding artefact
        exact = (Fraction(X) - Fraction(cx)) ** 2 + (Fraction(Y) - Fraction(cy)) ** 2
        assert exact != Fraction(r) ** 2
        fX = fused_point(x0[e], j00[e], j01[e], *QUAD_X[:, q])
        fY = fused_point(y0[e], j10[e], j11[e], *QUAD_X[:, q])
        assert flip == (fused_inside(fX, fY, cx, cy, r) != ref_inside(X, Y, cx, cy, r))
        nflip[kind] += flip
    # several points of each kind are decided the other way by the contracted order
    assert nflip["on"] >= 3 and nflip["ulp_out"] >= 3, nflip
    assert 0 < sum(ties.flips) < len(ties.flips)


def test_tie_set_leaves_every_other_point_clear(ties):
    g = ties.geometry()
    qx, qy = ties.basis.qx
    core = ties.core(g)
    assert core.sum() > 6 * len(ties.radii)                               # every disc holds points of its own
    for (cx, cy), r, target in zip(ties.positions, ties.radii, ties.targets):
        rel = np.abs((qx - cx) ** 2 + (qy - cy) ** 2 - r * r) / (r * r)
        assert [tuple(int(v) for v in ix) for ix in np.argwhere(rel < 1e-9)] == [target]
    # the reference classification is the union of the discs, each decided as ref_inside decides it
    for (e, q) in ties.targets:
        X, Y = float(qx[e, q]), float(qy[e, q])
        assert core[e, q] == any(ref_inside(X, Y, cx, cy, r) for (cx, cy), r in zip(ties.positions, ties.radii))


def test_sixty_five_cores_are_refused_before_the_device(built_library):
    mesh = jittered_square_mesh(4)
    g = Ties(jittered_square_mesh(8)).geometry()
    g.positions = np.random.default_rng(0).uniform(0, 1, (65, 2))
    g.core_radii = np.full(65, 0.01)
    mf = ModeFields(mesh)
    scal = [{"field_vector": np.ones(mf.N), "beta": 1.0}]
    with pytest.raises(ValueError, match="64 cores"):
        mf.grams(scal, g)
    with pytest.raises(ValueError, match="64 cores"):
        mode_overlap(scal, mf, scal, mf, weight=g)
    assert mf._loc is None                                                # nothing reached the device
