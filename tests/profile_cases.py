"""The sections of the index-profile tests: P5 on the three-core mesh of the core tests, and tie discs plus a ring on the
jittered square of tests/core_ties.py."""
from __future__ import annotations

import numpy as np

from core_ties import Ties, jittered_square_mesh
from pl_fem_vectoriel_amd import IndexProfile, PhotonicLanternGeometry, ProfiledGeometry, generate_mesh

POS = np.array([[0.0, 0.0], [5.0, 0.0], [-2.5, 4.33]])               # the three unequal cores of tests/test_cores_host.py
RAD = np.array([1.5, 1.3, 1.1])
TIE_RING_N = 1.47


def three_core():
    """(geometry, mesh): n = 1.535 / 1.0 at 1.55 um on generate_mesh(g, 0.5, 0), 4055 elements."""
    g = PhotonicLanternGeometry(3, "triangular_3", POS, RAD, 1.535, 1.0, wavelength=1.55)
    mesh = generate_mesh(g, 0.5, 0)
    assert mesh.t.shape[1] == 4055
    return g, mesh


def p5_profile() -> IndexProfile:
    """A cladding disc in air, a trench ring round the second core, a graded first core, two step cores of unequal index."""
    return (IndexProfile(1.0).disc((0.8, 1.4), 9.0, 1.45).ring((5.0, 0.0), 1.3, 2.2, 1.40)
            .graded((0.0, 0.0), 1.5, 1.535, 1.50, 2).disc((5.0, 0.0), 1.3, 1.530).disc((-2.5, 4.33), 1.1, 1.540))


def p5(base) -> ProfiledGeometry:
    return ProfiledGeometry(base, p5_profile(), n_core=1.540)


def own_discs(g) -> ProfiledGeometry:
    """The geometry's own discs at n_core over a background n_clad: the step model written as a profile."""
    prof = IndexProfile(g.n_clad)
    for (cx, cy), r in zip(np.atleast_2d(g.positions), np.asarray(g.core_radii).reshape(-1)):
        prof.disc((cx, cy), r, g.n_core)
    return ProfiledGeometry(g, prof, n_core=g.n_core, n_clad=g.n_clad)


def tie_square(n: int = 8):
    """(ties, base geometry, profiled geometry, mesh) on the jittered unit square: a ring whose two rims cross elements,
    the tie discs of core_ties.Ties at alternating indices, and, painted last, a ring round the first "on" tie disc and
    one round the first "ulp_out" one whose INNER radius is the disc's: the target point of the first lies exactly on
    the inner rim (in the ring: the rim is closed), that of the second one ulp outside it (in the ring either way), over
    a background of 1.2.  TIE_RING_N is the index of those rings."""
    mesh = jittered_square_mesh(n)
    ties = Ties(mesh)
    g = ties.geometry()
    prof = IndexProfile(1.2).ring((0.5, 0.5), 0.22, 0.37, 1.40)
    for i, ((cx, cy), r) in enumerate(zip(ties.positions, ties.radii)):
        prof.disc((cx, cy), r, 1.535 if i % 2 == 0 else 1.50)
    for kind in ("on", "ulp_out"):
        i = ties.kinds.index(kind)
        prof.ring(ties.positions[i], ties.radii[i], 1.5 * ties.radii[i], TIE_RING_N)
    return ties, g, ProfiledGeometry(g, prof, n_core=1.535, n_clad=1.2), mesh
