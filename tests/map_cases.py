"""The sections of the index-map tests: M3 / M3L, a 41 x 33 map on the three-core mesh of the core tests, and small maps
on the jittered square of tests/core_ties.py whose edges pass exactly through chosen quadrature points."""
from __future__ import annotations

import numpy as np

from core_ties import Ties, jittered_square_mesh
from pl_fem_vectoriel_amd import IndexProfile, ProfiledGeometry

M3_X = np.linspace(-7.0, 9.0, 41)                                   # dx = 0.4
M3_Y = np.linspace(-5.0, 9.0, 33)                                   # dy = 0.4375: nx != ny and dx != dy
M3_BLOBS = ((0.0, 0.0, 1.9, 1.3, 0.4, 0.085), (5.0, 0.0, 1.5, 1.5, 0.0, 0.080), (-2.5, 4.33, 1.2, 1.6, -0.7, 0.090))
SQUARE_BG = 1.2


def m3_index(x, y):
    """n = 1 + 0.45 P + P (b1 + b2 + b3): a super-Gaussian cladding plateau P of radius 6 about (0.8, 1.4) that carries
    three elliptical Gaussian cores, two of them turned.  No circle anywhere."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    P = np.exp(-((((x - 0.8) ** 2 + (y - 1.4) ** 2) / 36.0) ** 4))
    blobs = 0.0
    for cx, cy, a, b, phi, dn in M3_BLOBS:
        u = np.cos(phi) * (x - cx) + np.sin(phi) * (y - cy)
        v = -np.sin(phi) * (x - cx) + np.cos(phi) * (y - cy)
        blobs = blobs + dn * np.exp(-((u / a) ** 2) - (v / b) ** 2)
    return 1.0 + 0.45 * P + P * blobs


def m3_profile() -> IndexProfile:
    X, Y = np.meshgrid(M3_X, M3_Y)
    return IndexProfile(1.0).sampled(M3_X, M3_Y, m3_index(X, Y))


def m3l_profile() -> IndexProfile:
    """M3 with a step core and a trench ring painted over the map."""
    return m3_profile().disc((5.0, 0.0), 1.3, 1.530).ring((0.0, 0.0), 2.5, 3.0, 1.40)


def m3(base, n_clad=1.0) -> ProfiledGeometry:
    return ProfiledGeometry(base, m3_profile(), n_clad=n_clad)


def m3l(base, n_clad=1.0) -> ProfiledGeometry:
    return ProfiledGeometry(base, m3l_profile(), n_clad=n_clad)


def outside_profile(layers=True) -> IndexProfile:
    """A map wholly outside the three-core mesh (domain radius far below 100), over the layers of M3L or none."""
    x, y = np.linspace(100.0, 110.0, 6), np.linspace(-3.0, 4.0, 5)
    prof = IndexProfile(1.0).sampled(x, y, np.full((5, 6), 1.7))
    return prof.disc((5.0, 0.0), 1.3, 1.530).ring((0.0, 0.0), 2.5, 3.0, 1.40) if layers else prof


def layers_only_profile() -> IndexProfile:
    """The layers of M3L over the constant background: what ``outside_profile`` must equal bit for bit."""
    return IndexProfile(1.0).disc((5.0, 0.0), 1.3, 1.530).ring((0.0, 0.0), 2.5, 3.0, 1.40)


class SquareMaps:
    """The jittered unit square (n = 8, 128 elements) with the tie discs of core_ties.Ties painted over small maps:

    ``left``: a 4 x 5 map whose x0 IS the X of the quadrature point ``left_target``: tx = 0, the point is inside;
    ``left_out``: the same with x0 the double just above it: the point is outside, on the background;
    ``far``: dx = 2^-3 and x0 = X_q - 0.375 for the point ``far_target`` with X_q in [0.1875, 0.75]: both differences are
    exact, tx = nx - 1 = 3 exactly, and the point takes the clamped cell i0 = 2 with a = 1;
    ``two``: a 2 x 2 map, one cell.
    The targets lie in no tie disc, so the map decides their permittivity."""

    def __init__(self, n: int = 8):
        self.mesh = jittered_square_mesh(n)
        self.ties = Ties(self.mesh)
        self.base = self.ties.geometry(1.535, SQUARE_BG)
        qx, qy = self.ties.basis.qx
        self.qx, self.qy = qx, qy
        discs = self._paint(IndexProfile(SQUARE_BG)).epsilon(qx, qy) != SQUARE_BG ** 2
        rng = np.random.default_rng(7)
        self.n45 = rng.uniform(1.25, 1.5, (5, 4))                 # (ny, nx) = (5, 4)
        self.left_target = self._target(discs, 0.2, 0.5)
        self.far_target = self._target(discs, 0.1875, 0.75)
        y45 = -0.1 + 0.3 * np.arange(5)                            # covers the square in y
        Xl = float(qx[self.left_target])
        self.left_x0 = {"left": Xl, "left_out": float(np.nextafter(Xl, np.inf))}
        self.far_x0 = float(qx[self.far_target]) - 0.375
        self.profiles = {
            "left": self._paint(IndexProfile(SQUARE_BG).sampled(self.left_x0["left"] + 0.2 * np.arange(4), y45, self.n45)),
            "left_out": self._paint(IndexProfile(SQUARE_BG).sampled(self.left_x0["left_out"] + 0.2 * np.arange(4), y45, self.n45)),
            "far": self._paint(IndexProfile(SQUARE_BG).sampled(self.far_x0 + 0.125 * np.arange(4), y45, self.n45)),
            "two": self._paint(IndexProfile(SQUARE_BG).sampled([0.1, 0.8], [0.2, 0.9], [[1.3, 1.45], [1.5, 1.25]])),
        }

    def _paint(self, prof):
        for i, ((cx, cy), r) in enumerate(zip(self.ties.positions, self.ties.radii)):
            prof.disc((cx, cy), r, 1.535 if i % 2 == 0 else 1.50)
        return prof

    def _target(self, discs, lo, hi):
        """The first quadrature point (element, q) outside every disc with lo < X < hi and 0.3 < Y < 0.7."""
        ok = ~discs & (self.qx > lo) & (self.qx < hi) & (self.qy > 0.3) & (self.qy < 0.7)
        e, q = np.argwhere(ok)[0]
        return int(e), int(q)

    def geometry(self, name) -> ProfiledGeometry:
        return ProfiledGeometry(self.base, self.profiles[name], n_core=1.535, n_clad=SQUARE_BG)
