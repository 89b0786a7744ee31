"""Core-boundary ties for the tests: discs built so that chosen quadrature points of a mesh lie exactly on a disc's
boundary, or one ulp outside it, under the reference's arithmetic.

The reference puts a point in a core when ``(x - cx)**2 + (y - cy)**2 <= r**2`` (``MCFGeometry.epsilon``), every
operation rounded on its own, at the quadrature point ``p0 + J xi`` of ``oracle.p2.P2Basis.qx`` (the two products rounded,
then summed, then added to the vertex).  A device that forms the point with fused multiply-adds, or the squared distance
with one, can decide such a point the other way.  Exact arithmetic (``fractions.Fraction``; ``float(Fraction)`` rounds to
nearest, ties to even) emulates both orders here, so that a test can check on the host that the set discriminates.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from oracle.p2 import P2Basis, MeshTriLite, QUAD_X


def fma(a: float, b: float, c: float) -> float:
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def ref_point(x0, j0, j1, xi, eta) -> float:
    """x0 + (fl(j0 xi) + fl(j1 eta)): the order of P2Basis.qx."""
    return x0 + (j0 * xi + j1 * eta)


def fused_point(x0, j0, j1, xi, eta) -> float:
    """fma(j1, eta, fma(j0, xi, x0)): the contracted order."""
    return fma(j1, eta, fma(j0, xi, x0))


def ref_inside(X, Y, cx, cy, r) -> bool:
    dx, dy = X - cx, Y - cy
    return dx * dx + dy * dy <= r * r


def fused_inside(X, Y, cx, cy, r) -> bool:
    dx, dy = X - cx, Y - cy
    return fma(dx, dx, dy * dy) <= r * r


def jittered_square_mesh(n: int, jitter: float = 0.25, seed: int = 0):
    """unit_square_mesh(n) with its interior vertices moved by up to ``jitter`` of the grid step (seeded): a
    triangulation of the unit square whose coordinates and Jacobians are not dyadic, so products round."""
    from pl_fem_vectoriel_amd.mesh import TriMesh, unit_square_mesh
    sq = unit_square_mesh(n)
    p = sq.p.copy()
    inner = (p[0] > 0) & (p[0] < 1) & (p[1] > 0) & (p[1] < 1)
    p[:, inner] += np.random.default_rng(seed).uniform(-jitter, jitter, (2, int(inner.sum()))) / n
    return TriMesh(p, sq.t.copy())


def maps(mesh: MeshTriLite):
    """Per element: x0, y0, j00, j01, j10, j11 (J = [p1 - p0, p2 - p0]), as P2Basis forms them."""
    p, t = mesh.p, mesh.t
    p0, p1, p2 = p[:, t[0]], p[:, t[1]], p[:, t[2]]
    return p0[0], p0[1], p1[0] - p0[0], p2[0] - p0[0], p1[1] - p0[1], p2[1] - p0[1]


class Ties:
    """Discs on ``mesh`` (positions (n, 2), radii (n,)) and, per disc, its target quadrature point (element, q) and kind:
    ``"on"`` (the reference's squared distance equals fl(r^2): inside) or ``"ulp_out"`` (it is the double just above
    fl(r^2): outside).  ``flips[i]``: the fused order (fused point and fused squared distance) decides the target of disc
    i the other way.  Every other quadrature point of the mesh is at least ``margin`` (relative) away from every
    boundary, so any reasonable arithmetic decides it as the reference does."""

    def __init__(self, mesh, n_discs: int = 12, seed: int = 0, margin: float = 1e-9):
        self.mesh = MeshTriLite(mesh.p, mesh.t)
        self.basis = P2Basis(self.mesh)
        qx, qy = self.basis.qx                                     # (ne, 6)
        x0, y0, j00, j01, j10, j11 = maps(self.mesh)
        ne = qx.shape[0]
        h = np.sqrt(np.median(self.basis.absdet))                 # element size
        rng = np.random.default_rng(seed)
        self.positions, self.radii, self.targets, self.kinds, self.flips = [], [], [], [], []
        want = {("on", True): n_discs // 3, ("ulp_out", True): n_discs // 3,
                ("on", False): n_discs // 6, ("ulp_out", False): n_discs - 2 * (n_discs // 3) - n_discs // 6}
        for e in rng.permutation(ne):
            if sum(want.values()) == 0:
                break
            q = int(rng.integers(6))
            X, Y = float(qx[e, q]), float(qy[e, q])
            fX = fused_point(x0[e], j00[e], j01[e], *QUAD_X[:, q])
            fY = fused_point(y0[e], j10[e], j11[e], *QUAD_X[:, q])
            for _ in range(24):
                th, d = rng.uniform(0, 2 * np.pi), h * rng.uniform(0.3, 0.6)
                cx, cy = X - d * np.cos(th), Y - d * np.sin(th)
                if any(np.hypot(cx - a, cy - b) < d + rb + h / 2 for (a, b), rb in zip(self.positions, self.radii)):
                    continue
                dx, dy = X - cx, Y - cy
                d2 = dx * dx + dy * dy
                found = None
                r0 = float(np.sqrt(d2))
                for s in range(-6, 7):
                    r = float(np.nextafter(r0, np.inf if s > 0 else -np.inf)) if s else r0
                    for _s in range(abs(s) - 1):
                        r = float(np.nextafter(r, np.inf if s > 0 else -np.inf))
                    r2 = r * r
                    kind = "on" if r2 == d2 else ("ulp_out" if np.nextafter(r2, np.inf) == d2 else None)
                    if kind is None:
                        continue
                    flip = fused_inside(fX, fY, cx, cy, r) != ref_inside(X, Y, cx, cy, r)
                    if want.get((kind, flip), 0) > 0:
                        found = (r, kind, flip)
                        break
                if found is None:
                    continue
                r, kind, flip = found
                # every other quadrature point well clear of this boundary
                rel = np.abs((qx - cx) ** 2 + (qy - cy) ** 2 - r * r) / (r * r)
                rel[e, q] = np.inf
                if rel.min() < margin:
                    continue
                want[(kind, flip)] -= 1
                self.positions.append((cx, cy))
                self.radii.append(r)
                self.targets.append((int(e), q))
                self.kinds.append(kind)
                self.flips.append(bool(flip))
                break
        if sum(want.values()):
            raise RuntimeError(f"could not build the tie set on this mesh: missing {want}")
        self.positions = np.array(self.positions)
        self.radii = np.array(self.radii)

    def geometry(self, n_core=1.535, n_clad=1.0):
        """A geometry of the package with these discs as its cores (no PML: the eigenmode path reads real eps only)."""
        from pl_fem_vectoriel_amd import MCFGeometry
        g = MCFGeometry(7, 8.0, 1.5, n_core, n_clad, wavelength_um=1.55, use_complex_pml=False)
        g.positions = g.core_positions = self.positions.copy()
        g.core_radii = self.radii.copy()
        g.n_cores = len(self.radii)
        return g

    def core(self, geometry):
        """(ne, 6) the reference's region of every quadrature point (MCFGeometry.epsilon)."""
        qx, qy = self.basis.qx
        return np.real(geometry.epsilon(qx, qy)) == geometry.n_core ** 2
