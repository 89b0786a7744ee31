"""NumPy emulation of the sampled projection (k_mode_project_sampled + k_project_sampled_reduce) for the tests.

On top of ``ProjectionEmulation``: the mode values at the 16-point rule (``values16``), the weights ``|det J| w_q``
(``weights16``) and the physical points (``points16``) are its own.  Frame f is a complex image on the node grid
``x_i = x0 + i dx``, ``y_j = y0 + j dy`` with ``x0 = x[0]``, ``dx = (x[-1] - x[0]) / (nx - 1)`` (what
``ModeFields.project_sampled`` passes to the library), and its bilinear interpolant is formed in the order of
``include/plfem.h``: ``tx = (X - x0) * (1 / dx)``, a point with ``tx < 0``, ``tx > nx - 1``, ``ty < 0`` or ``ty > ny - 1``
contributes 0, otherwise ``i0 = min(floor(tx), nx - 2)``, ``a = tx - i0`` and
``F = ((1 - a) F[j0][i0] + a F[j0][i0+1]) (1 - b) + ((1 - a) F[j0+1][i0] + a F[j0+1][i0+1]) b``.

``tolerance`` is ``1.2e-16 (Q + 64) S_m Fmax_f``: the bound of ``projection_emulation.py`` without the phase term.  The
interpolation weights are non-negative and sum to 1, so ``|F(x)| <= Fmax_f`` (the largest |re| or |im| pixel of the
frame) for re and im each, and the interpolation adds a few ulps per term to the few of the products; the sum of Q
terms in a fixed order takes the rest.
"""
from __future__ import annotations

import numpy as np

from projection_emulation import ProjectionEmulation


def grid_of(x, y):
    """(x0, y0, 1 / dx, 1 / dy, nx, ny) of the pixel axes, as the library receives them."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    dx = float(x[-1] - x[0]) / (x.size - 1)
    dy = float(y[-1] - y[0]) / (y.size - 1)
    return float(x[0]), float(y[0]), 1.0 / dx, 1.0 / dy, x.size, y.size


class SampledProjectionEmulation(ProjectionEmulation):
    def grid_coordinates(self, x, y):
        """(tx, ty), each (ne, 16): the quadrature points in pixel units."""
        x0, y0, inv_dx, inv_dy, _, _ = grid_of(x, y)
        X, Y = self.points16()
        return (X - x0) * inv_dx, (Y - y0) * inv_dy

    def edge_distance(self, x, y):
        """The smallest distance, in units of tx / ty, of any quadrature point to one of the four lines of the outer
        edge: a point nearer than the rounding of tx could be counted in by one side and out by the other."""
        tx, ty = self.grid_coordinates(x, y)
        nx, ny = np.size(x), np.size(y)
        return float(min(np.abs(tx).min(), np.abs(tx - (nx - 1)).min(), np.abs(ty).min(), np.abs(ty - (ny - 1)).min()))

    def inside(self, x, y):
        """(ne, 16) bool: the quadrature points within the closed extent."""
        tx, ty = self.grid_coordinates(x, y)
        return (tx >= 0) & (tx <= np.size(x) - 1) & (ty >= 0) & (ty <= np.size(y) - 1)

    def interpolate(self, frames, x, y):
        """F (Q, nf) complex: the bilinear interpolant of every frame (nf, ny, nx) at every quadrature point, 0 outside."""
        frames = np.asarray(frames, dtype=np.complex128)
        nx, ny = np.size(x), np.size(y)
        tx, ty = (t.reshape(-1) for t in self.grid_coordinates(x, y))
        ok = self.inside(x, y).reshape(-1)
        i0 = np.minimum(np.floor(np.where(ok, tx, 0.0)).astype(np.int64), nx - 2)
        j0 = np.minimum(np.floor(np.where(ok, ty, 0.0)).astype(np.int64), ny - 2)
        a = (tx - i0)[:, None]
        b = (ty - j0)[:, None]
        Ft = np.moveaxis(frames, 0, -1)                               # (ny, nx, nf)

        def part(P):
            lo = (1.0 - a) * P[j0, i0] + a * P[j0, i0 + 1]
            hi = (1.0 - a) * P[j0 + 1, i0] + a * P[j0 + 1, i0 + 1]
            return lo * (1.0 - b) + hi * b

        F = part(Ft.real) + 1j * part(Ft.imag)
        F[~ok] = 0.0
        return F

    def project_sampled(self, vals, indexed, frames, x, y):
        """P complex (ncomp, k, nf), the output of plfem_mode_project_sampled."""
        ncomp, k = vals.shape[:2]
        U = self.values16(vals, indexed).reshape(ncomp * k, -1)      # (fields, points)
        B = self.weights16().reshape(-1)[:, None] * self.interpolate(frames, x, y)
        return (U @ B.real + 1j * (U @ B.imag)).reshape(ncomp, k, -1)

    def tolerance(self, vals, indexed, frames):
        """tol (ncomp, k, nf) of the module docstring."""
        frames = np.asarray(frames, dtype=np.complex128)
        fmax = np.maximum(np.abs(frames.real), np.abs(frames.imag)).reshape(frames.shape[0], -1).max(axis=1)
        Q = self.weights16().size
        return 1.2e-16 * (Q + 64) * self.scale(vals, indexed)[:, :, None] * fmax[None, None, :]
