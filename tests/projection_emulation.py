"""NumPy emulation of the projection kernel (k_mode_project + k_project_reduce) for the tests.

Independent of the library: the mode values at the 16-point degree-8 rule come from ``QuarticEmulation.values16``, the
weights from ``weights16``, and the physical quadrature points are formed as the assembly forms them (``p0 + (J[r, 0] xi
+ J[r, 1] eta)``, every operation rounded on its own).  A factor (c, s, kappa) is
``phi(t) = exp(-s (t - c)^2) (cos(kappa t) - i sin(kappa t))``, the Gaussian part exactly 1 when s = 0.

``tolerance`` is the bound every comparison against these values uses: ``1.2e-16 (Q + 64 + 8 Phi) S_m`` with Q the
number of quadrature points, ``S_m = sum |det J| w_q |u_m(x_q)|`` (it bounds |P|, because |phi| <= 1) and Phi the largest
phase in radians -- the worst case of a fixed-order sum of Q terms, each with a few ulps from sincos / exp and the
products, plus the phase error of a last-bit difference in kappa t or in the point.
"""
from __future__ import annotations

import numpy as np

from pl_fem_vectoriel_amd.nonlinear import QUAD16_X
from quartic_emulation import QuarticEmulation


def factor_values(fac, t):
    """phi(t; c, s, kappa) of every factor (l, 3) at the points t (n,): complex (l, n)."""
    fac = np.asarray(fac, dtype=np.float64).reshape(-1, 3)
    c, s, kap = fac[:, 0:1], fac[:, 1:2], fac[:, 2:3]
    ph = kap * t[None]
    d = t[None] - c
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        g = np.where(s == 0.0, 1.0, np.exp(-(s * (d * d))))
    return g * np.cos(ph) - 1j * (g * np.sin(ph))


class ProjectionEmulation(QuarticEmulation):
    def points16(self):
        """(X, Y), each (ne, 16): the physical points of the 16-point rule."""
        p0 = self.mesh.p[:, self.mesh.t[0]]
        J = self.basis.J                                             # (2, 2, ne)
        q = p0[:, :, None] + (J[:, 0][:, :, None] * QUAD16_X[0][None, None] + J[:, 1][:, :, None] * QUAD16_X[1][None, None])
        return q[0], q[1]

    def scale(self, vals, indexed):
        """S (ncomp, k) = sum |det J| w_q |u_c,m(x_q)|."""
        U = self.values16(vals, indexed)
        return np.einsum("ckeq,eq->ck", np.abs(U), self.weights16())

    def tolerance(self, vals, indexed, xfac, yfac):
        """tol (ncomp, k, 1, 1) of the module docstring for these factor tables."""
        X, Y = self.points16()
        xfac, yfac = np.asarray(xfac).reshape(-1, 3), np.asarray(yfac).reshape(-1, 3)
        phase = np.abs(xfac[:, 2]).max() * np.abs(X).max() + np.abs(yfac[:, 2]).max() * np.abs(Y).max()
        return 1.2e-16 * (X.size + 64 + 8 * phase) * self.scale(vals, indexed)[:, :, None, None]

    def project(self, vals, indexed, xfac, yfac):
        """P complex (ncomp, k, lb, la), the output of plfem_mode_project."""
        ncomp, k = vals.shape[:2]
        X, Y = self.points16()
        U = self.values16(vals, indexed).reshape(ncomp * k, -1)      # (fields, points)
        fx = factor_values(xfac, X.reshape(-1))                       # (la, points)
        wfy = factor_values(yfac, Y.reshape(-1)) * self.weights16().reshape(-1)[None]
        out = np.empty((ncomp * k, wfy.shape[0], fx.shape[0]), dtype=np.complex128)
        for a in range(fx.shape[0]):
            out[:, :, a] = (U * fx[a][None]) @ wfy.T
        return out.reshape(ncomp, k, wfy.shape[0], fx.shape[0])

    def beam_norm(self, xfac, yfac):
        """sum |det J| w_q |phi_x(X_q) phi_y(Y_q)|^2 of one x- and one y-factor: the beam's norm in the 16-point inner
        product."""
        X, Y = self.points16()
        g = factor_values(xfac, X.reshape(-1))[0] * factor_values(yfac, Y.reshape(-1))[0]
        return float((self.weights16().reshape(-1) * (g.real ** 2 + g.imag ** 2)).sum())
