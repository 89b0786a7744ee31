"""Modal power, power confinement and power orthogonality of vectorial modes.

The solver's records hold the transverse magnetic field (``Ex_dofs`` / ``Ey_dofs`` are Hx / Hy).  With fields varying as
exp(j (w t - beta z)), ``curl H = j w eps0 eps E`` gives the electric field from them; in units of ``Z0`` (``e = E / Z0``,
so that e has the units of H) and with ``w = 1 / eps``::

    gx = -(Hx,xx + Hy,xy)      gy = -(Hx,xy + Hy,yy)
    Ex    =  w (beta Hy + gy / beta) / k0
    Ey    = -w (beta Hx + gx / beta) / k0
    Ez_im = -w (dx Hy - dy Hx) / k0                      (Ez = j Ez_im)
    Sz    =  (Ex Hy - Ey Hx) / 2

(:meth:`.fields.ModeFields.sample_e`).  The cross power of two modes of one mesh is::

    P[m, n] = 1/2 int (Ex_m Hy_n - Ey_m Hx_n) dA = (beta_m M_w[m, n] + G_w[m, n] / beta_m) / (2 k0)

with the Grams ``M_w``, ``G_w`` of :meth:`.fields.ModeFields.flux_grams` (``plfem_flux_grams``), which are free of beta
and k0 and split into the core discs and the rest: :func:`power_quantities_from_grams` is the k x k host math on them,
:func:`mode_power` the whole path from records.  ``P`` is in units of ``Z0 |H|^2 length^2``: multiply by ``Z0_OHM`` for
watts with H in A / length.

These are the formulas for any P2 field with a given beta, eigenpair or not.  The transverse E rests on element-wise
second derivatives of a P2 field, so it converges at first order in h.  The solver reproduces the reference pencil's sign
convention as coded, so the power orthogonality of its modes is reported (``orthogonality``), not promised.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from .fields import FLUX_GRAM_NAMES, ModeFields

Z0_OHM = 376.730313668              # impedance of free space: E = Z0 e


def power_quantities_from_grams(grams: Dict[str, np.ndarray], beta, k0: float) -> Dict[str, np.ndarray]:
    """Power quantities of k modes from their flux Grams (pure NumPy).  ``grams``: ``M_w_core``, ``M_w_rest``,
    ``G_w_core``, ``G_w_rest``, each (k, k); ``beta`` (k,) finite and non-zero; ``k0`` finite and positive.  Returns

    * ``cross`` (k, k): ``P[m, n] = (beta_m M_w[m, n] + G_w[m, n] / beta_m) / (2 k0)``, core + rest;
    * ``cross_core``: the same over the core discs only;
    * ``power`` (k,): ``diag(cross)``, the power each mode carries along z;
    * ``core_fraction`` (k,): ``diag(cross_core) / power``, the power-confinement factor (0 where ``power`` is 0);
    * ``cross_sym``: ``(P + P^T) / 2``;
    * ``orthogonality`` (k, k): ``|cross_sym[m, n]| / sqrt(|P_m P_n|)`` with a zero diagonal (0 where a power is 0);
    * ``scale`` (k,): ``1 / sqrt(|power|)``, the amplitude factor that brings a mode to unit power in units of Z0 (0 where
      ``power`` is 0); multiply by ``1 / sqrt(Z0_OHM)`` for SI."""
    try:
        G = {nm: np.asarray(grams[nm], dtype=np.float64) for nm in FLUX_GRAM_NAMES}
    except (KeyError, TypeError, ValueError):
        raise ValueError("grams must hold " + ", ".join(FLUX_GRAM_NAMES) + " as real arrays") from None
    b = np.asarray(beta, dtype=np.float64).reshape(-1)
    k = b.size
    if any(g.shape != (k, k) for g in G.values()):
        raise ValueError(f"every Gram must have shape ({k}, {k}): one row and column per entry of beta")
    if not np.all(np.isfinite(b) & (b != 0)):
        raise ValueError("every beta must be finite and non-zero")
    k0 = float(k0)
    if not (np.isfinite(k0) and k0 > 0):
        raise ValueError("k0 must be finite and positive")

    def cross_of(M, Gw):
        return (b[:, None] * M + Gw / b[:, None]) / (2.0 * k0)

    cross_core = cross_of(G["M_w_core"], G["G_w_core"])
    cross = cross_of(G["M_w_core"] + G["M_w_rest"], G["G_w_core"] + G["G_w_rest"])
    power = np.diag(cross).copy()
    live = power != 0
    safe = np.where(live, power, 1.0)
    core_fraction = np.where(live, np.diag(cross_core) / safe, 0.0)
    cross_sym = 0.5 * (cross + cross.T)
    scale = np.where(live, 1.0 / np.sqrt(np.abs(safe)), 0.0)
    orthogonality = np.abs(cross_sym) * scale[:, None] * scale[None, :]
    np.fill_diagonal(orthogonality, 0.0)
    return {"cross": cross, "cross_core": cross_core, "power": power, "core_fraction": core_fraction, "cross_sym": cross_sym,
            "orthogonality": orthogonality, "scale": scale}


def mode_power(modes: Sequence[Dict], mesh, geometry, fields: Optional[ModeFields] = None) -> Dict[str, np.ndarray]:
    """Modal power, power confinement and power orthogonality of the vectorial ``modes`` solved on ``mesh`` with
    ``geometry`` (k0, and the material: its index profile if it carries one, else its core discs at n_core on n_clad),
    from one ``plfem_flux_grams`` call: what :func:`power_quantities_from_grams` returns, plus ``grams``.  ``fields``: a
    :class:`ModeFields` of the mesh to reuse (its analysis and locator); ``mesh`` may also be one.  The records are not
    mutated.  Argument errors raise ``ValueError`` before any device call."""
    try:
        k0 = float(geometry.k0)
    except (AttributeError, TypeError, ValueError):
        raise ValueError("geometry must have k0") from None
    if not (np.isfinite(k0) and k0 > 0):
        raise ValueError("k0 must be finite and positive")
    mf = fields if fields is not None else (mesh if isinstance(mesh, ModeFields) else ModeFields(mesh))
    grams = mf.flux_grams(modes, geometry)
    beta = np.array([float(m["beta"]) for m in modes], dtype=np.float64)
    res = power_quantities_from_grams(grams, beta, k0)
    res["grams"] = grams
    return res


__all__ = ["Z0_OHM", "power_quantities_from_grams", "mode_power"]
