"""Intermodal nonlinear coupling tensor, effective area and mode-field diameter from one solve.

Every multimode / multicore nonlinear propagation model (SPM, XPM, FWM; ``gamma = n2 k0 / A_eff``) takes the overlap of
four mode fields as input:

    f_ijlm = integral (u_i . u_j)(u_l . u_m) dA / sqrt(N_i N_j N_l N_m),   N_i = integral u_i . u_i dA,

``A_eff,i = 1 / f_iiii`` and ``A_eff,ij = 1 / f_iijj``.  The products of four P2 fields are of degree 8, so the integral
runs on the 16-point degree-8 rule below (the assembly's six-point rule is of degree 4), over the mesh the modes live
on, on the GPU (:meth:`ModeFields.quartic`, ``plfem_mode_quartic``).  The norms and the gradient Grams come from
``plfem_mode_grams`` (:meth:`ModeFields.grams`).  :func:`nonlinearity_from_pairs` is the host math, a pure function of
the packed matrix and the Grams, so that it can be fed inputs from anywhere.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Optional, Sequence

import numpy as np

from .fields import ModeFields, _records
from .profile import reject_profile

# 16-point degree-8 rule on the reference triangle (0,0), (1,0), (0,1) (Dunavant 1985), digits polished on its moment
# equations; weights sum to 1/2.  The device copy is c_q16x / c_q16y / c_q16w of csrc/p2_element.h.
_A, _B, _C = 0.45929258829272315603, 0.17056930775176020662, 0.050547228317030975458     # the 3-point orbits (a, a)
_A2, _B2, _C2 = 0.081414823414553687942, 0.65886138449647958676, 0.89890554336593804908  # 1 - 2a
_P, _Q, _R = 0.0083947774099576053372, 0.26311282963463811342, 0.72849239295540428124    # the 6-point orbit
_T = 0.33333333333333333333
QUAD16_X = np.array([[_T, _A, _A, _A2, _B, _B, _B2, _C, _C, _C2, _P, _P, _Q, _Q, _R, _R],
                     [_T, _A, _A2, _A, _B, _B2, _B, _C, _C2, _C, _Q, _R, _P, _R, _P, _Q]])      # (2, 16)
QUAD16_W = np.array([0.072157803838893584126] + [0.047545817133642312397] * 3 + [0.051608685267359125141] * 3 +
                    [0.016229248811599040155] * 3 + [0.013615157087217497132] * 6)            # (16,)


def pair_index(k: int) -> np.ndarray:
    """(k, k) int64: the packed pair number p(min(i, j), max(i, j)), ``p(i,j) = i k - i (i - 1) / 2 + (j - i)``."""
    i, j = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    a, b = np.minimum(i, j), np.maximum(i, j)
    return a * k - a * (a - 1) // 2 + (b - a)


def expand_pairs(pairs) -> np.ndarray:
    """The packed np x np matrix as the (k, k, k, k) tensor Q[i, j, l, m] = pairs[p(i,j), p(l,m)]."""
    pairs = np.asarray(pairs, dtype=np.float64)
    npair = pairs.shape[0]
    k = int(round((np.sqrt(8 * npair + 1) - 1) / 2))
    if pairs.shape != (npair, npair) or k * (k + 1) // 2 != npair:
        raise ValueError("pairs must be np x np with np = k (k + 1) / 2")
    P = pair_index(k)
    return pairs[P[:, :, None, None], P[None, None, :, :]]


def nonlinearity_from_pairs(kind: str, pairs, grams: Dict[str, np.ndarray], k0: Optional[float] = None,
                            pairs_n2=None) -> Dict:
    """Host math of :func:`mode_nonlinearity` from the packed quartic overlap ``pairs`` (np x np, unweighted), the Grams
    ``grams`` (``ModeFields.grams`` names, any core split: only M_core + M_clad and the gradient forms enter) and,
    for gamma, the n2-weighted packed overlap ``pairs_n2`` with k0 in um^-1.  Lengths in um."""
    if kind not in ("vectorial", "scalar"):
        raise ValueError("kind must be 'vectorial' or 'scalar'")
    G = {nm: np.asarray(v, dtype=np.float64) for nm, v in grams.items()}
    N = np.diag(G["M_core"] + G["M_clad"]).copy()
    grad = np.diag(G["S"] if kind == "scalar" else G["K_core"] + G["K_clad"] + G["D"]).copy()
    Q = expand_pairs(pairs)
    k = N.size
    if Q.shape[0] != k:
        raise ValueError(f"pairs are of {Q.shape[0]} modes, the Grams of {k}")
    s = 1.0 / np.sqrt(N)
    scale = s[:, None, None, None] * s[None, :, None, None] * s[None, None, :, None] * s[None, None, None, :]
    f = Q * scale
    ii = np.arange(k)
    out = {"Q": Q, "pairs": np.asarray(pairs, dtype=np.float64), "norm": N, "f": f, "a_eff": 1.0 / f[ii, ii, ii, ii],
           "a_eff_pair": 1.0 / f[ii[:, None], ii[:, None], ii[None, :], ii[None, :]],
           "mfd_petermann": 2.0 * np.sqrt(2.0 * N / grad)}
    if pairs_n2 is not None:
        if k0 is None:
            raise ValueError("gamma needs k0")
        gamma = 1e21 * float(k0) * expand_pairs(pairs_n2) * scale
        out["gamma"] = gamma
        out["gamma_self"] = gamma[ii, ii, ii, ii].copy()
    return out


def mode_nonlinearity(modes: Sequence[Dict], mesh, geometry=None, n2=None, device: Optional[int] = None) -> Dict:
    """Nonlinear overlap quantities of the solver's modes (at most 64), in um.

    ``mesh`` is the mesh the modes were solved on (or its :class:`ModeFields`).  Returns

    * ``Q`` (k, k, k, k) = integral (u_i . u_j)(u_l . u_m) dA of the records as given, and ``pairs`` its packed np x np
      form (:func:`pair_index`);
    * ``norm`` (k,) ``N_i`` = integral u_i . u_i dA (``plfem_mode_grams``);
    * ``f`` = Q_ijlm / sqrt(N_i N_j N_l N_m) in um^-2, ``a_eff`` (k,) = 1 / f_iiii and ``a_eff_pair`` (k, k) = 1 / f_iijj
      in um^2;
    * ``mfd_petermann`` (k,) = 2 sqrt(2 N_i / G_i) in um (Petermann II), G = the S Gram for scalar records and
      (K_core + K_clad + D)_ii for vectorial ones.  K + D integrates |grad hx|^2 + |grad hy|^2 - 2 det(grad h), and the
      integral of det(grad h) vanishes for continuous fields that are zero on the boundary, which the interior-DOF
      vectorial records are, so G is the integral of |grad h|^2 exactly;
    * with ``n2 = (n2_core, n2_clad)`` in m^2/W (``geometry`` required): ``gamma`` (k, k, k, k) = 1e21 k0 Q^n2_ijlm /
      sqrt(N_i N_j N_l N_m) in 1/(W km), Q^n2 the overlap weighted by n2 of the region (the assembly's closed-disc core
      test), and ``gamma_self`` its diagonal.  The lanterns' cladding is air: ``n2_clad = 0``.

    The tensor refers to the records as given: for a degenerate pair, A_eff of one member depends on the rotation the
    solver returned (rotation-invariant combinations are not formed here).  For vectorial records it is the tensor of
    the records' transverse H fields, not reinterpreted; DESIGN.md section 13 explains why the vectorial records near
    the positive shift are not guided modes.  The records are not mutated.  Argument errors raise ``ValueError`` before
    any device call."""
    kind, vals, _ = _records(modes)
    if kind is None:
        raise ValueError("no mode records")
    k = vals.shape[1]
    if k > 64:
        raise ValueError(f"at most 64 modes, got {k}")
    if geometry is not None and not all(hasattr(geometry, a) for a in ("positions", "core_radii", "k0")):
        raise ValueError("geometry must have positions, core_radii and k0")
    if geometry is not None and np.atleast_2d(np.asarray(geometry.positions)).shape[0] > 64:
        raise ValueError("at most 64 cores")
    n2v = None
    if n2 is not None:
        if geometry is None:
            raise ValueError("n2 needs a geometry (the core test and k0)")
        reject_profile(geometry, "mode_nonlinearity with n2")
        try:
            n2v = np.asarray(n2, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError("n2 must be two finite numbers (n2_core, n2_clad) in m^2/W") from None
        if n2v.size != 2 or not np.all(np.isfinite(n2v)):
            raise ValueError("n2 must be two finite numbers (n2_core, n2_clad) in m^2/W")
    mf = mesh if isinstance(mesh, ModeFields) else ModeFields(mesh, device=device)
    mf._check_records(modes)                                # lengths, before the device
    norm_geom = SimpleNamespace(positions=np.zeros((0, 2)), core_radii=np.zeros(0))     # ncore = 0: every point "clad"
    grams = mf.grams(modes, norm_geom)
    pairs = mf.quartic(modes)
    pairs_n2 = mf.quartic(modes, geometry, (n2v[0], n2v[1])) if n2v is not None else None
    res = nonlinearity_from_pairs(kind, pairs, grams, k0=None if geometry is None else float(geometry.k0),
                                  pairs_n2=pairs_n2)
    res["grams"] = grams
    return res


__all__ = ["mode_nonlinearity", "nonlinearity_from_pairs", "expand_pairs", "pair_index", "QUAD16_X", "QUAD16_W"]
