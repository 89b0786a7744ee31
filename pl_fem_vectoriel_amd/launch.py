"""Coupling of modes to fields arriving at or leaving the facet: far fields and Gaussian-beam launch maps (DESIGN.md
section 15).

Both are the projection of the mode fields on analytic fields that separate in x and y,

    P = integral u(x, y) phi_x(x) phi_y(y) dA,   phi(t; c, s, kappa) = exp(-s (t - c)^2) exp(-i kappa t),

a plane wave ``exp(-i kappa . x)`` (s = 0) or a Gaussian beam of any centre, waist and tilt (s = 1 / w^2), evaluated on
the GPU over the mesh the modes live on with the 16-point degree-8 rule (:meth:`ModeFields.project`,
``plfem_mode_project``).  It is defined on the discrete fields alone, like sampling, the Grams and the quartic overlap:
every component of a vectorial record (``Ex_dofs`` / ``Ey_dofs`` hold Hx / Hy) is projected on its own, and nothing is
assumed about the pencil the modes came from.  The reference has no counterpart: it turns no mode vector back into a
field.

What a lantern meets in practice is neither separable nor analytic -- an aberrated PSF, a speckle pattern, a measured
near field, the output of a beam-propagation run: complex images on a pixel grid.  :func:`field_coupling` takes a batch
of them: the overlap of every mode with the bilinear interpolant of every image, on the same
16-point rule and on the GPU (:meth:`ModeFields.project_sampled`, ``plfem_mode_project_sampled``), with the coupling
efficiency per mode, the power fraction the span of the modes captures, and the images' own power
(:func:`sampled_power`, exact for the interpolant, on the host).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from .fields import PROJECT_MAX_FACTORS, ModeFields, _frames, _grid_axis, _records, mode_overlap


def _axis(v, name: str) -> np.ndarray:
    """A 1-D axis of 1 .. 4096 finite numbers."""
    try:
        a = np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a 1-D array of finite numbers") from None
    if a.ndim != 1 or not 1 <= a.size <= PROJECT_MAX_FACTORS or not np.all(np.isfinite(a)):
        raise ValueError(f"{name} must be a 1-D array of 1 to {PROJECT_MAX_FACTORS} finite numbers")
    return a


def _pair(v, name: str) -> np.ndarray:
    try:
        a = np.asarray(v, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be two finite numbers") from None
    if a.size != 2 or not np.all(np.isfinite(a)):
        raise ValueError(f"{name} must be two finite numbers")
    return a


def _fields_of(modes, mesh, device) -> ModeFields:
    """The mesh's :class:`ModeFields`, with the records checked against it before any device call."""
    kind, vals, _ = _records(modes)
    if kind is None:
        raise ValueError("no mode records")
    if vals.shape[1] > 64:
        raise ValueError(f"at most 64 modes, got {vals.shape[1]}")
    mf = mesh if isinstance(mesh, ModeFields) else ModeFields(mesh, device=device)
    mf._check_records(modes)
    return mf


def far_field(modes: Sequence[Dict], mesh, kx, ky, device: Optional[int] = None) -> Dict[str, np.ndarray]:
    """Far field of the modes (at most 64) on the transverse-wavenumber grid ``kx`` (nkx,) x ``ky`` (nky,), in 1/um:

    * ``amplitude`` complex (ncomp, k, nky, nkx): ``F = integral u exp(-i (kx x + ky y)) dA`` of every component;
    * ``intensity`` (k, nky, nkx): the sum over the components of ``|F|^2``;
    * ``kx``, ``ky``: the axes.

    A direction of the far field is ``kappa / k0`` (its sine); :func:`encircled_na` turns the intensity into the NA a
    mode fills.  ``mesh`` is the mesh the modes were solved on, or its :class:`ModeFields`.  Argument errors raise
    ``ValueError`` before any device call."""
    kx, ky = _axis(kx, "kx"), _axis(ky, "ky")
    mf = _fields_of(modes, mesh, device)
    zero = np.zeros_like
    amp = mf.project(modes, np.stack([zero(kx), zero(kx), kx], 1), np.stack([zero(ky), zero(ky), ky], 1))
    return {"amplitude": amp, "intensity": (amp.real ** 2 + amp.imag ** 2).sum(0), "kx": kx, "ky": ky}


def encircled_na(intensity, kx, ky, k0: float, fraction: float = 0.95) -> np.ndarray:
    """Per mode, the smallest ``|kappa| / k0`` whose disc about kappa = 0 holds ``fraction`` of the grid's intensity sum
    (host only).  ``intensity`` is (k, nky, nkx) (or (nky, nkx) for one mode) on the grid ``kx`` x ``ky``; the radii
    tried are those of the grid points, so the answer is as fine as the grid."""
    kx, ky = _axis(kx, "kx"), _axis(ky, "ky")
    I = np.asarray(intensity, dtype=np.float64)
    single = I.ndim == 2
    if single:
        I = I[None]
    if I.ndim != 3 or I.shape[1:] != (ky.size, kx.size):
        raise ValueError(f"intensity must have shape (k, {ky.size}, {kx.size})")
    if not np.all(np.isfinite(I)) or np.any(I < 0):
        raise ValueError("intensity must be finite and >= 0")
    k0, fraction = float(k0), float(fraction)
    if not (np.isfinite(k0) and k0 > 0):
        raise ValueError("k0 must be a positive number")
    if not 0 < fraction <= 1:
        raise ValueError("fraction must be in (0, 1]")
    radius, inv = np.unique(np.hypot(kx[None, :], ky[:, None]).ravel(), return_inverse=True)
    na = np.empty(I.shape[0])
    for m, img in enumerate(I):
        inside = np.cumsum(np.bincount(inv.ravel(), weights=img.ravel(), minlength=radius.size))
        if inside[-1] <= 0:
            raise ValueError(f"mode {m} has no intensity on the grid")
        # (the last radius always qualifies: rounding of the comparison is kept from running past it)
        na[m] = radius[min(int(np.searchsorted(inside, fraction * inside[-1], "left")), radius.size - 1)] / k0
    return na[0] if single else na


def gaussian_coupling(modes: Sequence[Dict], mesh, waist: float, cx, cy, tilt=(0.0, 0.0), polarization=(1.0, 0.0),
                      device: Optional[int] = None) -> Dict[str, np.ndarray]:
    """Launch map of a Gaussian beam scanned over the facet: the beam of 1/e field radius ``waist`` (um) centred at
    every (cx[i], cy[j]) of the grid ``cx`` (nx,) x ``cy`` (ny,), with the transverse wavevector ``tilt`` =
    (kappa_x, kappa_y) in 1/um (``k0 sin(theta)`` per axis for a beam arriving at the angle theta in air):

        g(x, y) = exp(-((x - cx)^2 + (y - cy)^2) / waist^2) exp(-i (kappa_x x + kappa_y y)).

    * ``amplitude`` complex (ncomp, k, ny, nx): ``A = integral u g dA`` of every component (the tilt's phase refers to
      the origin, not to the spot);
    * ``efficiency`` (k, ny, nx) = ``|sum_c p_c A_c|^2 / (N_m pi waist^2 / 2)``, with ``N_m = sum_c integral u_c,m^2``
      (the diagonal of :func:`mode_overlap` of the modes with themselves) and ``p`` the unit vector along
      ``polarization`` (ignored for scalar records);
    * ``cx``, ``cy``: the axes.

    ``pi waist^2 / 2`` is the beam's norm over the whole plane: power the beam carries outside the mesh counts as
    lost, so a spot near or beyond the mesh boundary couples less than its overlap with the truncated beam would say.
    ``mesh`` is the mesh the modes were solved on, or its :class:`ModeFields`.  At most 64 modes.  Argument errors
    raise ``ValueError`` before any device call."""
    cx, cy = _axis(cx, "cx"), _axis(cy, "cy")
    try:
        w = float(waist)
    except (TypeError, ValueError):
        raise ValueError("waist must be a positive number") from None
    if not (0 < w < np.inf and 0 < w * w < np.inf and 1.0 / (w * w) < np.inf):
        raise ValueError("waist must be a positive number whose square and inverse square are finite")
    kap = _pair(tilt, "tilt")
    pol = _pair(polarization, "polarization")
    if not np.hypot(pol[0], pol[1]) > 0:
        raise ValueError("polarization must not be the zero vector")
    pol = pol / np.hypot(pol[0], pol[1])
    mf = _fields_of(modes, mesh, device)
    s = 1.0 / (w * w)
    amp = mf.project(modes, np.stack([cx, np.full_like(cx, s), np.full_like(cx, kap[0])], 1),
                     np.stack([cy, np.full_like(cy, s), np.full_like(cy, kap[1])], 1))
    norm = np.diag(mode_overlap(modes, mf, modes, mf)).copy()
    a = amp[0] if amp.shape[0] == 1 else pol[0] * amp[0] + pol[1] * amp[1]
    eff = (a.real ** 2 + a.imag ** 2) / (norm[:, None, None] * (np.pi * w * w / 2.0))
    return {"amplitude": amp, "efficiency": eff, "cx": cx, "cy": cy}


def _mass_1d(f: np.ndarray, h: float, axis: int) -> np.ndarray:
    """The 1-D piecewise-linear mass matrix of step ``h`` (cells of ``(h / 6) [[2, 1], [1, 2]]``) applied along ``axis``."""
    f = np.moveaxis(f, axis, -1)
    out = 4.0 * f
    out[..., 0] = 2.0 * f[..., 0]
    out[..., -1] = 2.0 * f[..., -1]
    out[..., 1:] += f[..., :-1]
    out[..., :-1] += f[..., 1:]
    return np.moveaxis(out * (h / 6.0), -1, axis)


def sampled_power(fields, x, y) -> np.ndarray:
    """``P_f`` (nf,): the exact integral of ``|bilinear interpolant of fields[f]|^2`` over the whole pixel grid ``x`` (nx,) x
    ``y`` (ny,) (host only).  On a cell the interpolant is a tensor product of linear functions, so the integral is the
    quadratic form of the tensor product of the two 1-D mass matrices, cells of ``(h / 6) [[2, 1], [1, 2]]``.  ``fields``
    and the axes are those of :meth:`ModeFields.project_sampled`."""
    xa, dx = _grid_axis(x, "x")
    ya, dy = _grid_axis(y, "y")
    f = _frames(fields, xa.size, ya.size)
    out = np.empty(f.shape[0])
    for s in range(0, f.shape[0], 64):                              # (bounded temporaries)
        c = f[s:s + 64]
        m = _mass_1d(_mass_1d(c, dx, 2), dy, 1)
        out[s:s + 64] = (c.real * m.real + c.imag * m.imag).sum(axis=(1, 2))
    return out


def field_coupling(modes: Sequence[Dict], mesh, fields, x, y, polarization=(1.0, 0.0), power=None,
                   device: Optional[int] = None) -> Dict[str, np.ndarray]:
    """Coupling of the modes (at most 64) to a batch of sampled input fields -- PSF frames of an aberrated telescope,
    speckle, a measured near field, the output of a beam-propagation run: ``fields`` complex or real (nf, ny, nx) or
    (ny, nx) on the pixel grid ``x`` (nx,) x ``y`` (ny,) (ascending, uniformly spaced), taken between the pixels as their
    bilinear interpolant and as 0 outside the grid (:meth:`ModeFields.project_sampled`).

    * ``amplitude`` complex (ncomp, k, nf): ``A = integral u F dA`` of every component (no conjugation);
    * ``efficiency`` (k, nf) = ``|sum_c p_c A_c|^2 / (N_m P_f)``, with ``N_m`` as in :func:`gaussian_coupling` and ``p`` the
      unit vector along ``polarization`` (ignored for scalar records);
    * ``captured`` (nf,) = ``c^H G^-1 c / P_f`` with ``G = mode_overlap(modes, mesh, modes, mesh)`` and ``c = sum_c p_c
      A_c``: the power fraction the span of the given modes takes, also for modes that are not orthonormal;
    * ``power`` (nf,) = ``P_f``: by default :func:`sampled_power`, the exact integral of the interpolant's modulus
      squared over the whole grid, so power outside the mesh counts as lost, as in :func:`gaussian_coupling`;
      ``power=`` takes the caller's own (nf,) finite, non-negative numbers instead.  A field without power gives NaN
      or inf.

    ``mesh`` is the mesh the modes were solved on, or its :class:`ModeFields`.  Argument errors raise ``ValueError``
    before any device call."""
    xa, dx = _grid_axis(x, "x")
    ya, dy = _grid_axis(y, "y")
    fr = _frames(fields, xa.size, ya.size)
    pol = _pair(polarization, "polarization")
    if not np.hypot(pol[0], pol[1]) > 0:
        raise ValueError("polarization must not be the zero vector")
    pol = pol / np.hypot(pol[0], pol[1])
    if power is None:
        pw = sampled_power(fr, xa, ya)
    else:
        try:
            pw = np.asarray(power, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"power must be an array of {fr.shape[0]} numbers") from None
        if pw.shape != (fr.shape[0],) or not np.all(np.isfinite(pw)) or np.any(pw < 0):
            raise ValueError(f"power must have shape ({fr.shape[0]},), finite and >= 0")
    mf = _fields_of(modes, mesh, device)
    amp = mf.project_sampled(modes, fr, xa, ya)
    G = mode_overlap(modes, mf, modes, mf)
    c = amp[0] if amp.shape[0] == 1 else pol[0] * amp[0] + pol[1] * amp[1]                # (k, nf)
    with np.errstate(divide="ignore", invalid="ignore"):
        eff = (c.real ** 2 + c.imag ** 2) / (np.diag(G)[:, None] * pw[None, :])
        cap = np.real(np.sum(np.conj(c) * np.linalg.solve(G, c), axis=0)) / pw
    return {"amplitude": amp, "efficiency": eff, "captured": cap, "power": pw}


__all__ = ["far_field", "encircled_na", "gaussian_coupling", "field_coupling", "sampled_power"]
