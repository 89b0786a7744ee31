"""Core displacement, radius and ellipticity sensitivities of every mode from one solve.

A core that moves THROUGH a fixed mesh changes the discrete permittivity in steps.  A mesh that
moves WITH the core does not: take a vertex velocity field V -- a rigid translation, a radial scaling or a stretch on the
core disc and a collar round it, decaying to zero before the next core -- and move every vertex by ``t V``.  Every
quadrature point keeps its material, every element matrix is a smooth rational function of t, and the derivative of both
pencils has a closed form per element (the volume form of the shape derivative, the velocity method).  For straight-sided
P2 elements that is the exact derivative of the discrete eigenvalue.  :meth:`ModeFields.velocity_grams` reduces it on the
GPU to k x k matrices per velocity over the few elements where V has a gradient; everything here is host math on them:

* :func:`core_velocities` -- the P1 fields dx, dy, dr, e2c, e2s of every core;
* :func:`shape_response_from_grams`, :func:`shape_response` -- ``d n_eff / d p`` of every mode for every velocity by
  Hellmann-Feynman, degenerate clusters as in :func:`.profile_response.profile_sensitivity_from_grams`;
* :func:`disorder_statistics` -- first-order standard deviations of n_eff and of n_eff differences under independent
  core-position and radius errors.

First order only; touching or overlapping cores are excluded (the collar does not fit); a quadrature point that a finite
step would carry across a rim is not seen by a derivative.  The vectorial numbers describe the reference's pencil as it is
("What the vectorial numbers mean").
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from .fields import VELOCITY_GRAM_NAMES, VELOCITY_MAX, ModeFields, _mesh_arrays, _records
from .profile import index_profile_of
from .profile_response import _pencil, _rtol, _sensitivity_from_pencil
from .solver_fem import TrueVectorialMaxwellSolver, _core_table

KINDS = ("dx", "dy", "dr", "e2c", "e2s")


def _boundary_distance(p: np.ndarray, t: np.ndarray, c: np.ndarray) -> float:
    """Distance from the point ``c`` to the boundary edges of the mesh (the edges of exactly one element)."""
    e = np.sort(np.hstack([t[[0, 1]], t[[1, 2]], t[[0, 2]]]), axis=0)
    key, counts = np.unique(e[0].astype(np.int64) * p.shape[1] + e[1], return_counts=True)
    key = key[counts == 1]
    a, b = p[:, key // p.shape[1]], p[:, key % p.shape[1]]
    ab = b - a
    s = np.clip(((c[:, None] - a) * ab).sum(0) / np.maximum((ab * ab).sum(0), 1e-300), 0.0, 1.0)
    return float(np.sqrt((((a + s * ab) - c[:, None]) ** 2).sum(0)).min())


def core_velocities(mesh, geometry, kinds: Sequence[str] = KINDS, inner: float = 1.5, cores: Optional[Sequence[int]] = None):
    """The P1 velocity fields that move, resize and stretch each core with its surroundings: ``(V, labels)`` with ``V``
    (nvel, nv, 2) and ``labels`` a list of ``(core, kind)``, core-major.

    For core c at ``(cx, cy)`` with radius r, ``X = x - cx``, ``Y = y - cy``, ``rho = hypot(X, Y)``: ``r_in = inner r``, d the
    smallest of the gaps from the centre to the other discs' rims and to the domain boundary, ``r_out = r_in + 0.8 (d -
    r_in)`` and the cut-off ``eta = clip((r_out - rho) / (r_out - r_in), 0, 1)``, exactly 1 up to ``r_in`` and 0 from
    ``r_out`` on.  Fields: ``dx = (eta, 0)``, ``dy = (0, eta)``, ``dr = eta (X, Y) / r`` (unit radius change), ``e2c = eta (X,
    -Y) / r`` and ``e2s = eta (Y, X) / r`` (the two ellipticities), all exactly linear where ``eta = 1``.

    ``geometry`` gives ``positions`` / ``core_radii`` (of its base for a ``ProfiledGeometry``: the shapes of the profile
    are then assumed to ride with V -- a layer that crosses a collar is sheared with it).  ``cores``: the core indices to
    build fields for, default all.  ``ValueError`` when ``d <= r_in`` (touching or overlapping cores: the collar does not
    fit), when an element with a vertex in the closed disc has a vertex with ``eta < 1`` (the mesh is too coarse for this
    ``inner``), or when an element with ``eta > 0`` at a vertex has a vertex in another core's closed disc."""
    p, t = _mesh_arrays(mesh)
    p = np.asarray(p, dtype=np.float64)
    if not all(hasattr(geometry, a) for a in ("positions", "core_radii")):
        raise ValueError("geometry must have positions and core_radii")
    table = _core_table(geometry)
    ncore = table.shape[0]
    kinds = tuple(kinds)
    if not kinds or any(kd not in KINDS for kd in kinds):
        raise ValueError(f"kinds must be a non-empty selection of {', '.join(KINDS)}")
    if not (np.isfinite(inner) and inner > 1.0):
        raise ValueError("inner must be finite and > 1")
    which = list(range(ncore)) if cores is None else [int(c) for c in cores]
    if not which or any(not 0 <= c < ncore for c in which):
        raise ValueError(f"cores must be indices in [0, {ncore})")
    V, labels = [], []
    in_disc = [(p[0] - cx) ** 2 + (p[1] - cy) ** 2 <= r * r for cx, cy, r in table]
    for c in which:
        cx, cy, r = table[c]
        X, Y = p[0] - cx, p[1] - cy
        rho = np.hypot(X, Y)
        r_in = inner * r
        gaps = [np.hypot(ox - cx, oy - cy) - orad for j, (ox, oy, orad) in enumerate(table) if j != c]
        d = min(gaps + [_boundary_distance(p, t, np.array([cx, cy]))])
        if d <= r_in:
            raise ValueError(f"core {c}: the collar does not fit (gap {d:g} <= inner x radius {r_in:g}): touching or "
                             "overlapping cores, or a core at the domain boundary")
        r_out = r_in + 0.8 * (d - r_in)
        eta = np.clip((r_out - rho) / (r_out - r_in), 0.0, 1.0)
        et = eta[t]                                                     # (3, ne)
        if np.any(in_disc[c][t].any(0) & (et < 1.0).any(0)):
            raise ValueError(f"core {c}: an element that touches the disc reaches past inner x radius: the mesh is too "
                             f"coarse for inner = {inner:g}")
        others = np.zeros(p.shape[1], dtype=bool)
        for j in range(ncore):
            if j != c:
                others |= in_disc[j]
        if np.any((et > 0.0).any(0) & others[t].any(0)):
            raise ValueError(f"core {c}: the collar reaches an element of another core")
        zero = np.zeros_like(eta)
        fields = {"dx": (eta, zero), "dy": (zero, eta), "dr": (eta * X / r, eta * Y / r),
                  "e2c": (eta * X / r, -(eta * Y / r)), "e2s": (eta * Y / r, eta * X / r)}
        for kd in kinds:
            V.append(np.stack(fields[kd], axis=1))
            labels.append((c, kd))
    return np.ascontiguousarray(np.stack(V)), labels


def _velocity_stack(kind: str, velocity_grams: Dict[str, np.ndarray], k: int):
    names = VELOCITY_GRAM_NAMES[kind]
    if any(nm not in velocity_grams for nm in names):
        raise ValueError(f"velocity_grams must hold {', '.join(names)}")
    T = {nm: np.asarray(velocity_grams[nm], dtype=np.float64) for nm in names}
    T = {nm: 0.5 * (v + np.swapaxes(v, -1, -2)) for nm, v in T.items()}
    if any(v.ndim != 3 or v.shape[1:] != (k, k) for v in T.values()) or len({v.shape for v in T.values()}) != 1:
        raise ValueError("the velocity Grams must be (nvel, k, k) with k = beta.size, all of one shape")
    return T


def shape_response_from_grams(kind: str, grams: Dict[str, np.ndarray], velocity_grams: Dict[str, np.ndarray], beta, k0: float,
                              direction=None, cluster_rtol: float = 1e-10,
                              alpha_p: float = TrueVectorialMaxwellSolver.ALPHA_P) -> Dict:
    """The k x k host math of :func:`shape_response`: a pure function of the Grams of the solve under
    ``ModeFields.profile_grams`` names (``M``, ``M_w``, ``K_w``, ``D`` or ``M``, ``M_w``, ``S``) and of the velocity Grams
    (``ModeFields.velocity_grams`` names, each (nvel, k, k)).  Vectorial: ``dA/dp = dK_w + alpha_p dD - k0^2 dM``, ``dB/dp =
    dM_w``; scalar: ``dA/dp = dS - k0^2 dM_w``, ``dB/dp = dM``.

    Returns ``dneff_dp`` (k, nvel), d n_eff of mode m per unit step along velocity p; ``sensitivity`` (nvel, k, k), ``S_p[m,
    n] = h_m^T (dA/dp - mu_n dB/dp) h_n`` between B-normalised records; ``cluster`` (k,); ``rayleigh_defect`` (k,); with
    ``direction`` (nvel,) also ``dneff_direction`` (k,), the derivative along ``sum_p direction_p V_p``.  Degenerate
    clusters as in :func:`.profile_response.profile_sensitivity_from_grams`."""
    _rtol(cluster_rtol)
    _, A, B, mu, sgn, beta = _pencil(kind, grams, beta, k0, alpha_p)
    k, k0 = beta.size, float(k0)
    T = _velocity_stack(kind, velocity_grams, k)
    nvel = T["dM"].shape[0]
    if kind == "vectorial":
        dA, dB = T["dK_w"] + alpha_p * T["dD"] - k0 * k0 * T["dM"], T["dM_w"]
    else:
        dA, dB = T["dS"] - k0 * k0 * T["dM_w"], T["dM"]
    dirs = None
    if direction is not None:
        try:
            dirs = np.asarray(direction, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"direction must be {nvel} finite numbers, one per velocity") from None
        if dirs.size != nvel or not np.all(np.isfinite(dirs)):
            raise ValueError(f"direction must be {nvel} finite numbers, one per velocity")
    return _sensitivity_from_pencil(A, B, dA, dB, mu, sgn, beta, k0, dirs, cluster_rtol)


def _as_profile_grams(kind: str, grams: Dict[str, np.ndarray], eps_core: float, eps_clad: float) -> Dict[str, np.ndarray]:
    """The region Grams of ``ModeFields.grams`` under the names of ``ModeFields.profile_grams`` (w = 1 / eps or eps)."""
    wc, wl = (1.0 / eps_core, 1.0 / eps_clad) if kind == "vectorial" else (eps_core, eps_clad)
    out = {"M": grams["M_core"] + grams["M_clad"], "M_w": wc * grams["M_core"] + wl * grams["M_clad"]}
    if kind == "vectorial":
        out.update(K_w=wc * grams["K_core"] + wl * grams["K_clad"], D=grams["D"])
    else:
        out["S"] = grams["S"]
    return out


def shape_response(modes: Sequence[Dict], mesh, geometry, velocities=None, labels=None, kinds: Sequence[str] = KINDS,
                   inner: float = 1.5, direction=None, cluster_rtol: float = 1e-10, device: Optional[int] = None) -> Dict:
    """d n_eff of every mode per unit step of the mesh along velocity fields, from one solve.

    ``velocities`` (nvel, nv, 2) or (nv, 2): P1 fields on the mesh vertices, with optional ``labels`` (one per
    velocity); default :func:`core_velocities` of ``geometry`` with ``kinds`` and ``inner``.  A caller's own V goes the
    same way: ``V = x`` (``mesh.p.T``) scales the whole section (a taper step), a stretch is ``(x, 0)``.  The material of
    every quadrature point rides with V; for a ``ProfiledGeometry`` or a sampled map that means the profile's shapes are
    assumed to be carried along.  ``mesh``: the mesh or its :class:`ModeFields`.

    Returns what :func:`shape_response_from_grams` does, and ``labels``, ``count`` (nvel,) the elements each velocity has
    a gradient on, ``grams`` (``profile_grams`` names) and ``velocity_grams``.  When every label is a ``(core, kind)`` pair
    also ``dneff_dx``, ``dneff_dy``, ``dneff_dr``, ``dneff_de2c``, ``dneff_de2s`` for the kinds present, each (k, ncore) over
    the cores of the geometry (NaN for a core without that velocity).  Nothing is assembled, factorised or solved again.
    Argument errors raise ``ValueError`` before any device call."""
    kind, _, beta = _records(modes)
    if kind is None:
        raise ValueError("no mode records")
    if not np.all(np.isfinite(beta) & (beta > 0)):
        raise ValueError("every record needs a finite, positive 'beta'")
    k0 = getattr(geometry, "k0", None)
    if k0 is None or not np.isfinite(float(k0)) or float(k0) <= 0:
        raise ValueError("geometry must have a finite, positive k0")
    k0 = float(k0)
    _rtol(cluster_rtol)
    mf = mesh if isinstance(mesh, ModeFields) else ModeFields(mesh, device=device)
    _, vals, _ = mf._check_records(modes)                   # lengths, before the device
    mat = mf._material(geometry)
    if velocities is None:
        if labels is not None:
            raise ValueError("labels come with velocities")
        vel, labels = core_velocities(mf.mesh, geometry, kinds, inner)
    else:
        vel = np.asarray(velocities, dtype=np.float64)
        if vel.ndim == 2:
            vel = vel[None]
        if vel.ndim != 3 or vel.shape[0] < 1 or vel.shape[1:] != (mf.nv, 2) or not np.all(np.isfinite(vel)):
            raise ValueError(f"velocities must be finite, of shape (nvel, {mf.nv}, 2) or ({mf.nv}, 2)")
        vel = np.ascontiguousarray(vel)
        labels = list(range(vel.shape[0])) if labels is None else list(labels)
        if len(labels) != vel.shape[0]:
            raise ValueError("one label per velocity")
    nvel = vel.shape[0]
    if direction is not None:
        try:
            d = np.asarray(direction, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"direction must be {nvel} finite numbers, one per velocity") from None
        if d.size != nvel or not np.all(np.isfinite(d)):
            raise ValueError(f"direction must be {nvel} finite numbers, one per velocity")
    mf._ensure_locator()
    staged, _src = mf._stage(vals)
    profile = index_profile_of(geometry)
    if profile is None:
        grams = _as_profile_grams(kind, mf._grams_staged(kind, staged, mat.cores), mat.eps_core, mat.eps_clad)
    else:
        grams = mf._profile_grams_staged(kind, staged, profile.table(), profile.eps_background, index_map=profile.index_map)
    parts = [mf._velocity_grams_staged(kind, staged, mat, vel[s:s + VELOCITY_MAX]) for s in range(0, nvel, VELOCITY_MAX)]
    vg = {nm: np.concatenate([q[nm] for q in parts]) for nm in parts[0]}
    res = shape_response_from_grams(kind, grams, vg, beta, k0, direction, cluster_rtol)
    res.update(labels=labels, count=vg.pop("count"), grams=grams, velocity_grams=vg)
    if all(isinstance(lb, tuple) and len(lb) == 2 and lb[1] in KINDS for lb in labels):
        ncore = mat.cores.shape[0]
        for kd in KINDS:
            cols = [(i, lb[0]) for i, lb in enumerate(labels) if lb[1] == kd]
            if cols:
                out = np.full((beta.size, ncore), np.nan)
                for i, c in cols:
                    out[:, c] = res["dneff_dp"][:, i]
                res["dneff_" + (kd if kd.startswith("d") else "d" + kd)] = out
    return res


def disorder_statistics(response: Dict, sigma_position, sigma_radius=0.0) -> Dict:
    """First-order standard deviations of n_eff under fabrication disorder, from :func:`shape_response` with the default
    velocities (``dneff_dx``, ``dneff_dy`` and, for ``sigma_radius``, ``dneff_dr``, each (k, ncore)).

    The errors are independent from core to core: each core centre is displaced isotropically with standard deviation
    ``sigma_position`` per axis, each radius changes with ``sigma_radius`` (numbers, or one per core; um).  Returns
    ``neff_std`` (k,), ``sqrt(sum_c sigma_p,c^2 (dx_mc^2 + dy_mc^2) + sigma_r,c^2 dr_mc^2)``, and ``dneff_std`` (k, k), the same
    for every difference ``n_eff,m - n_eff,n`` (with the differences of the derivatives: correlated shifts cancel).  Only k x
    ncore arithmetic; valid to first order and, inside a degenerate cluster, for the cluster values (see
    :func:`shape_response_from_grams`)."""
    if any(nm not in response for nm in ("dneff_dx", "dneff_dy")):
        raise ValueError("response must hold dneff_dx and dneff_dy (shape_response with the default velocities)")
    gx, gy = (np.asarray(response[nm], dtype=np.float64) for nm in ("dneff_dx", "dneff_dy"))
    ncore = gx.shape[1]

    def sigma(v, name):
        try:
            a = np.broadcast_to(np.asarray(v, dtype=np.float64), (ncore,))
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a number or {ncore} numbers, one per core") from None
        if not np.all(np.isfinite(a) & (a >= 0)):
            raise ValueError(f"{name} must be finite and >= 0")
        return a

    sp, sr = sigma(sigma_position, "sigma_position"), sigma(sigma_radius, "sigma_radius")
    terms = [(gx, sp), (gy, sp)]
    if np.any(sr > 0):
        if "dneff_dr" not in response:
            raise ValueError("sigma_radius needs dneff_dr in response")
        terms.append((np.asarray(response["dneff_dr"], dtype=np.float64), sr))
    if any(np.any(np.isnan(g[:, s > 0])) for g, s in terms):
        raise ValueError("response lacks the derivative of a core with a non-zero sigma")
    var = sum((np.where(s > 0, g, 0.0) ** 2 * s ** 2).sum(1) for g, s in terms)
    dvar = sum((((np.where(s > 0, g, 0.0)[:, None, :] - np.where(s > 0, g, 0.0)[None, :, :]) * s) ** 2).sum(2) for g, s in terms)
    return {"neff_std": np.sqrt(var), "dneff_std": np.sqrt(dvar)}


__all__ = ["core_velocities", "shape_response", "shape_response_from_grams", "disorder_statistics"]
