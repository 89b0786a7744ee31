"""Group index, index sensitivities and bend response of profile solves from one solve.

The pencils of a profile solve (:meth:`ModeFields.profile_grams` for the forms) are

* vectorial: ``A = K_w + alpha_p D - k0^2 M``, ``B = M_w`` with ``w = 1 / eps``, ``mu = beta^2``;
* scalar: ``A = S - k0^2 M_w``, ``B = M`` with ``w = eps``, ``lambda = -beta^2``,

and ``IndexProfile.epsilon`` is linear in the VALUES of the profile at fixed shapes: the background, ``eps_a`` and ``eps_b``
of every layer, every pixel of the map.  A first-order change of those values is a :class:`.profile.ProfileTangent`, and
along it ``w`` changes by ``dw = -d eps / eps^2`` (vectorial) or ``d eps`` (scalar) point by point.  So the derivative of
the projected pencil along a tangent is ``(K_d, M_d)`` (vectorial) or ``(-k0^2 M_d, 0)`` (scalar) with ``M_d``, ``K_d`` the
Grams of the modes under ``dw``, and a bend ``eps -> eps (1 + 2 kappa Xt)`` moves it by ``-2 kappa (K_wX, M_wX)`` or
``(-2 kappa k0^2 M_wX, 0)``: all of them columns of one GPU reduction, :meth:`ModeFields.profile_tangent_grams`.
Material dispersion (a tangent of ``dn / d lambda0``), the index of a layer (thermal drift, index inhomogeneity) and
bends are the same Hellmann-Feynman computation with different tangents; everything here is k x k host math on the
Grams.  Nothing is assembled, factorised or solved again.

Shapes (radii, centres) are not values: on a fixed mesh the discrete permittivity is a staircase in them (DESIGN.md
section 20); their derivatives come from moving the mesh with the core, :mod:`.shape`.  The
vectorial numbers describe the reference's pencil as it is ("What the vectorial numbers mean").
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from .bend import _bend_from_pencil, _curvature_and_angle
from .cores import _cluster_members, _directional_dmu, _sym
from .dispersion import _clusters, _dispersion_from_pencil
from .fields import ModeFields, _records
from .profile import ProfileTangent, index_profile_of
from .solver_fem import TrueVectorialMaxwellSolver


def _pencil(kind: str, grams: Dict[str, np.ndarray], beta, k0: float, alpha_p: float):
    """``(G, A, B, mu, sgn, beta)`` of a profile solve from its Grams (``ModeFields.profile_grams`` names)."""
    if kind not in ("vectorial", "scalar"):
        raise ValueError("kind must be 'vectorial' or 'scalar'")
    need = ("M", "M_w", "K_w", "D") if kind == "vectorial" else ("M", "M_w", "S")
    if any(nm not in grams for nm in need):
        raise ValueError(f"grams must hold {', '.join(need)}")
    G = {nm: _sym(grams[nm]) for nm in need}
    beta = np.asarray(beta, dtype=np.float64).reshape(-1)
    k = beta.size
    if k < 1 or any(G[nm].shape != (k, k) for nm in need):
        raise ValueError("the Grams must be k x k with k = beta.size >= 1")
    k0 = float(k0)
    if kind == "vectorial":
        return G, G["K_w"] + alpha_p * G["D"] - k0 * k0 * G["M"], G["M_w"], beta ** 2, 1.0, beta
    return G, G["S"] - k0 * k0 * G["M_w"], G["M"], -beta ** 2, -1.0, beta


def _tangent_stack(kind: str, tangent_grams: Dict[str, np.ndarray], names, k: int, lead=None):
    """The named Grams of ``ModeFields.profile_tangent_grams``, symmetrised, each (..., k, k)."""
    if any(nm not in tangent_grams for nm in names):
        raise ValueError(f"tangent_grams must hold {', '.join(names)}")
    T = [_sym(tangent_grams[nm]) for nm in names]
    if any(t.shape[-2:] != (k, k) or (lead is not None and t.ndim != lead + 2) for t in T) or len({t.shape for t in T}) != 1:
        raise ValueError("the tangent Grams must be k x k with k = beta.size, all of one shape")
    return T


def _rtol(cluster_rtol) -> None:
    if not (np.isfinite(cluster_rtol) and cluster_rtol >= 0):
        raise ValueError("cluster_rtol must be finite and >= 0")


def profile_dispersion_from_grams(kind: str, grams: Dict[str, np.ndarray], tangent_grams: Optional[Dict[str, np.ndarray]],
                                  beta, k0: float, cluster_rtol: float = 1e-10,
                                  alpha_p: float = TrueVectorialMaxwellSolver.ALPHA_P) -> Dict:
    """The k x k host math of :func:`profile_dispersion`: a pure function of the Grams of the profile solve
    (``ModeFields.profile_grams`` names) and of ``M_d`` (and ``K_d``) (1, k, k) or (k, k) of the tangent ``d eps / d k0``
    (``ModeFields.profile_tangent_grams`` names; None: no material dispersion).  Vectorial: ``A' = -2 k0 M + K_d``, ``B' =
    M_d``; scalar: ``A' = -2 k0 M_w - k0^2 M_d``, ``B' = 0``.  Returns what :func:`.dispersion.dispersion_from_grams` does."""
    _rtol(cluster_rtol)
    G, A, B, mu, sgn, beta = _pencil(kind, grams, beta, k0, alpha_p)
    k, k0 = beta.size, float(k0)
    names = ("M_d", "K_d") if kind == "vectorial" else ("M_d",)
    if tangent_grams is None:
        T = [np.zeros((k, k)) for _ in names]
    else:
        T = [t.reshape(-1, k, k) for t in _tangent_stack(kind, tangent_grams, names, k)]
        if T[0].shape[0] != 1:
            raise ValueError("dispersion takes the Grams of ONE tangent, d eps / d k0")
        T = [t[0] for t in T]
    if kind == "vectorial":
        Ad, Bd = -2.0 * k0 * G["M"] + T[1], T[0]
    else:
        Ad, Bd = -2.0 * k0 * G["M_w"] - k0 * k0 * T[0], np.zeros_like(B)
    return _dispersion_from_pencil(A, B, Ad, Bd, mu, sgn, beta, cluster_rtol)


def profile_sensitivity_from_grams(kind: str, grams: Dict[str, np.ndarray], tangent_grams: Dict[str, np.ndarray], beta,
                                   k0: float, direction=None, cluster_rtol: float = 1e-10,
                                   alpha_p: float = TrueVectorialMaxwellSolver.ALPHA_P) -> Dict:
    """The k x k host math of :func:`profile_sensitivity`: a pure function of the Grams of the profile solve and of
    ``M_d`` (and ``K_d``) (ntan, k, k), one per tangent p.  Vectorial: ``dA/dp = K_d[p]``, ``dB/dp = M_d[p]``; scalar:
    ``dA/dp = -k0^2 M_d[p]``, ``dB/dp = 0``.

    Returns ``dneff_dp`` (k, ntan), d n_eff of mode m per unit step along tangent p; ``sensitivity`` (ntan, k, k),
    ``S_p[m, n] = h_m^T (dA/dp - mu_n dB/dp) h_n`` between B-normalised records; ``cluster`` (k,); ``rayleigh_defect``
    (k,); with ``direction`` (ntan,) also ``dneff_direction`` (k,), the derivative along ``sum_p direction_p tangent_p``.
    Degenerate clusters as in :func:`.cores.core_quantities_from_grams`: inside a cluster every column holds the
    generalised eigenvalues of ``S_p`` on the cluster block, ascending, handed to the members in record order."""
    _rtol(cluster_rtol)
    G, A, B, mu, sgn, beta = _pencil(kind, grams, beta, k0, alpha_p)
    k, k0 = beta.size, float(k0)
    names = ("M_d", "K_d") if kind == "vectorial" else ("M_d",)
    T = _tangent_stack(kind, tangent_grams, names, k, lead=1)
    ntan = T[0].shape[0]
    if kind == "vectorial":
        dA, dB = T[1], T[0]
    else:
        dA, dB = -k0 * k0 * T[0], np.zeros_like(T[0])
    dirs = None
    if direction is not None:
        try:
            dirs = np.asarray(direction, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"direction must be {ntan} finite numbers, one per tangent") from None
        if dirs.size != ntan or not np.all(np.isfinite(dirs)):
            raise ValueError(f"direction must be {ntan} finite numbers, one per tangent")
    return _sensitivity_from_pencil(A, B, dA, dB, mu, sgn, beta, k0, dirs, cluster_rtol)


def _sensitivity_from_pencil(A, B, dA, dB, mu, sgn, beta, k0: float, dirs, cluster_rtol: float) -> Dict:
    """What :func:`profile_sensitivity_from_grams` returns, from the projected pencil ``(A, B)`` and its derivatives ``dA``,
    ``dB`` (n, k, k) along n parameters; ``dirs`` (n,) or None (shared with :mod:`.shape`)."""
    k, ntan = beta.size, dA.shape[0]
    s = 1.0 / np.sqrt(np.diag(B))                          # B-normalisation of every record
    A, B = (s[:, None] * X * s[None, :] for X in (A, B))
    dA, dB = (s[None, :, None] * X * s[None, None, :] for X in (dA, dB))
    res = {"rayleigh_defect": np.abs(np.diag(A) - mu) / np.abs(mu)}
    label = _clusters(mu, cluster_rtol * float(np.abs(mu).max()))
    res["cluster"] = label
    res["sensitivity"] = dA - mu[None, None, :] * dB
    members = _cluster_members(label)
    to_neff = sgn / (2.0 * beta * k0)
    cols = [_directional_dmu(dA[p], dB[p], B, mu, members) for p in range(ntan)]
    res["dneff_dp"] = (np.stack(cols, axis=1) if cols else np.zeros((k, 0))) * to_neff[:, None]
    if dirs is not None:
        res["dneff_direction"] = _directional_dmu(np.tensordot(dirs, dA, 1), np.tensordot(dirs, dB, 1), B, mu, members) * to_neff
    return res


def profile_bend_from_grams(kind: str, grams: Dict[str, np.ndarray], tangent_grams: Dict[str, np.ndarray],
                            moment_grams: Dict[str, np.ndarray], beta, k0: float, curvature=None, angle=0.0,
                            cluster_rtol: float = 1e-10, alpha_p: float = TrueVectorialMaxwellSolver.ALPHA_P) -> Dict:
    """The k x k host math of :func:`profile_bend_response`: a pure function of the Grams of the profile solve, of ``M_wX``,
    ``M_wY`` (and ``K_wX``, ``K_wY``) of ``ModeFields.profile_tangent_grams(..., moments=True)`` and of the unweighted moment
    Grams (``plfem_moment_grams`` names with no cores: ``M_clad_X``, ``M_clad_Y``, ``M_XX``, ``M_XY``, ``M_YY``; ``M_core_X`` and
    ``M_core_Y`` are added when present).  Vectorial: ``A1 = -2 K_wX/Y``, ``B1 = -2 M_wX/Y``; scalar: ``A1 = -2 k0^2 M_wX/Y``,
    ``B1 = 0``.  Returns what :func:`.bend.bend_quantities_from_grams` does."""
    kappa, ang = _curvature_and_angle(curvature, angle)
    _rtol(cluster_rtol)
    G, A, B, mu, sgn, beta = _pencil(kind, grams, beta, k0, alpha_p)
    k, k0 = beta.size, float(k0)
    names = ("M_wX", "M_wY") + (("K_wX", "K_wY") if kind == "vectorial" else ())
    T = dict(zip(names, _tangent_stack(kind, tangent_grams, names, k, lead=0)))
    need = ("M_clad_X", "M_clad_Y", "M_XX", "M_XY", "M_YY")
    if any(nm not in moment_grams for nm in need):
        raise ValueError(f"moment_grams must hold {', '.join(need)}")
    P = {nm: _sym(v) for nm, v in moment_grams.items()}
    if any(P[nm].shape != (k, k) for nm in need):
        raise ValueError("the moment Grams must be k x k with k = beta.size")
    MX = P["M_clad_X"] + P["M_core_X"] if "M_core_X" in P else P["M_clad_X"]
    MY = P["M_clad_Y"] + P["M_core_Y"] if "M_core_Y" in P else P["M_clad_Y"]
    if kind == "vectorial":
        A1 = np.stack([-2.0 * T["K_w" + a] for a in "XY"])
        B1 = np.stack([-2.0 * T["M_w" + a] for a in "XY"])
    else:
        A1 = np.stack([-2.0 * k0 * k0 * T["M_w" + a] for a in "XY"])
        B1 = np.zeros_like(A1)
    return _bend_from_pencil(kind, A, B, A1, B1, mu, sgn, beta, k0, G["M"], MX, MY, P["M_XX"], P["M_XY"], P["M_YY"], kappa, ang,
                             angle, cluster_rtol)


def _enter(what: str, modes, mesh, geometry, cluster_rtol, device):
    """The checks the three entry points share, before any device call: ``(kind, beta, profile, mf, vals)``."""
    profile = index_profile_of(geometry)
    if profile is None:
        raise ValueError(f"{what} needs a geometry that carries an index profile (ProfiledGeometry)")
    kind, _, beta = _records(modes)
    if kind is None:
        raise ValueError("no mode records")
    if not np.all(np.isfinite(beta) & (beta > 0)):
        raise ValueError("every record needs a finite, positive 'beta'")
    k0 = getattr(geometry, "k0", None)
    if k0 is None or not np.isfinite(float(k0)) or float(k0) <= 0:
        raise ValueError("geometry must have a finite, positive k0")
    _rtol(cluster_rtol)
    mf = mesh if isinstance(mesh, ModeFields) else ModeFields(mesh, device=device)
    _, vals, _ = mf._check_records(modes)                   # lengths, before the device
    return kind, beta, profile, mf, vals


def _profile_grams(mf, kind, staged, profile):
    return mf._profile_grams_staged(kind, staged, profile.table(), profile.eps_background, index_map=profile.index_map)


def profile_dispersion(modes: Sequence[Dict], mesh, geometry, dn_dlambda: Optional[ProfileTangent] = None,
                       cluster_rtol: float = 1e-10, device: Optional[int] = None) -> Dict:
    """Group quantities of the modes of a profile solve from one solve: :func:`.dispersion.mode_dispersion` for a
    :class:`.profile.ProfiledGeometry`.

    ``dn_dlambda``: the material dispersion as a tangent of the profile, ``profile.tangent_index(...)`` with ``dn / d
    lambda0`` in um^-1 in place of ``dn`` (background, every layer, centre and edge of a graded one, the map), or None: no
    material dispersion.  It is scaled by ``-lambda0 / k0`` (``d eps / d k0 = 2 n (-lambda0 / k0) dn/dlambda0``, as
    :func:`.dispersion.deps_dk0` does).  Returns the keys of ``mode_dispersion`` -- ``n_g``, ``group_delay_ps_per_m``,
    ``dmgd_ps_per_m``, ``coupling``, ``cluster``, ``cluster_rotation``, ``rayleigh_defect`` -- and ``grams``,
    ``tangent_grams``.  The modes are staged once; ``plfem_profile_grams`` and, with a tangent,
    ``plfem_profile_tangent_grams`` run on them.  Argument errors raise ``ValueError`` before any device call."""
    kind, beta, profile, mf, vals = _enter("profile_dispersion", modes, mesh, geometry, cluster_rtol, device)
    k0 = float(geometry.k0)
    tangent = None
    if dn_dlambda is not None:
        if not isinstance(dn_dlambda, ProfileTangent):
            raise ValueError("dn_dlambda must be a ProfileTangent of the geometry's profile (profile.tangent_index), or None")
        tangent = dn_dlambda.check(profile).scaled(-(2.0 * np.pi / k0) / k0)
    mf._ensure_locator()
    staged, _src = mf._stage(vals)
    grams = _profile_grams(mf, kind, staged, profile)
    tg = None if tangent is None else mf._profile_tangent_grams_staged(kind, staged, profile, [tangent], False, mf._origin((0.0, 0.0)))
    res = profile_dispersion_from_grams(kind, grams, tg, beta, k0, cluster_rtol)
    res.pop("dmu_dk0")
    res.update(grams=grams, tangent_grams=tg)
    return res


def profile_sensitivity(modes: Sequence[Dict], mesh, geometry, tangents=None, direction=None, cluster_rtol: float = 1e-10,
                        device: Optional[int] = None) -> Dict:
    """d n_eff of the modes of a profile solve per unit step along tangents of the profile, from one solve.

    ``tangents``: :class:`.profile.ProfileTangent` objects of the geometry's profile; default ``profile.unit_tangents()``,
    for which ``dneff_dp`` (k, ntan) is d n_eff / d n of the background (with the map) and of each layer in turn -- of the
    part of a layer that no later layer paints over.  See :func:`profile_sensitivity_from_grams` for every returned
    quantity; also returned: ``grams``, ``tangent_grams``.  Argument errors raise ``ValueError`` before any device call."""
    kind, beta, profile, mf, vals = _enter("profile_sensitivity", modes, mesh, geometry, cluster_rtol, device)
    tangents = mf._tangents(profile, profile.unit_tangents() if tangents is None else tangents)
    if not tangents:
        raise ValueError("no tangents")
    if direction is not None:
        try:
            d = np.asarray(direction, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"direction must be {len(tangents)} finite numbers, one per tangent") from None
        if d.size != len(tangents) or not np.all(np.isfinite(d)):
            raise ValueError(f"direction must be {len(tangents)} finite numbers, one per tangent")
    mf._ensure_locator()
    staged, _src = mf._stage(vals)
    grams = _profile_grams(mf, kind, staged, profile)
    tg = mf._profile_tangent_grams_staged(kind, staged, profile, tangents, False, mf._origin((0.0, 0.0)))
    res = profile_sensitivity_from_grams(kind, grams, tg, beta, float(geometry.k0), direction, cluster_rtol)
    res.update(grams=grams, tangent_grams=tg)
    return res


def profile_bend_response(modes: Sequence[Dict], mesh, geometry, radius=None, angle=0.0, origin=(0.0, 0.0),
                          cluster_rtol: float = 1e-10, device: Optional[int] = None) -> Dict:
    """What a bend does to the modes of a profile solve, from one solve: :func:`.bend.bend_response` for a
    :class:`.profile.ProfiledGeometry` -- the same arguments, the same keys (``dneff_dkappa``, ``coupling``, ``centroid``,
    ``second_moment``, ``width_d4sigma``, ``cluster``, ``rayleigh_defect``, ``pencil``, with ``radius`` ``n_eff_ritz``,
    ``beta_ritz``, ``mixing``), and ``grams``, ``tangent_grams``, ``moment_grams``.  The bent permittivity is ``eps (1 + 2 Xt /
    R)`` with the profile's eps at every point.  Centroids and widths come from ``plfem_moment_grams`` with no cores.  The
    ``pencil`` of scalar records feeds :func:`.bend.bend_propagate` unchanged."""
    kind, beta, profile, mf, vals = _enter("profile_bend_response", modes, mesh, geometry, cluster_rtol, device)
    o = ModeFields._origin(origin)
    kappa = None
    if radius is not None:
        try:
            r = np.asarray(radius, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("radius must be a non-zero number (numpy.inf: straight) or a 1-D array of them") from None
        if r.ndim > 1 or r.size == 0 or np.any(np.isnan(r)) or np.any(r == 0):
            raise ValueError("radius must be a non-zero number (numpy.inf: straight) or a 1-D array of them")
        kappa = 1.0 / r
    kap, ang = _curvature_and_angle(kappa, angle)
    if kap is not None:
        x0, x1, y0, y1 = mf.bbox
        corners = np.array([[x0, y0], [x0, y1], [x1, y0], [x1, y1]]) - o
        xt = np.abs(np.cos(ang)[:, None] * corners[None, :, 0] + np.sin(ang)[:, None] * corners[None, :, 1]).max(1)
        worst = 2.0 * np.abs(kap) * xt
        if np.any(worst >= 1.0):
            i = int(np.argmax(worst))
            raise ValueError(f"radius {1.0 / kap[i]:g} um: 2 |x| / R reaches {worst[i]:.3g} on the mesh, the bent permittivity "
                             "eps (1 + 2 x / R) would change sign")
    mf._ensure_locator()
    staged, _src = mf._stage(vals)
    grams = _profile_grams(mf, kind, staged, profile)
    tg = mf._profile_tangent_grams_staged(kind, staged, profile, [], True, o)
    mg = mf._moment_grams_staged(kind, staged, np.zeros((0, 3), dtype=np.float64), o)
    res = profile_bend_from_grams(kind, grams, tg, mg, beta, float(geometry.k0), kappa, angle, cluster_rtol)
    res.update(grams=grams, tangent_grams=tg, moment_grams=mg)
    return res


__all__ = ["profile_dispersion", "profile_dispersion_from_grams", "profile_sensitivity", "profile_sensitivity_from_grams",
           "profile_bend_response", "profile_bend_from_grams"]
