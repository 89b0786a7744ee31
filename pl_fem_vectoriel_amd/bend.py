"""Bent fibres from one solve: index shifts, mode mixing and beam moments from coordinate-weighted Grams (DESIGN.md
section 20).

To first order in the curvature ``kappa = 1 / R`` a bend is the conformal map ``eps -> eps (1 + 2 kappa Xt)`` with ``Xt
= c X + s Y`` the coordinate along the bend direction ``(c, s) = (cos angle, sin angle)``, which points away from the
centre of curvature; ``X = x - origin[0]``, ``Y = y - origin[1]``.  Both discrete pencils (:mod:`.dispersion` for the
forms) are linear in the per-point material constant, so they are linear in kappa:

* scalar: ``A(kappa) = A - 2 kappa k0^2 sum_r eps_r (c M_r_X + s M_r_Y)``, ``B = M``;
* vectorial: ``1/eps -> (1 - 2 kappa Xt) / eps``, so ``A(kappa) = A - 2 kappa sum_r (c K_r_X + s K_r_Y) / eps_r`` and
  ``B(kappa) = B - 2 kappa sum_r (c M_r_X + s M_r_Y) / eps_r``; ``D`` and the unweighted ``M`` carry no eps and stay.

Projected on the computed modes these are k x k matrices made of the region Grams (:meth:`ModeFields.grams`) and the
coordinate-weighted Grams (:meth:`ModeFields.moment_grams`), both computed on the GPU; the projection of the bent pencil
is exact, and everything here is k x k host math on it.  Nothing is assembled, factorised or solved again.

Lengths are in um, curvatures in 1 / um.  ``R`` is the radius that enters the index profile: the elasto-optic correction
(an effective radius of about 1.28 R for silica) is the caller's business.  The vectorial numbers describe the
reference's pencil as it is ("What the vectorial numbers mean").
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import scipy.linalg

from .cores import _cluster_members, _directional_dmu, _sym
from .dispersion import _clusters
from .fields import ModeFields, _records
from .profile import reject_profile
from .solver_fem import TrueVectorialMaxwellSolver


def _curvature_and_angle(curvature, angle):
    """(kappa (nR,), angle (nR,)) broadcast against each other, or (None, angle scalar); ``ValueError`` otherwise."""
    try:
        ang = np.asarray(angle, dtype=np.float64)
        kap = None if curvature is None else np.asarray(curvature, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("curvature and angle must be finite numbers or 1-D arrays of them") from None
    if ang.ndim > 1 or not np.all(np.isfinite(ang)):
        raise ValueError("angle must be a finite number or a 1-D array of finite numbers")
    if kap is None:
        if ang.ndim != 0:
            raise ValueError("angle must be one number when no curvature is given")
        return None, ang
    if kap.ndim > 1 or kap.size == 0 or not np.all(np.isfinite(kap)):
        raise ValueError("curvature must be a finite number or a non-empty 1-D array of finite numbers")
    try:
        kap, ang = np.broadcast_arrays(np.atleast_1d(kap), np.atleast_1d(ang))
    except ValueError:
        raise ValueError("angle does not broadcast against the curvatures") from None
    return kap.copy(), ang.copy()


def bend_quantities_from_grams(kind: str, moment_grams: Dict[str, np.ndarray], grams: Dict[str, np.ndarray], beta, k0: float,
                               eps, curvature=None, angle=0.0, cluster_rtol: float = 1e-10,
                               alpha_p: float = TrueVectorialMaxwellSolver.ALPHA_P) -> Dict:
    """The k x k host math of :func:`bend_response`: a pure function of the coordinate-weighted Grams
    (``ModeFields.moment_grams`` names, each (k, k)) and the region Grams (``ModeFields.grams`` names).  ``eps`` =
    (eps_core, eps_clad), the permittivities the modes were solved with; ``beta`` (k,) from the records; ``curvature``
    in 1 / um, ``angle`` in rad.  Coordinates are those of the moment Grams, that is relative to their origin.

    Returns ``centroid`` (k, 2), the mean of (X, Y) under the weight ``|u_m|^2``; ``second_moment`` (k, 2, 2), central;
    ``width_d4sigma`` (k, 2), four times the standard deviation along the major and the minor principal axis (2 w for
    a Gaussian field exp(-r^2 / w^2)); ``coupling`` (2, k, k) = ``C_x``, ``C_y`` with ``C[m, n] = h_m^T (A_1 - mu_n B_1) h_n``
    between B-normalised records, ``A_1``, ``B_1`` the derivative of the pencil with respect to the curvature of a bend
    along x or y (the diagonal is d mu_n / d kappa of a non-degenerate mode, ``C[m, n] / (mu_n - mu_m)`` the first-order
    admixture ``h_m^T B dh_n/dkappa``); ``dneff_dkappa`` (k,) in um, along ``angle`` (one row per angle when ``angle`` is an
    array); ``cluster`` (k,) as in
    :func:`.dispersion.mode_dispersion`; ``rayleigh_defect`` (k,) ``|h^T A h - mu| / |mu|``; ``pencil``, the projected
    pencil on the B-normalised records that :func:`bend_propagate` takes (``A``, ``B``, ``A1`` and ``B1`` (2, k, k), ``kind``,
    ``k0``, ``scale`` (k,) = the factor that B-normalises each record).

    Degenerate clusters: the derivative of a repeated eigenvalue is a property of the cluster, not of one record.
    Inside a cluster ``dneff_dkappa`` holds the generalised eigenvalues of ``c C_x + s C_y`` on the cluster block,
    handed out in ascending order of d mu to the members in record order, as :func:`.cores.core_quantities_from_grams`
    does for an index direction.

    ``curvature`` (a number or (nR,); ``angle`` broadcasts against it): also ``n_eff_ritz`` (nR, k), descending, the
    Rayleigh-Ritz values of the bent pencil in the span of the given modes, ``beta_ritz`` and ``mixing`` (nR, k, k), column
    j = the j-th Ritz vector on the B-normalised records.  The projected pencil is exact; the span is not the bent
    eigenspace, so the values are variational estimates with an error of second order in the curvature (NaN for a Ritz
    value past cut-off, beta^2 <= 0).  ``ValueError`` when the bent ``B`` is no longer positive definite: the bent
    permittivity has changed sign inside the section."""
    if kind not in ("vectorial", "scalar"):
        raise ValueError("kind must be 'vectorial' or 'scalar'")
    kappa, ang = _curvature_and_angle(curvature, angle)
    if not (np.isfinite(cluster_rtol) and cluster_rtol >= 0):
        raise ValueError("cluster_rtol must be finite and >= 0")
    G = {nm: _sym(v) for nm, v in grams.items()}
    P = {nm: _sym(v) for nm, v in moment_grams.items()}
    beta = np.asarray(beta, dtype=np.float64).reshape(-1)
    k = beta.size
    k0 = float(k0)
    ec, el = float(eps[0]), float(eps[1])
    need = ("M_core_X", "M_core_Y", "M_clad_X", "M_clad_Y", "M_XX", "M_XY", "M_YY")
    need += ("K_core_X", "K_core_Y", "K_clad_X", "K_clad_Y") if kind == "vectorial" else ()
    if any(nm not in P for nm in need):
        raise ValueError(f"moment_grams must hold {', '.join(need)}")
    Mc, Ml = G["M_core"], G["M_clad"]
    M = Mc + Ml
    if k < 1 or M.shape != (k, k) or any(P[nm].shape != (k, k) for nm in need):
        raise ValueError("the Grams must be k x k with k = beta.size >= 1")
    if kind == "vectorial":
        A = G["K_core"] / ec + G["K_clad"] / el + alpha_p * G["D"] - k0 * k0 * M
        B = Mc / ec + Ml / el
        A1 = np.stack([-2.0 * (P["K_core_" + a] / ec + P["K_clad_" + a] / el) for a in "XY"])
        B1 = np.stack([-2.0 * (P["M_core_" + a] / ec + P["M_clad_" + a] / el) for a in "XY"])
        mu, sgn = beta ** 2, 1.0
    else:
        A = G["S"] - k0 * k0 * (ec * Mc + el * Ml)
        B = M
        A1 = np.stack([-2.0 * k0 * k0 * (ec * P["M_core_" + a] + el * P["M_clad_" + a]) for a in "XY"])
        B1 = np.zeros_like(A1)
        mu, sgn = -beta ** 2, -1.0

    return _bend_from_pencil(kind, A, B, A1, B1, mu, sgn, beta, k0, M, P["M_core_X"] + P["M_clad_X"], P["M_core_Y"] + P["M_clad_Y"],
                             P["M_XX"], P["M_XY"], P["M_YY"], kappa, ang, angle, cluster_rtol)


def _bend_from_pencil(kind, A, B, A1, B1, mu, sgn, beta, k0, M, MX, MY, MXX, MXY, MYY, kappa, ang, angle, cluster_rtol) -> Dict:
    """What :func:`bend_quantities_from_grams` makes of the projected pencil ``(A, B)`` of the records, its curvature
    derivatives ``A1``, ``B1`` (2, k, k) and the unweighted Grams ``M``, ``MX`` .. ``MYY`` of the beam moments; ``kappa``,
    ``ang`` from :func:`_curvature_and_angle` (shared with :mod:`.profile_response`)."""
    k = beta.size
    dm = np.diag(M)
    cx = np.diag(MX) / dm
    cy = np.diag(MY) / dm
    sxx, sxy, syy = np.diag(MXX) / dm - cx * cx, np.diag(MXY) / dm - cx * cy, np.diag(MYY) / dm - cy * cy
    second = np.stack([np.stack([sxx, sxy], -1), np.stack([sxy, syy], -1)], -2)
    res = {"centroid": np.stack([cx, cy], -1), "second_moment": second,
           "width_d4sigma": 4.0 * np.sqrt(np.maximum(np.linalg.eigvalsh(second)[:, ::-1], 0.0))}

    s = 1.0 / np.sqrt(np.diag(B))                          # B-normalisation of every record
    A, B = (s[:, None] * X * s[None, :] for X in (A, B))
    A1, B1 = (s[None, :, None] * X * s[None, None, :] for X in (A1, B1))
    res["rayleigh_defect"] = np.abs(np.diag(A) - mu) / np.abs(mu)
    label = _clusters(mu, cluster_rtol * float(np.abs(mu).max()))
    res["cluster"] = label
    res["coupling"] = A1 - mu[None, None, :] * B1
    members = _cluster_members(label)
    dirs = np.asarray(angle, dtype=np.float64)               # one number: (k,); an array: one row per angle
    dmu = np.array([_directional_dmu(np.cos(a) * A1[0] + np.sin(a) * A1[1], np.cos(a) * B1[0] + np.sin(a) * B1[1], B, mu, members)
                    for a in dirs.reshape(-1)])
    res["dneff_dkappa"] = (sgn * dmu / (2.0 * beta * k0)[None, :]).reshape(dirs.shape + (k,))
    res["pencil"] = {"kind": kind, "k0": k0, "A": A, "B": B, "A1": A1, "B1": B1, "scale": s}
    if kappa is not None:
        nR = kappa.size
        br, mix = np.empty((nR, k)), np.empty((nR, k, k))
        for i, (kp, a) in enumerate(zip(kappa, ang)):
            c, sn = np.cos(a), np.sin(a)
            A2 = A + kp * (c * A1[0] + sn * A1[1])
            B2 = B + kp * (c * B1[0] + sn * B1[1])
            try:
                w, Y = scipy.linalg.eigh(0.5 * (A2 + A2.T), 0.5 * (B2 + B2.T))
            except np.linalg.LinAlgError:
                raise ValueError(f"curvature {kp:g} / um: the bent B is not positive definite (the bent permittivity "
                                 "changes sign inside the section)") from None
            b2 = sgn * w
            order = np.argsort(-b2, kind="stable")
            with np.errstate(invalid="ignore"):
                br[i] = np.sqrt(np.where(b2 > 0, b2, np.nan))[order]
            mix[i] = Y[:, order]
        res.update(beta_ritz=br, n_eff_ritz=br / k0, mixing=mix)
    return res


def bend_response(modes: Sequence[Dict], mesh, geometry, radius=None, angle=0.0, origin=(0.0, 0.0), cluster_rtol: float = 1e-10,
                  device: Optional[int] = None) -> Dict:
    """What a bend of radius ``radius`` (um) does to the solver's modes, from one solve: ``d n_eff / d kappa``, the bend
    coupling between the modes, Rayleigh-Ritz effective indices and mode mixing of the bent fibre, and the centroids
    and D4-sigma widths of the straight modes.

    ``mesh`` is the mesh the modes were solved on (or its :class:`ModeFields`); ``geometry`` supplies k0, the core discs
    and n_core / n_clad the modes were solved with.  ``angle`` (rad) is the direction, in the cross-section, that points
    away from the centre of curvature; ``origin`` is the point of the cross-section on the bend's neutral axis, where the
    index is left as it is (coordinates, ``centroid`` included, are relative to it).  ``radius`` is None (derivatives
    only), a number or an (nR,) array, ``angle`` broadcasting against it; ``numpy.inf`` is the straight fibre.  It is the
    radius that enters the index profile ``eps (1 + 2 Xt / R)``: an effective radius for the elasto-optic effect is the
    caller's business.

    The modes are staged on the device once; ``plfem_mode_grams`` and ``plfem_moment_grams`` run on them, and
    :func:`bend_quantities_from_grams` (see there for every returned quantity, for what the values mean inside a
    degenerate cluster, and for the variational nature of ``n_eff_ritz``) does the k x k host math.  Also returned:
    ``grams`` and ``moment_grams``.  ``ValueError`` when ``2 |kappa| max |Xt|`` over the mesh's bounding box reaches 1: the
    first-order bent permittivity would change sign inside the section.  The records are not mutated.  Argument errors
    raise ``ValueError`` before any device call."""
    reject_profile(geometry, "bend_response")
    kind, _, beta = _records(modes)
    if kind is None:
        raise ValueError("no mode records")
    if not np.all(np.isfinite(beta) & (beta > 0)):
        raise ValueError("every record needs a finite, positive 'beta'")
    if not all(hasattr(geometry, a) for a in ("positions", "core_radii", "n_core", "n_clad", "k0")):
        raise ValueError("geometry must have positions, core_radii, n_core, n_clad and k0")
    cores = ModeFields._cores(geometry)
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
    if not (np.isfinite(cluster_rtol) and cluster_rtol >= 0):
        raise ValueError("cluster_rtol must be finite and >= 0")
    mf = mesh if isinstance(mesh, ModeFields) else ModeFields(mesh, device=device)
    _, vals, _ = mf._check_records(modes)                   # lengths, before the device
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
    grams = mf._grams_staged(kind, staged, cores)
    mg = mf._moment_grams_staged(kind, staged, cores, o)
    nc, nl = float(geometry.n_core), float(geometry.n_clad)
    res = bend_quantities_from_grams(kind, mg, grams, beta, float(geometry.k0), (nc * nc, nl * nl), kappa, angle,
                                     cluster_rtol)
    res.update(grams=grams, moment_grams=mg)
    return res


def bend_propagate(response_or_grams: Dict, segments) -> Dict:
    """Amplitudes of the straight modes along a path of bent segments, for scalar records.

    ``response_or_grams``: what :func:`bend_response` or :func:`bend_quantities_from_grams` returned (its ``pencil``).
    ``segments`` (nseg, 3): length (um), curvature (1 / um; 0 is straight) and angle (rad) of each segment, in the order
    the light meets them.  In a segment the field is expanded in the Ritz modes of that segment's projected pencil,
    ``Y_j^T B Y_j = I``, each advancing by ``exp(-i beta_j L_j)``: ``T_j = Y_j diag(exp(-i beta_j L_j)) Y_j^T B`` acts on the
    amplitudes ``a`` of the B-normalised straight records (record m times ``pencil["scale"][m]``), and ``transfer`` is the
    ordered product ``T_nseg ... T_1``.  Every ``T_j`` is B-unitary, ``T^H B T = B``: the projected model has no loss, so
    bend loss is not in it.  Returns ``transfer`` (k, k) complex, ``segment_transfer`` (nseg, k, k) and ``beta`` (nseg, k)
    descending.

    With the per-core Grams of :meth:`ModeFields.core_grams`, scaled as the amplitudes are (``M_c[m, n] scale[m]
    scale[n]``, likewise ``M = M_core + M_clad``), the share of the power in core c after the path is ``a^H M_c a / a^H M a``
    with ``a = transfer @ a_in``: the bend-induced crosstalk.

    ``ValueError`` for vectorial records (``B`` moves with the bend there, so the segments have no common inner
    product), for a segment with a Ritz value past cut-off (named), and for malformed ``segments``."""
    pencil = response_or_grams.get("pencil") if hasattr(response_or_grams, "get") else None
    if not hasattr(pencil, "get") or any(nm not in pencil for nm in ("kind", "A", "B", "A1")):
        raise ValueError("bend_propagate takes the result of bend_response or bend_quantities_from_grams")
    if pencil["kind"] != "scalar":
        raise ValueError("bend_propagate is for scalar records: the vectorial B changes with the bend")
    try:
        seg = np.asarray(segments, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("segments must be an array of shape (nseg, 3): length, curvature, angle") from None
    if seg.ndim != 2 or seg.shape[1] != 3 or not np.all(np.isfinite(seg)) or np.any(seg[:, 0] < 0):
        raise ValueError("segments must be a finite array of shape (nseg, 3): length >= 0, curvature, angle")
    A, B, A1 = pencil["A"], pencil["B"], pencil["A1"]
    k = A.shape[0]
    T = np.eye(k, dtype=np.complex128)
    each, betas = np.empty((seg.shape[0], k, k), dtype=np.complex128), np.empty((seg.shape[0], k))
    for j, (length, kp, a) in enumerate(seg):
        A2 = A + kp * (np.cos(a) * A1[0] + np.sin(a) * A1[1])
        w, Y = scipy.linalg.eigh(0.5 * (A2 + A2.T), 0.5 * (B + B.T))
        if np.any(w >= 0):
            raise ValueError(f"segment {j} (curvature {kp:g} / um): a Ritz value is past cut-off (beta^2 <= 0)")
        b = np.sqrt(-w)
        each[j] = (Y * np.exp(-1j * b * length)[None, :]) @ (Y.T @ B)
        betas[j] = b
        T = each[j] @ T
    return {"transfer": T, "segment_transfer": each, "beta": betas}


__all__ = ["bend_response", "bend_quantities_from_grams", "bend_propagate"]
