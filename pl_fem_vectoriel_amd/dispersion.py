"""Group index, modal group delay and k0-derivative mode coupling from one solve.

The discrete pencils of the two solvers depend on k0 explicitly and, with material dispersion, through eps_r(k0):

* vectorial (``TrueVectorialMaxwellSolver``): ``A h = mu B h``, ``mu = beta^2``, ``A = sum_r K_r / eps_r + alpha_p D -
  k0^2 (M_core + M_clad)``, ``B = sum_r M_r / eps_r``;
* scalar (``ScalarHelmholtzSolver``): ``A u = lambda B u``, ``lambda = -beta^2``, ``A = S - k0^2 sum_r eps_r M_r``,
  ``B = M_core + M_clad``.

With B-normalised modes, Hellmann-Feynman gives ``d mu_n / dk0 = h_n^T (A' - mu_n B') h_n`` and first-order perturbation
theory ``h_m^T B dh_n/dk0 = h_m^T (A' - mu_n B') h_n / (mu_n - mu_m)`` (m != n), ``-1/2 h_n^T B' h_n`` (m = n).  Every term
is a k x k Gram of the returned modes under the element forms of the assembly, split by region, which
:meth:`ModeFields.grams` computes on the GPU (``plfem_mode_grams``).  :func:`dispersion_from_grams` is the k x k host
math, a pure function of the Grams, so it can be fed Grams from anywhere.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import scipy.linalg

from .fields import ModeFields, _records
from .profile import reject_profile
from .solver_fem import TrueVectorialMaxwellSolver

C_M_PER_S = 299792458.0


def deps_dk0(n: float, k0: float, dn_dlambda: float) -> float:
    """d eps / d k0 of a material of index n with dn/d lambda0 (um^-1) at k0 (um^-1): ``2 n (-lambda0 / k0) dn/dlambda0``,
    lambda0 = 2 pi / k0; for bulk material this gives the textbook ``n_g = n - lambda0 dn/dlambda0``."""
    lam0 = 2.0 * np.pi / k0
    return 2.0 * n * (-lam0 / k0) * dn_dlambda


def _clusters(mu: np.ndarray, tol: float) -> np.ndarray:
    """Connected components of |mu_m - mu_n| <= tol (consecutive runs in sorted order); -1 for a singleton."""
    k = mu.size
    order = np.argsort(mu, kind="stable")
    label = np.full(k, -1, dtype=np.int64)
    runs, cur = [], [order[0]] if k else []
    for a, b in zip(order[:-1], order[1:]):
        if mu[b] - mu[a] <= tol:
            cur.append(b)
        else:
            runs.append(cur)
            cur = [b]
    if cur:
        runs.append(cur)
    members = sorted((sorted(int(i) for i in r) for r in runs if len(r) > 1), key=lambda r: r[0])
    for c, r in enumerate(members):
        label[r] = c
    return label


def dispersion_from_grams(kind: str, grams: Dict[str, np.ndarray], beta, k0: float, eps, deps=(0.0, 0.0),
                          cluster_rtol: float = 1e-10, alpha_p: float = TrueVectorialMaxwellSolver.ALPHA_P) -> Dict:
    """The k x k host math of :func:`mode_dispersion` from the region-split Grams (``ModeFields.grams`` names).
    ``eps`` = (eps_core, eps_clad), ``deps`` = their k0-derivatives; ``beta`` (k,) from the records: mu = beta^2
    (vectorial) or lambda = -beta^2 (scalar)."""
    if kind not in ("vectorial", "scalar"):
        raise ValueError("kind must be 'vectorial' or 'scalar'")
    G = {nm: 0.5 * (np.asarray(v, dtype=np.float64) + np.asarray(v, dtype=np.float64).T) for nm, v in grams.items()}
    beta = np.asarray(beta, dtype=np.float64)
    ec, el = float(eps[0]), float(eps[1])
    dc, dl = float(deps[0]), float(deps[1])
    Mc, Ml = G["M_core"], G["M_clad"]
    if kind == "vectorial":
        Kc, Kl = G["K_core"], G["K_clad"]
        A = Kc / ec + Kl / el + alpha_p * G["D"] - k0 * k0 * (Mc + Ml)
        B = Mc / ec + Ml / el
        Ad = -2.0 * k0 * (Mc + Ml) - (dc / ec ** 2) * Kc - (dl / el ** 2) * Kl
        Bd = -(dc / ec ** 2) * Mc - (dl / el ** 2) * Ml
        mu, sgn = beta ** 2, 1.0
    else:
        A = G["S"] - k0 * k0 * (ec * Mc + el * Ml)
        B = Mc + Ml
        Ad = -2.0 * k0 * (ec * Mc + el * Ml) - k0 * k0 * (dc * Mc + dl * Ml)
        Bd = np.zeros_like(B)
        mu, sgn = -beta ** 2, -1.0
    return _dispersion_from_pencil(A, B, Ad, Bd, mu, sgn, beta, cluster_rtol)


def _dispersion_from_pencil(A, B, Ad, Bd, mu, sgn, beta, cluster_rtol) -> Dict:
    """What :func:`dispersion_from_grams` makes of the projected pencil ``(A, B)`` of the records, its k0-derivative
    ``(Ad, Bd)`` and ``mu`` = ``sgn beta^2`` (shared with :mod:`.profile_response`)."""
    k = beta.size
    s = 1.0 / np.sqrt(np.diag(B))                          # B-normalisation of every record
    A, B, Ad, Bd = (s[:, None] * X * s[None, :] for X in (A, B, Ad, Bd))
    rayleigh = np.abs(np.diag(A) - mu) / np.abs(mu)
    label = _clusters(mu, cluster_rtol * float(np.abs(mu).max()))
    ncl = int(label.max()) + 1 if k else 0
    Q = np.eye(k)
    dmu = np.diag(Ad) - mu * np.diag(Bd)
    rotations = []
    for c in range(ncl):
        S = np.nonzero(label == c)[0]
        mbar = float(mu[S].mean())
        T = (Ad - mbar * Bd)[np.ix_(S, S)]
        w, Y = scipy.linalg.eigh(T, B[np.ix_(S, S)])       # Y^T B_SS Y = I: the adapted basis of the cluster
        dmu[S] = w
        Q[np.ix_(S, S)] = Y
        rotations.append(Y)
    if ncl:
        Ad, Bd = Q.T @ Ad @ Q, Q.T @ Bd @ Q
    Ad, Bd = 0.5 * (Ad + Ad.T), 0.5 * (Bd + Bd.T)          # (so that coupling is exactly antisymmetric when B' = 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        coup = (Ad - mu[None, :] * Bd) / (mu[None, :] - mu[:, None])
    same = (label[:, None] == label[None, :]) & (label[:, None] >= 0)
    coup[same] = 0.0
    coup[np.diag_indices(k)] = -0.5 * np.diag(Bd)
    n_g = sgn * dmu / (2.0 * beta)
    delay = n_g * 1e12 / C_M_PER_S
    return {"n_g": n_g, "group_delay_ps_per_m": delay, "dmgd_ps_per_m": float(delay.max() - delay.min()) if k else 0.0,
            "coupling": coup, "cluster": label, "cluster_rotation": rotations, "rayleigh_defect": rayleigh,
            "dmu_dk0": dmu}


def mode_dispersion(modes: Sequence[Dict], mesh, geometry, dn_dlambda=(0.0, 0.0), cluster_rtol: float = 1e-10,
                    device: Optional[int] = None) -> Dict:
    """Group quantities of the solver's modes from one solve.

    ``mesh`` is the mesh the modes were solved on (or its :class:`ModeFields`); ``geometry`` supplies k0, the cores and
    n_core / n_clad; ``dn_dlambda`` = (dn_core/dlambda0, dn_clad/dlambda0) in um^-1 (0: no material dispersion).
    Returns ``n_g`` (k,), ``group_delay_ps_per_m`` (= n_g 1e12 / c), ``dmgd_ps_per_m`` (max - min over the given modes),
    ``coupling`` (k, k) = h_m^T B dh_n/dk0 in um, ``cluster`` (k,) (-1 for a mode whose eigenvalue no other shares within
    ``cluster_rtol`` max|mu|), ``cluster_rotation`` (per cluster: the B-orthonormal combination of its members, in record
    order, that diagonalises the derivative; its columns are the modes that ``n_g`` and ``coupling`` refer to for those
    members; in-cluster coupling is 0), ``rayleigh_defect`` |h^T A h - mu| / |mu| (mu = beta^2 or -beta^2; the check that
    regions and forms match the solver's pencil) and ``grams``.  The records are not mutated.  Argument errors raise
    ``ValueError`` before any device call."""
    reject_profile(geometry, "mode_dispersion")
    kind, _, beta = _records(modes)
    if kind is None:
        raise ValueError("no mode records")
    if not np.all(np.isfinite(beta) & (beta > 0)):
        raise ValueError("every record needs a finite, positive 'beta'")
    if not all(hasattr(geometry, a) for a in ("positions", "core_radii", "n_core", "n_clad", "k0")):
        raise ValueError("geometry must have positions, core_radii, n_core, n_clad and k0")
    try:
        dn = np.asarray(dn_dlambda, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("dn_dlambda must be two finite numbers (dn_core/dlambda, dn_clad/dlambda)") from None
    if dn.size != 2 or not np.all(np.isfinite(dn)):
        raise ValueError("dn_dlambda must be two finite numbers (dn_core/dlambda, dn_clad/dlambda)")
    if not (np.isfinite(cluster_rtol) and cluster_rtol >= 0):
        raise ValueError("cluster_rtol must be finite and >= 0")
    if np.atleast_2d(np.asarray(geometry.positions)).shape[0] > 64:
        raise ValueError("at most 64 cores")
    mf = mesh if isinstance(mesh, ModeFields) else ModeFields(mesh, device=device)
    mf._check_records(modes)                                # lengths, before the device
    k0 = float(geometry.k0)
    nc, nl = float(geometry.n_core), float(geometry.n_clad)
    grams = mf.grams(modes, geometry)
    res = dispersion_from_grams(kind, grams, beta, k0, (nc * nc, nl * nl),
                                (deps_dk0(nc, k0, dn[0]), deps_dk0(nl, k0, dn[1])), cluster_rtol)
    res.pop("dmu_dk0")
    res["grams"] = grams
    return res


__all__ = ["mode_dispersion", "dispersion_from_grams", "deps_dk0"]
