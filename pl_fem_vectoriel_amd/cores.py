"""Which core carries what: core power, per-core index sensitivity and unequal cores from one solve.

Both discrete pencils are linear in a per-region material constant (:mod:`.dispersion` for the forms):

* vectorial: ``A = sum_r K_r / eps_r + alpha_p D - k0^2 M``, ``B = sum_r M_r / eps_r``, ``mu = beta^2``;
* scalar: ``A = S - k0^2 sum_r eps_r M_r``, ``B = M``, ``lambda = -beta^2``.

Splitting the region "core" into its discs, ``K_core = sum_c K_c`` and ``M_core = sum_c M_c`` (``M_c = Mx_c + My_c`` for
vectorial records), gives for core c at index n_c the pencil ``A + sum_c (1/n_c^2 - 1/n_core^2) K_c``, ``B + sum_c (1/n_c^2
- 1/n_core^2) M_c`` (vectorial) or ``A - k0^2 sum_c (n_c^2 - n_core^2) M_c``, ``B`` (scalar).  Projected on the computed modes
these are k x k matrices made of the region Grams (:meth:`ModeFields.grams`) and the per-core Grams
(:meth:`ModeFields.core_grams`), both computed on the GPU; everything here is k x k host math on them.  Nothing is
assembled, factorised or solved again.

* power map: ``power[m, c] = M_c[m, m] / M[m, m]``, the share of mode m's ``int |u|^2`` in core c;
* Hellmann-Feynman: ``d mu_n / d n_c = h_n^T (dA/dn_c - mu_n dB/dn_c) h_n / (h_n^T B h_n)`` with ``dA/dn_c = -(2 n_c /
  eps_c^2) K_c``, ``dB/dn_c = -(2 n_c / eps_c^2) M_c`` (vectorial) or ``dA/dn_c = -2 n_c k0^2 M_c``, ``dB/dn_c = 0``
  (scalar), and ``d n_eff = +-d mu / (2 beta k0)``; for scalar records that is ``(n_c / n_eff) power[m, c]``;
* unequal cores: Rayleigh-Ritz with the exact projected pencil in the span of the given modes.

The vectorial numbers describe the reference's pencil as it is ("What the vectorial numbers mean").
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import scipy.linalg

from .dispersion import _clusters
from .fields import ModeFields, _records
from .profile import reject_profile
from .solver_fem import TrueVectorialMaxwellSolver


def _sym(v) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64)
    return 0.5 * (v + np.swapaxes(v, -1, -2))


def _vector(v, n: int, name: str, positive: bool = False) -> np.ndarray:
    try:
        a = np.asarray(v, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be {n} finite numbers, one per core") from None
    if a.size != n or not np.all(np.isfinite(a)) or (positive and np.any(a <= 0)):
        raise ValueError(f"{name} must be {n} finite{' positive' if positive else ''} numbers, one per core")
    return a


def _cluster_members(label: np.ndarray) -> list:
    """The index sets of the clusters of :func:`.dispersion._clusters` labels, in label order."""
    return [np.nonzero(label == c)[0] for c in range(int(label.max()) + 1 if label.size else 0)]


def _directional_dmu(Ad: np.ndarray, Bd: np.ndarray, B: np.ndarray, mu: np.ndarray, members: list) -> np.ndarray:
    """d mu of every B-normalised record along a direction in which the pencil moves by (Ad, Bd): Hellmann-Feynman for
    a singleton; inside a cluster the generalised eigenvalues of the cluster block against ``B_SS``, handed out in
    ascending order to the members in record order (shared with :mod:`.bend`)."""
    dmu = np.diag(Ad) - mu * np.diag(Bd)
    for S in members:
        T = (Ad - float(mu[S].mean()) * Bd)[np.ix_(S, S)]
        dmu[S] = scipy.linalg.eigh(0.5 * (T + T.T), B[np.ix_(S, S)], eigvals_only=True)
    return dmu


def core_quantities_from_grams(kind: str, core_grams: Dict[str, np.ndarray], grams: Dict[str, np.ndarray], beta, k0: float,
                               eps, n_cores=None, direction=None, cluster_rtol: float = 1e-10,
                               alpha_p: float = TrueVectorialMaxwellSolver.ALPHA_P) -> Dict:
    """The k x k host math of :func:`core_decomposition`: a pure function of the per-core Grams (``ModeFields.core_grams``
    names, each (ncore, k, k)) and the region Grams (``ModeFields.grams`` names).  ``eps`` = (eps_core, eps_clad), the
    permittivities the modes were solved with (every core at eps_core); ``beta`` (k,) from the records.

    Returns ``power`` (k, ncore), ``power_clad`` (k,); for vectorial records ``power_x``, ``power_y`` (the hx and hy
    shares of ``power``) and ``pdl_db`` (k, ncore) = ``clip(10 log10(max / min), 0, 50)`` of ``power_x + 1e-30`` and
    ``power_y + 1e-30``, the reference's per-mode formula applied core by core; ``dneff_dn`` (k, ncore), d n_eff of
    mode m per unit index change of core c; ``sensitivity`` (ncore, k, k), ``S_c[m, n] = h_m^T (dA/dn_c - mu_n dB/dn_c)
    h_n`` between B-normalised records (the diagonal is d mu_n / d n_c of a non-degenerate mode, ``S_c[m, n] / (mu_n -
    mu_m)`` the first-order admixture ``h_m^T B dh_n/dn_c``); ``cluster`` (k,) as in :func:`.dispersion.mode_dispersion`;
    ``rayleigh_defect`` (k,) ``|h^T A h - mu| / |mu|``.

    Degenerate clusters: the derivative of a repeated eigenvalue along a direction ``n_c = n_core + t d_c`` is not a
    property of one record but of the cluster: the generalised eigenvalues of ``sum_c d_c S_c`` on the cluster block
    against ``V_S^T B V_S``.  They are handed out in ascending order of d mu to the cluster's members in record order.
    Every column c of ``dneff_dn`` is such a derivative along ``e_c``, so inside a cluster its entries are cluster
    values, not per-record ones, and the columns of different cores belong to different adapted bases.

    ``direction`` (ncore,): also ``dneff_direction`` (k,), the derivative along ``n_c = n_core + t direction_c`` (for a
    mode outside every cluster this is ``dneff_dn @ direction``).

    ``n_cores`` (ncore,): also ``n_eff_ritz`` (k,), descending, the Rayleigh-Ritz values of the pencil with core c at index
    ``n_cores[c]`` in the span of the given modes, ``beta_ritz`` and ``mixing`` (k, k), column j = the j-th Ritz vector
    on the B-normalised records (orthonormal in the new B).  The projected pencil is exact; the span is not the new
    eigenspace, so the values are variational estimates with an error of second order in the index offsets (NaN for a
    Ritz value past cut-off, beta^2 <= 0).  Nothing is solved again."""
    if kind not in ("vectorial", "scalar"):
        raise ValueError("kind must be 'vectorial' or 'scalar'")
    G = {nm: _sym(v) for nm, v in grams.items()}
    C = {nm: _sym(v) for nm, v in core_grams.items() if nm != "points"}
    beta = np.asarray(beta, dtype=np.float64)
    k = beta.size
    ec, el = float(eps[0]), float(eps[1])
    n_core = float(np.sqrt(ec))
    Mc, Ml = G["M_core"], G["M_clad"]
    M = Mc + Ml
    if kind == "vectorial":
        Mcc = C["Mx"] + C["My"]
        A = G["K_core"] / ec + G["K_clad"] / el + alpha_p * G["D"] - k0 * k0 * M
        B = Mc / ec + Ml / el
        f = -2.0 * n_core / ec ** 2
        dA, dB = f * C["K"], f * Mcc
        mu, sgn = beta ** 2, 1.0
    else:
        Mcc = C["M"]
        A = G["S"] - k0 * k0 * (ec * Mc + el * Ml)
        B = M
        dA, dB = -2.0 * n_core * k0 * k0 * Mcc, np.zeros_like(Mcc)
        mu, sgn = -beta ** 2, -1.0
    ncore = Mcc.shape[0]
    if Mcc.shape[1:] != (k, k) or M.shape != (k, k):
        raise ValueError("the Grams must be k x k with k = beta.size")
    dirs = None if direction is None else _vector(direction, ncore, "direction")
    new_n = None if n_cores is None else _vector(n_cores, ncore, "n_cores", positive=True)

    dm = np.diag(M)
    idx = np.arange(k)
    res = {"power": (Mcc[:, idx, idx] / dm[None]).T, "power_clad": np.diag(Ml) / dm}
    if kind == "vectorial":
        px, py = (C["Mx"][:, idx, idx] / dm[None]).T, (C["My"][:, idx, idx] / dm[None]).T
        qx, qy = px + 1e-30, py + 1e-30
        res.update(power_x=px, power_y=py,
                   pdl_db=np.clip(10.0 * np.log10(np.maximum(qx, qy) / np.minimum(qx, qy)), 0.0, 50.0))

    s = 1.0 / np.sqrt(np.diag(B))                          # B-normalisation of every record
    A, B = (s[:, None] * X * s[None, :] for X in (A, B))
    dA, dB = (s[None, :, None] * X * s[None, None, :] for X in (dA, dB))
    res["rayleigh_defect"] = np.abs(np.diag(A) - mu) / np.abs(mu)
    label = _clusters(mu, cluster_rtol * float(np.abs(mu).max()))
    res["cluster"] = label
    res["sensitivity"] = dA - mu[None, None, :] * dB
    members = _cluster_members(label)

    def along(d):
        """d mu of every mode along the direction d (ncore,)."""
        return _directional_dmu(np.tensordot(d, dA, 1), np.tensordot(d, dB, 1), B, mu, members)

    to_neff = sgn / (2.0 * beta * k0)
    res["dneff_dn"] = np.stack([along(e) for e in np.eye(ncore)], axis=1) * to_neff[:, None]
    if dirs is not None:
        res["dneff_direction"] = along(dirs) * to_neff
    if new_n is not None:
        if kind == "vectorial":
            c = 1.0 / new_n ** 2 - 1.0 / ec
            A2 = A + np.tensordot(c, s[None, :, None] * C["K"] * s[None, None, :], 1)
            B2 = B + np.tensordot(c, s[None, :, None] * Mcc * s[None, None, :], 1)
        else:
            A2 = A - k0 * k0 * np.tensordot(new_n ** 2 - ec, s[None, :, None] * Mcc * s[None, None, :], 1)
            B2 = B
        w, Y = scipy.linalg.eigh(0.5 * (A2 + A2.T), 0.5 * (B2 + B2.T))
        b2 = sgn * w
        order = np.argsort(-b2, kind="stable")
        with np.errstate(invalid="ignore"):
            br = np.sqrt(np.where(b2 > 0, b2, np.nan))[order]
        res.update(beta_ritz=br, n_eff_ritz=br / k0, mixing=Y[:, order])
    return res


def core_decomposition(modes: Sequence[Dict], mesh, geometry, n_cores=None, direction=None, cluster_rtol: float = 1e-10,
                       device: Optional[int] = None) -> Dict:
    """Supermode-to-core power map, per-core index sensitivity and unequal-core estimates of the solver's modes.

    ``mesh`` is the mesh the modes were solved on (or its :class:`ModeFields`); ``geometry`` supplies k0, the core discs
    and n_core / n_clad the modes were solved with.  The modes are staged on the device once; ``plfem_mode_grams`` and
    ``plfem_core_grams`` run on them, and :func:`core_quantities_from_grams` (see there for every returned quantity,
    for what the values mean inside a degenerate cluster, and for the variational nature of ``n_eff_ritz``) does the
    k x k host math.  Also returned: ``points`` (ncore,) the quadrature points each core owns (a point in several discs
    belongs to the highest-index one, as in the reference's ``epsilon``), ``grams`` and ``core_grams``.  The records are
    not mutated.  Argument errors raise ``ValueError`` before any device call."""
    reject_profile(geometry, "core_decomposition")
    kind, _, beta = _records(modes)
    if kind is None:
        raise ValueError("no mode records")
    if not np.all(np.isfinite(beta) & (beta > 0)):
        raise ValueError("every record needs a finite, positive 'beta'")
    if not all(hasattr(geometry, a) for a in ("positions", "core_radii", "n_core", "n_clad", "k0")):
        raise ValueError("geometry must have positions, core_radii, n_core, n_clad and k0")
    cores = ModeFields._cores(geometry)
    ncore = cores.shape[0]
    if ncore < 1:
        raise ValueError("geometry has no cores")
    if n_cores is not None:
        _vector(n_cores, ncore, "n_cores", positive=True)
    if direction is not None:
        _vector(direction, ncore, "direction")
    if not (np.isfinite(cluster_rtol) and cluster_rtol >= 0):
        raise ValueError("cluster_rtol must be finite and >= 0")
    mf = mesh if isinstance(mesh, ModeFields) else ModeFields(mesh, device=device)
    _, vals, _ = mf._check_records(modes)                   # lengths, before the device
    mf._ensure_locator()
    staged, _src = mf._stage(vals)
    grams = mf._grams_staged(kind, staged, cores)
    cg = mf._core_grams_staged(kind, staged, cores)
    k0 = float(geometry.k0)
    nc, nl = float(geometry.n_core), float(geometry.n_clad)
    res = core_quantities_from_grams(kind, cg, grams, beta, k0, (nc * nc, nl * nl), n_cores, direction, cluster_rtol)
    res.update(points=cg["points"], grams=grams, core_grams=cg)
    return res


__all__ = ["core_decomposition", "core_quantities_from_grams"]
