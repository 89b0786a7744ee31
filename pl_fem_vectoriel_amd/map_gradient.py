"""Gradient of every n_eff in every pixel of a sampled index map, from one solve.

A profile over a sampled map (``IndexProfile.sampled``) is linear in the permittivity of every pixel, through the bilinear
hat of the pixel.  By Hellmann-Feynman the derivative of an eigenvalue of the pencils of :mod:`.profile_response` in one
pixel is a sum over the quadrature points under that hat, and the derivative in ALL pixels is one pass over the
quadrature points scattered through the adjoint of the interpolant: :meth:`ModeFields.index_map_densities`
(``plfem_index_map_gradients``).  What is left is a division per mode:

* vectorial: ``mu = beta^2``, ``N_r = M_w[r, r]``, ``d mu_r / dE = (K_px[r] - mu_r M_px[r]) / N_r``,
  ``d n_eff / d eps = d mu / (2 beta k0)``;
* scalar: ``lambda = -beta^2``, ``N_r = M[r, r]``, ``d lambda_r / dE = -k0^2 M_px[r] / N_r``,
  ``d n_eff / d eps = -d lambda / (2 beta k0)``,

the sign conventions of ``profile_response._pencil``.  The gradient feeds surrogate models, inverse design and the
refinement of measured or generated index maps; no optimiser is part of this package.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from .cores import _cluster_members
from .dispersion import _clusters
from .profile_response import _enter, _profile_grams, _rtol


def index_map_gradient_from_densities(kind: str, grams: Dict[str, np.ndarray], densities: Dict[str, np.ndarray], beta,
                                      k0: float, n_map, cluster_rtol: float = 1e-10) -> Dict:
    """The host math of :func:`index_map_gradient`: a pure function of the Grams of the profile solve
    (``ModeFields.profile_grams`` names: ``M_w`` for vectorial records, ``M`` for scalar ones), of the pixel densities
    (``ModeFields.index_map_densities`` names) of the same records, of ``beta`` (k,), ``k0`` and the map of indices
    ``n_map`` (ny, nx).

    Returns ``dneff_deps`` (k, ny, nx), d n_eff of every mode per unit permittivity of every pixel; ``dneff_dn`` = ``2 n_map
    dneff_deps``, per unit index; ``cluster`` (k,), the labels of ``dispersion._clusters`` under ``cluster_rtol`` (-1: a mode
    on its own); ``dneff_deps_cluster``, ``dneff_dn_cluster``: the mean over the mode's cluster, handed to every member --
    inside a degenerate cluster the single derivatives depend on the basis the solver happened to return, their mean does
    not --; ``support`` (ny, nx) and ``norm`` (k,) = ``N_r``."""
    if kind not in ("vectorial", "scalar"):
        raise ValueError("kind must be 'vectorial' or 'scalar'")
    _rtol(cluster_rtol)
    beta = np.asarray(beta, dtype=np.float64).reshape(-1)
    k, k0 = beta.size, float(k0)
    if k < 1 or not np.all(np.isfinite(beta) & (beta > 0)) or not (np.isfinite(k0) and k0 > 0):
        raise ValueError("beta must hold k >= 1 finite positive numbers and k0 must be finite and positive")
    need = ("M_px", "K_px") if kind == "vectorial" else ("M_px",)
    if any(nm not in densities for nm in need) or "support" not in densities:
        raise ValueError(f"densities must hold {', '.join(need)} and support")
    n_map = np.asarray(n_map, dtype=np.float64)
    P = {nm: np.asarray(densities[nm], dtype=np.float64) for nm in need}
    if n_map.ndim != 2 or any(P[nm].shape != (k,) + n_map.shape for nm in need):
        raise ValueError("the densities must be (k, ny, nx) with k = beta.size and (ny, nx) the shape of n_map")
    gram = "M_w" if kind == "vectorial" else "M"
    if gram not in grams or np.shape(grams[gram]) != (k, k):
        raise ValueError(f"grams must hold {gram}, k x k")
    norm = np.diag(np.asarray(grams[gram], dtype=np.float64)).copy()
    if not np.all(norm > 0):
        raise ValueError(f"the diagonal of {gram} must be positive")
    if kind == "vectorial":
        mu = beta ** 2
        dmu = (P["K_px"] - mu[:, None, None] * P["M_px"]) / norm[:, None, None]
        deps = dmu / (2.0 * beta * k0)[:, None, None]
    else:
        mu = -beta ** 2
        dlam = -(k0 * k0) * P["M_px"] / norm[:, None, None]
        deps = -dlam / (2.0 * beta * k0)[:, None, None]
    label = _clusters(mu, cluster_rtol * float(np.abs(mu).max()))
    mean = deps.copy()
    for S in _cluster_members(label):
        mean[S] = deps[S].mean(axis=0)[None]
    two_n = 2.0 * n_map[None]
    return {"dneff_deps": deps, "dneff_dn": two_n * deps, "cluster": label, "dneff_deps_cluster": mean,
            "dneff_dn_cluster": two_n * mean, "support": np.asarray(densities["support"]), "norm": norm}


def index_map_gradient(modes: Sequence[Dict], mesh, geometry, cluster_rtol: float = 1e-10, device: Optional[int] = None) -> Dict:
    """d n_eff of every mode of a profile solve in every pixel of the profile's sampled map, from one solve.

    ``geometry``: a :class:`.profile.ProfiledGeometry` whose profile carries a map (``IndexProfile.sampled``); ``mesh``: the
    mesh of the solve or a :class:`ModeFields` on it.  The modes are staged once; ``plfem_profile_grams`` (for the norms)
    and ``plfem_index_map_gradients`` run on them.  Returns what :func:`index_map_gradient_from_densities` does, and
    ``grams``, ``densities``.  A pixel with ``support`` 0 -- outside the mesh, or wholly under layers -- has an exact zero
    gradient.  Argument errors raise ``ValueError`` before any device call."""
    kind, beta, profile, mf, vals = _enter("index_map_gradient", modes, mesh, geometry, cluster_rtol, device)
    if profile.index_map is None:
        raise ValueError("index_map_gradient needs a profile with a sampled map (IndexProfile.sampled)")
    mf._ensure_locator()
    staged, _src = mf._stage(vals)
    grams = _profile_grams(mf, kind, staged, profile)
    dens = mf._index_map_densities_staged(kind, staged, profile)
    n_map = np.sqrt(profile.index_map[0])
    res = index_map_gradient_from_densities(kind, grams, dens, beta, float(geometry.k0), n_map, cluster_rtol)
    res.update(grams=grams, densities=dens)
    return res


__all__ = ["index_map_gradient", "index_map_gradient_from_densities"]
