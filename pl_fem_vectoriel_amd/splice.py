"""Splices, alignment maps and scaling tapers from posed mode overlaps.

Between two cross-sections of a photonic lantern everything is an overlap of two mode sets that do not share a frame: a
splice with a lateral offset, the angular alignment of a multicore fibre, the step from one taper section to the next.
:func:`.fields.mode_overlap_poses` computes ``O[p, i, j] = integral over mesh B of u'_a,i . u_b,j`` for many poses p of
mesh A relative to mesh B in one GPU call; the rest is host math on ka x kb matrices:

* with the self-Grams ``Gaa``, ``Gbb`` of the two sets, each on its own mesh, ``T = Gbb^(-1/2) O^T Gaa^(-1/2) / m`` takes
  amplitudes on the Loewdin-orthonormalised set A to amplitudes on the orthonormalised set B (the posed A has the
  self-overlap ``m^2 Gaa``).  Its singular values are the field transmissions of the splice's eigenchannels;
* a taper whose cross-section only scales is a staircase of such interfaces with free propagation in between.

This is plain overlap projection: what is not captured by set B is lost, reflections and the admittance factor ``2
sqrt(beta_a beta_b) / (beta_a + beta_b)`` of a step are neglected.  Lengths are in um.
"""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np

from .fields import ModeFields, _records, mode_overlap, mode_overlap_poses, pose_table


def _inv_sqrt(G, name: str) -> np.ndarray:
    """``G^(-1/2)`` of a symmetric positive definite Gram; ``ValueError`` otherwise."""
    G = np.asarray(G, dtype=np.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1] or G.shape[0] < 1 or not np.all(np.isfinite(G)):
        raise ValueError(f"{name} must be a finite square matrix")
    w, V = np.linalg.eigh(0.5 * (G + G.T))
    if w[0] <= 0:
        raise ValueError(f"{name} is not positive definite: the modes of that set are linearly dependent")
    return (V / np.sqrt(w)[None, :]) @ V.T


def _db_of_singular_values(sv: np.ndarray):
    """(IL_dB, MDL_dB) of singular values (..., n): -10 log10(mean sigma^2), 10 log10(sigma_max^2 / sigma_min^2)."""
    p = sv * sv
    with np.errstate(divide="ignore", invalid="ignore"):
        il = -10.0 * np.log10(p.mean(axis=-1))
        mdl = 10.0 * np.log10(p.max(axis=-1) / p.min(axis=-1))
    return il, np.where(p.max(axis=-1) > 0, mdl, np.inf)


def splice_quantities_from_overlaps(O, Gaa, Gbb, scale=1.0) -> Dict[str, np.ndarray]:
    """The host math of :func:`splice_map`: a pure function of the posed overlaps ``O`` (T, ka, kb) (or one (ka, kb)
    matrix), the self-Grams ``Gaa`` (ka, ka) and ``Gbb`` (kb, kb) of the two sets on their own meshes, and the
    magnification ``scale`` of each pose (a number or (T,)).

    Returns ``transfer`` (T, kb, ka) = ``Gbb^(-1/2) O^T Gaa^(-1/2) / scale``, from amplitudes on the Loewdin-orthonormalised
    set A to amplitudes on the orthonormalised set B; ``singular_values`` (T, min(ka, kb)), descending; ``IL_dB`` (T,) =
    ``-10 log10(mean sigma^2)`` over the min(ka, kb) channels; ``MDL_dB`` (T,) = ``10 log10(sigma_max^2 / sigma_min^2)``
    (inf when a channel is dark); ``power`` (T, kb, ka) = ``|transfer|^2``.  A single (ka, kb) matrix gives the same without
    the leading axis."""
    O = np.asarray(O, dtype=np.float64)
    single = O.ndim == 2
    if single:
        O = O[None]
    if O.ndim != 3 or O.shape[1] < 1 or O.shape[2] < 1 or not np.all(np.isfinite(O)):
        raise ValueError("O must be a finite array of shape (T, ka, kb) or (ka, kb)")
    Sa, Sb = _inv_sqrt(Gaa, "Gaa"), _inv_sqrt(Gbb, "Gbb")
    if Sa.shape[0] != O.shape[1] or Sb.shape[0] != O.shape[2]:
        raise ValueError("Gaa must be ka x ka and Gbb kb x kb for O of shape (T, ka, kb)")
    try:
        m = np.broadcast_to(np.asarray(scale, dtype=np.float64), (O.shape[0],))
    except (TypeError, ValueError):
        raise ValueError("scale must be a positive number or one per pose") from None
    if not np.all(np.isfinite(m) & (m > 0)):
        raise ValueError("scale must be finite and > 0")
    T = (Sb @ O.transpose(0, 2, 1) @ Sa) / m[:, None, None]
    sv = np.linalg.svd(T, compute_uv=False)
    il, mdl = _db_of_singular_values(sv)
    res = {"transfer": T, "singular_values": sv, "IL_dB": il, "MDL_dB": mdl, "power": T * T}
    return {nm: v[0] for nm, v in res.items()} if single else res


def _axis(v, name: str) -> np.ndarray:
    try:
        a = np.atleast_1d(np.asarray(v, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number or a 1-D array of numbers") from None
    if a.ndim != 1 or a.size < 1 or not np.all(np.isfinite(a)):
        raise ValueError(f"{name} must be a finite number or a non-empty 1-D array of finite numbers")
    return a


def _number(v, name: str, positive: bool = False) -> float:
    try:
        x = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be one number") from None
    if not np.isfinite(x) or (positive and x <= 0):
        raise ValueError(f"{name} must be finite" + (" and > 0" if positive else ""))
    return x


def splice_map(modes_a: Sequence[Dict], mesh_a, modes_b: Sequence[Dict], mesh_b, dx, dy, angle: float = 0.0,
               scale: float = 1.0, device=None) -> Dict[str, np.ndarray]:
    """Splice of mode set A (on ``mesh_a``) to mode set B (on ``mesh_b``) on the grid of lateral offsets ``dx`` (nx,) x
    ``dy`` (ny,) (um), A turned by ``angle`` (rad) and magnified by ``scale``: one :func:`.fields.mode_overlap_poses` call
    for all ny nx poses plus the two self-Grams through :func:`.fields.mode_overlap`, unweighted, then
    :func:`splice_quantities_from_overlaps` (see there for every returned quantity), each with the leading axes (ny, nx);
    also ``overlap`` (ny, nx, ka, kb), ``Gaa``, ``Gbb``, ``dx``, ``dy``.  An offset that takes A off B's mesh gives exact zeros
    (``IL_dB = inf``).  Argument errors raise ``ValueError`` before anything touches the device."""
    x, y = _axis(dx, "dx"), _axis(dy, "dy")
    ang, m = _number(angle, "angle"), _number(scale, "scale", positive=True)
    ka_kind, _, _ = _records(modes_a)
    kb_kind, _, _ = _records(modes_b)
    if ka_kind is None or kb_kind is None:
        raise ValueError("no mode records")
    if ka_kind != kb_kind:
        raise ValueError("vectorial and scalar mode records cannot be mixed")
    fa = mesh_a if isinstance(mesh_a, ModeFields) else ModeFields(mesh_a, device=device)
    fb = fa if mesh_b is mesh_a else (mesh_b if isinstance(mesh_b, ModeFields) else ModeFields(mesh_b, device=device))
    fa._check_records(modes_a)                               # lengths, before the device
    fb._check_records(modes_b)
    poses = pose_table(x[None, :], y[:, None], ang, m)     # row iy nx + ix
    O = mode_overlap_poses(modes_a, fa, modes_b, fb, poses)
    Gaa = mode_overlap(modes_a, fa, modes_a, fa)
    Gbb = mode_overlap(modes_b, fb, modes_b, fb)
    res = splice_quantities_from_overlaps(O, Gaa, Gbb, m)
    res = {nm: v.reshape((y.size, x.size) + v.shape[1:]) for nm, v in res.items()}
    res.update(overlap=O.reshape((y.size, x.size) + O.shape[1:]), Gaa=Gaa, Gbb=Gbb, dx=x, dy=y)
    return res


def taper_from_interfaces(T_list, betas, lengths) -> Dict[str, np.ndarray]:
    """Staircase transfer of n sections joined by n - 1 interfaces: a pure function.  Section i has the propagation
    constants ``betas[i]`` (k_i,) and the length ``lengths[i]``; ``T_list[i]`` (k_(i+1), k_i) takes amplitudes of section i
    to amplitudes of section i + 1.  The total is ``P_(n-1) T_(n-2) ... T_0 P_0`` with ``P_i = diag(exp(-1j betas[i]
    lengths[i]))``: the light meets section 0 first.

    Returns ``transfer`` (k_(n-1), k_0) complex; ``power`` = ``|transfer|^2``, the power reaching every output mode per input
    mode; ``transmitted`` (k_0,), its column sums; ``singular_values``, ``IL_dB`` and ``MDL_dB`` of the total as in
    :func:`splice_quantities_from_overlaps`."""
    try:
        Ts = [np.asarray(T, dtype=np.complex128) for T in T_list]
        bs = [np.asarray(b, dtype=np.float64).reshape(-1) for b in betas]
        L = np.asarray(lengths, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("T_list, betas and lengths must hold numeric arrays") from None
    n = len(bs)
    if n < 1 or len(Ts) != n - 1 or L.size != n:
        raise ValueError("n sections need n entries of betas and lengths and n - 1 interfaces")
    if not np.all(np.isfinite(L)) or np.any(L < 0) or any(b.size < 1 or not np.all(np.isfinite(b)) for b in bs):
        raise ValueError("lengths must be finite and >= 0, and every betas[i] a non-empty finite vector")
    for i, T in enumerate(Ts):
        if T.ndim != 2 or T.shape != (bs[i + 1].size, bs[i].size) or not np.all(np.isfinite(T)):
            raise ValueError(f"T_list[{i}] must be a finite ({bs[i + 1].size}, {bs[i].size}) matrix: from section {i} to {i + 1}")
    total = np.diag(np.exp(-1j * bs[0] * L[0]))
    for i, T in enumerate(Ts):
        total = np.exp(-1j * bs[i + 1] * L[i + 1])[:, None] * (T @ total)
    power = np.abs(total) ** 2
    sv = np.linalg.svd(total, compute_uv=False)
    il, mdl = _db_of_singular_values(sv)
    return {"transfer": total, "power": power, "transmitted": power.sum(axis=0), "singular_values": sv,
            "IL_dB": float(il), "MDL_dB": float(mdl)}


def taper_transfer(modes_list, mesh, scales, lengths, k0: float, device=None) -> Dict:
    """Mode-matching transfer of a taper whose cross-section only scales, for scalar records.

    Section i is the cross-section of ``mesh`` magnified by ``scales[i]``, of length ``lengths[i]`` (um), at the vacuum
    wavenumber ``k0`` (1 / um).  A cross-section scaled by s at k0 has exactly the discrete eigenvectors of the unscaled
    mesh at k0 s (in 2-D the stiffness form is scale invariant and the mass forms scale by s^2), with the same n_eff: so
    ``modes_list[i]`` are the records solved on ``mesh`` itself with the geometry's wavelength divided by ``scales[i]``, one
    mesh and one analysis for the whole taper, and ``betas[i] = k0 n_eff``.  Interface i is the posed overlap of
    ``modes_list[i]`` (set A, magnification ``scales[i] / scales[i+1]``, no shift, no rotation) on ``modes_list[i+1]`` (set
    B), Loewdin-normalised as in :func:`splice_quantities_from_overlaps`; the mode counts may differ from section to
    section.  The product is :func:`taper_from_interfaces` (see there for the returned quantities); also ``interfaces``
    (the list of T_i), ``betas`` and ``interface_IL_dB``.

    Plain overlap projection: reflections at the steps and the factor ``2 sqrt(beta_a beta_b) / (beta_a + beta_b)`` are
    neglected, and what a step scatters out of the next section's mode set is lost.  ``ValueError`` for vectorial records
    (their bi-orthogonality under the 1/eps mass form is not this inner product) and for malformed arguments, before
    anything touches the device."""
    try:
        sections = [list(m) for m in modes_list]
        s = np.asarray(scales, dtype=np.float64).reshape(-1)
        L = np.asarray(lengths, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("modes_list must be a list of record lists, scales and lengths 1-D arrays of numbers") from None
    n = len(sections)
    if n < 1 or s.size != n or L.size != n:
        raise ValueError("modes_list, scales and lengths must have one entry per section")
    if not np.all(np.isfinite(s) & (s > 0)) or not np.all(np.isfinite(L) & (L >= 0)):
        raise ValueError("scales must be finite and > 0, lengths finite and >= 0")
    k0 = _number(k0, "k0", positive=True)
    betas = []
    for i, modes in enumerate(sections):
        kind, _, _ = _records(modes)
        if kind is None:
            raise ValueError(f"section {i} has no mode records")
        if kind != "scalar":
            raise ValueError("taper_transfer is for scalar records: the vectorial modes are bi-orthogonal under the 1/eps "
                             "mass form, not under this inner product")
        try:
            ne = np.array([float(m["n_eff"]) for m in modes])
        except (KeyError, TypeError, ValueError):
            raise ValueError(f"every record of section {i} needs a numeric 'n_eff'") from None
        if not np.all(np.isfinite(ne) & (ne > 0)):
            raise ValueError(f"every record of section {i} needs a finite, positive 'n_eff'")
        betas.append(k0 * ne)
    mf = mesh if isinstance(mesh, ModeFields) else ModeFields(mesh, device=device)
    for modes in sections:
        mf._check_records(modes)                             # lengths, before the device
    grams = [mode_overlap(modes, mf, modes, mf) for modes in sections]
    Ts, ils = [], []
    for i in range(n - 1):
        m = s[i] / s[i + 1]
        O = mode_overlap_poses(sections[i], mf, sections[i + 1], mf, pose_table(scale=m))
        q = splice_quantities_from_overlaps(O[0], grams[i], grams[i + 1], m)
        Ts.append(q["transfer"])
        ils.append(float(q["IL_dB"]))
    res = taper_from_interfaces(Ts, betas, L)
    res.update(interfaces=Ts, betas=betas, interface_IL_dB=np.array(ils))
    return res


__all__ = ["splice_quantities_from_overlaps", "splice_map", "taper_from_interfaces", "taper_transfer"]
