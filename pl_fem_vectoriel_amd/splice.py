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

For vectorial records the H.H overlap above is not the power inner product: the physically
meaningful transfer is the cross flux ``int (E_a x H_b + E_b x H_a) . z`` over the modal powers.
:func:`.fields.flux_overlap_poses` returns its four beta-free sums per pose, :func:`flux_transfer_from_grams` is the host
math on them (with each set Loewdin-orthonormalised under its cross powers when those are given as a matrix), :func:`splice_power_map` and :func:`taper_transfer_vectorial` are the counterparts of :func:`splice_map` and
:func:`taper_transfer`.  Reflections and the backward modes stay neglected there too.
"""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np

from .fields import ModeFields, _records, flux_overlap_poses, mode_overlap, mode_overlap_poses, pose_table
from .power import power_quantities_from_grams


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


def _vector(v, n: int, name: str) -> np.ndarray:
    try:
        a = np.asarray(v, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be {n} numbers") from None
    if a.size != n or not np.all(np.isfinite(a)):
        raise ValueError(f"{name} must be {n} finite numbers")
    return a


def _power(p, n: int, name: str) -> np.ndarray:
    """The powers of a set of n modes: a finite vector (n,), or a finite symmetric matrix (n, n) of cross powers."""
    try:
        a = np.asarray(p, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be {n} numbers or an ({n}, {n}) matrix") from None
    if a.ndim == 2 and a.shape == (n, n) and (n > 1 or np.ndim(p) == 2):
        if not np.all(np.isfinite(a)) or np.abs(a - a.T).max() > 1e-12 * np.abs(a).max():
            raise ValueError(f"{name} as a matrix must be finite and symmetric (cross_sym of mode_power)")
        return a
    return _vector(a, n, name)


def _inv_sqrt_abs(p: np.ndarray) -> np.ndarray:
    """``1 / sqrt(|p|)`` entry by entry, 0 where p is 0."""
    live = p != 0
    return np.where(live, 1.0 / np.sqrt(np.abs(np.where(live, p, 1.0))), 0.0)


def flux_transfer_from_grams(MA, GA, MB, GB, beta_a, k0_a, beta_b, k0_b, power_a, power_b, scale=1.0) -> Dict[str, np.ndarray]:
    """The host math of :func:`splice_power_map`: a pure function of the four posed flux sums ``MA``, ``GA``, ``MB``, ``GB``
    of :func:`.fields.flux_overlap_poses`, each (T, ka, kb) (or one (ka, kb) matrix), the propagation constants and vacuum
    wavenumbers each set was solved with, the modal powers ``power_a`` (ka,), ``power_b`` (kb,) of each set on its own mesh
    (``power`` of :func:`.power.mode_power`), and the magnification ``scale`` = m of each pose (a number or (T,))::

        X_ab = (beta_a[:, None] MA + GA / beta_a[:, None]) / k0_a         int (E_a' x H_b) . z
        X_ba = (beta_b[None, :] MB + GB / beta_b[None, :]) / k0_b         int (E_b x H_a') . z
        T[j, i] = (X_ab + X_ba)[i, j] / (4 m sqrt(|P_a,i| |P_b,j|))

    A field magnified by m has every wavenumber divided by m and ``g`` divided by m^2, so its E is A's own E turned and its
    power is ``m^2 P_a``; the two sets meet at one optical frequency, so ``k0_a / m`` must equal ``k0_b`` to 1e-9 relative
    (``ValueError`` otherwise).  A mode of zero power gives a zero row or column, as in
    :func:`.power.power_quantities_from_grams`.

    With power vectors the modes of a set are taken as they are: ``transfer`` is the matrix of normalised cross fluxes, and
    it is the transfer between the two sets only as far as the modes of each are power-orthogonal.  Either power may
    instead be the set's symmetrised cross-power matrix, (ka, ka) or (kb, kb) (``cross_sym`` of :func:`.power.mode_power`),
    whose diagonal is the power vector: the set is then Loewdin-orthonormalised under it, as
    :func:`splice_quantities_from_overlaps` orthonormalises under the self-Gram::

        T = P_b^(-1/2) (X_ab + X_ba)^T P_a^(-1/2) / (4 m)

    which takes amplitudes on the power-orthonormalised set A to amplitudes on the power-orthonormalised set B; a set
    onto itself at the identity pose gives the identity whatever its cross powers are, and a diagonal matrix gives the
    vector formula.  ``ValueError`` unless such a matrix is symmetric positive definite (a set with a backward or a
    powerless mode has no such basis).

    Returns ``transfer`` (T, kb, ka); ``power`` = ``|transfer|^2``; ``singular_values`` (T, min(ka, kb)), descending;
    ``IL_dB`` and ``MDL_dB`` (T,) as in :func:`splice_quantities_from_overlaps`.  Single (ka, kb) matrices give the same
    without the leading axis."""
    try:
        G = [np.asarray(g, dtype=np.float64) for g in (MA, GA, MB, GB)]
    except (TypeError, ValueError):
        raise ValueError("MA, GA, MB and GB must be real arrays") from None
    single = G[0].ndim == 2
    if single:
        G = [g[None] if g.ndim == 2 else g for g in G]
    if G[0].ndim != 3 or G[0].shape[1] < 1 or G[0].shape[2] < 1 or any(g.shape != G[0].shape for g in G):
        raise ValueError("MA, GA, MB and GB must have one shape, (T, ka, kb) or (ka, kb)")
    if not all(np.all(np.isfinite(g)) for g in G):
        raise ValueError("MA, GA, MB and GB must be finite")
    nT, ka, kb = G[0].shape
    ba, bb = _vector(beta_a, ka, "beta_a"), _vector(beta_b, kb, "beta_b")
    if np.any(ba == 0) or np.any(bb == 0):
        raise ValueError("every beta must be finite and non-zero")
    pa, pb = _power(power_a, ka, "power_a"), _power(power_b, kb, "power_b")
    k0a, k0b = _number(k0_a, "k0_a", positive=True), _number(k0_b, "k0_b", positive=True)
    try:
        m = np.broadcast_to(np.asarray(scale, dtype=np.float64), (nT,))
    except (TypeError, ValueError):
        raise ValueError("scale must be a positive number or one per pose") from None
    if not np.all(np.isfinite(m) & (m > 0)):
        raise ValueError("scale must be finite and > 0")
    if np.any(np.abs(k0a / m - k0b) > 1e-9 * k0b):
        raise ValueError("k0_a / scale must equal k0_b to 1e-9 relative: a set magnified by m stands at the wavenumber k0_a / m, "
                         f"got k0_a = {k0a}, k0_b = {k0b}, scale = {m.tolist() if nT > 1 else float(m[0])}")
    X_ab = (ba[None, :, None] * G[0] + G[1] / ba[None, :, None]) / k0a
    X_ba = (bb[None, None, :] * G[2] + G[3] / bb[None, None, :]) / k0b
    if pa.ndim == 1 and pb.ndim == 1:
        na, nb = _inv_sqrt_abs(pa), _inv_sqrt_abs(pb)
        T = ((X_ab + X_ba) * na[None, :, None] * nb[None, None, :] / (4.0 * m[:, None, None])).transpose(0, 2, 1)
    else:
        Na = np.diag(_inv_sqrt_abs(pa)) if pa.ndim == 1 else _inv_sqrt(pa, "power_a")
        Nb = np.diag(_inv_sqrt_abs(pb)) if pb.ndim == 1 else _inv_sqrt(pb, "power_b")
        T = (Nb @ (X_ab + X_ba).transpose(0, 2, 1) @ Na) / (4.0 * m[:, None, None])
    sv = np.linalg.svd(T, compute_uv=False)
    il, mdl = _db_of_singular_values(sv)
    res = {"transfer": T, "singular_values": sv, "IL_dB": il, "MDL_dB": mdl, "power": T * T}
    return {nm: v[0] for nm, v in res.items()} if single else res


def _k0_of(geometry, name: str) -> float:
    try:
        return _number(geometry.k0, f"{name}.k0", positive=True)
    except AttributeError:
        raise ValueError(f"{name} must have k0") from None


def _betas_of(modes, what: str) -> np.ndarray:
    try:
        b = np.array([float(m["beta"]) for m in modes], dtype=np.float64)
    except (KeyError, TypeError, ValueError):
        raise ValueError(f"every record of {what} needs a numeric 'beta'") from None
    if not np.all(np.isfinite(b) & (b != 0)):
        raise ValueError(f"every record of {what} needs a finite, non-zero 'beta'")
    return b


def _vectorial(modes, what: str) -> list:
    try:
        modes = list(modes)
    except TypeError:
        raise ValueError(f"{what} must be a list of mode records") from None
    kind, _, _ = _records(modes)
    if kind is None:
        raise ValueError(f"{what} has no mode records")
    if kind != "vectorial":
        raise ValueError(f"{what}: the power-normalised transfer needs vectorial records (scalar ones: splice_map, taper_transfer)")
    return modes


def splice_power_map(modes_a: Sequence[Dict], mesh_a, geometry_a, modes_b: Sequence[Dict], mesh_b, geometry_b, dx, dy,
                     angle: float = 0.0, scale: float = 1.0, orthonormalize: bool = True, device=None) -> Dict[str, np.ndarray]:
    """Power-normalised splice of the vectorial mode set A (on ``mesh_a``, solved with ``geometry_a``) to set B on the grid
    of lateral offsets ``dx`` (nx,) x ``dy`` (ny,) (um), A turned by ``angle`` (rad) and magnified by ``scale``: one
    :func:`.fields.flux_overlap_poses` call for all ny nx poses plus the power quantities of each side
    (:func:`.power.mode_power`: one ``flux_grams`` call each), then :func:`flux_transfer_from_grams` (see there for every
    returned quantity and for ``geometry_a.k0 / scale == geometry_b.k0``), each with the leading axes (ny, nx); also
    ``grams`` (the four raw sums, each (ny, nx, ka, kb)), ``power_a``, ``power_b``, ``cross_a``, ``cross_b`` (the symmetrised
    cross powers), ``dx``, ``dy``.

    ``orthonormalize=True``: each set is Loewdin-orthonormalised under its symmetrised cross powers, as :func:`splice_map`
    orthonormalises under the self-overlap, so that the solver's records need not be power-orthogonal (they are not, to a
    few per cent on coarse meshes) and a set spliced onto itself at zero offset gives the identity; ``ValueError`` when a
    set's cross-power matrix is not positive definite.  ``orthonormalize=False``: the modes as they are, each divided by
    the root of its own power.

    Each geometry gives its side's material (its index profile if it carries one, without a sampled map, else its
    discs) and k0.  An offset that takes A off B's mesh gives exact zeros.  Reflections are neglected.  Argument errors
    raise ``ValueError`` before anything touches the device."""
    x, y = _axis(dx, "dx"), _axis(dy, "dy")
    ang, m = _number(angle, "angle"), _number(scale, "scale", positive=True)
    modes_a, modes_b = _vectorial(modes_a, "modes_a"), _vectorial(modes_b, "modes_b")
    ba, bb = _betas_of(modes_a, "modes_a"), _betas_of(modes_b, "modes_b")
    k0a, k0b = _k0_of(geometry_a, "geometry_a"), _k0_of(geometry_b, "geometry_b")
    if abs(k0a / m - k0b) > 1e-9 * k0b:
        raise ValueError(f"geometry_a.k0 / scale must equal geometry_b.k0 to 1e-9 relative, got {k0a}, {k0b} and scale = {m}")
    fa = mesh_a if isinstance(mesh_a, ModeFields) else ModeFields(mesh_a, device=device)
    fb = fa if mesh_b is mesh_a else (mesh_b if isinstance(mesh_b, ModeFields) else ModeFields(mesh_b, device=device))
    poses = pose_table(x[None, :], y[:, None], ang, m)     # row iy nx + ix
    G = flux_overlap_poses(modes_a, fa, geometry_a, modes_b, fb, geometry_b, poses)
    qa = power_quantities_from_grams(fa.flux_grams(modes_a, geometry_a), ba, k0a)
    qb = qa if (fb is fa and modes_b is modes_a and geometry_b is geometry_a) else \
        power_quantities_from_grams(fb.flux_grams(modes_b, geometry_b), bb, k0b)
    pa, pb = (qa["cross_sym"], qb["cross_sym"]) if orthonormalize else (qa["power"], qb["power"])
    res = flux_transfer_from_grams(G["MA"], G["GA"], G["MB"], G["GB"], ba, k0a, bb, k0b, pa, pb, m)
    res = {nm: v.reshape((y.size, x.size) + v.shape[1:]) for nm, v in res.items()}
    res.update(grams={nm: v.reshape((y.size, x.size) + v.shape[1:]) for nm, v in G.items()}, power_a=qa["power"],
               power_b=qb["power"], cross_a=qa["cross_sym"], cross_b=qb["cross_sym"], dx=x, dy=y)
    return res


def taper_transfer_vectorial(modes_list, mesh, geometry, scales, lengths, k0: float, device=None) -> Dict:
    """:func:`taper_transfer` for vectorial records, with power-normalised interfaces.

    Section i is the cross-section of ``mesh`` and ``geometry`` magnified by ``scales[i]``, of length ``lengths[i]`` (um), at
    the vacuum wavenumber ``k0`` (1 / um).  The scaling equivalence of :func:`taper_transfer` holds for the vectorial pencil
    too (its curl and divergence forms K and D are scale invariant in 2-D, both mass forms scale by s^2): ``modes_list[i]``
    are the records solved on ``mesh`` itself at the wavenumber ``k0 scales[i]`` (the geometry's wavelength divided by
    ``scales[i]``), whose ``beta`` is ``scales[i]`` times the section's own.  Interface i is one posed flux overlap of
    ``modes_list[i]`` (set A, magnification ``scales[i] / scales[i+1]``, no shift, no rotation) on ``modes_list[i+1]`` (set B)
    through :func:`flux_transfer_from_grams`, with the modal powers of each section from its own flux Grams; the mode
    counts may differ.  The product is :func:`taper_from_interfaces` with ``betas[i] = beta / scales[i]``; also
    ``interfaces``, ``betas``, ``interface_IL_dB`` and ``powers``.

    Reflections at the steps and the backward modes are neglected, what a step scatters out of the next section's set is
    lost, and the modes of a section are not assumed power-orthogonal.  ``geometry`` gives the material only (its index
    profile without a sampled map, else its discs).  ``ValueError`` for scalar records and malformed arguments, before
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
    sections = [_vectorial(modes, f"section {i}") for i, modes in enumerate(sections)]
    rec_betas = [_betas_of(modes, f"section {i}") for i, modes in enumerate(sections)]
    mf = mesh if isinstance(mesh, ModeFields) else ModeFields(mesh, device=device)
    mat = mf._material(geometry)                             # the material, before the device
    if mat.index_map is not None:
        raise ValueError("taper_transfer_vectorial: an index profile with a sampled map is not supported")
    for modes in sections:
        mf._check_records(modes)                             # lengths, before the device
    powers = [power_quantities_from_grams(mf.flux_grams(modes, geometry), b, k0 * si)["power"]
              for modes, b, si in zip(sections, rec_betas, s)]
    Ts, ils = [], []
    for i in range(n - 1):
        m = s[i] / s[i + 1]
        G = flux_overlap_poses(sections[i], mf, geometry, sections[i + 1], mf, geometry, pose_table(scale=m))
        q = flux_transfer_from_grams(G["MA"][0], G["GA"][0], G["MB"][0], G["GB"][0], rec_betas[i], k0 * s[i], rec_betas[i + 1],
                                     k0 * s[i + 1], powers[i], powers[i + 1], m)
        Ts.append(q["transfer"])
        ils.append(float(q["IL_dB"]))
    betas = [b / si for b, si in zip(rec_betas, s)]
    res = taper_from_interfaces(Ts, betas, L)
    res.update(interfaces=Ts, betas=betas, interface_IL_dB=np.array(ils), powers=powers)
    return res


__all__ = ["splice_quantities_from_overlaps", "splice_map", "taper_from_interfaces", "taper_transfer", "flux_transfer_from_grams",
           "splice_power_map", "taper_transfer_vectorial"]
