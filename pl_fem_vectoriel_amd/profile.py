"""Index profiles: cross-sections beyond "discs of one ``n_core`` on ``n_clad``".

A profile is a background permittivity and an ordered table of at most 64 layers, each a closed disc or ring around a
centre with a constant or a graded (alpha-profile) permittivity; a later layer overwrites an earlier one.  That covers a
cladding inside a low-index jacket, trenches and rings, graded cores and cores of unequal index.  The device evaluates the
same table, operation for operation (``profile_eps`` of ``csrc/p2_element.h``, ``plfem_set_index_profile`` of
``include/plfem.h``):

* membership: ``d2 = dx * dx + dy * dy`` with every product rounded on its own; the point is in the layer when
  ``r_in * r_in <= d2 <= r_out * r_out`` -- with ``r_in = 0`` the closed disc of ``MCFGeometry.epsilon``, ties included;
* value: ``eps_a`` for a constant layer, ``eps_a + (eps_b - eps_a) * t ** g`` with ``t = (sqrt(d2) - r_in) / (r_out -
  r_in)`` clamped to [0, 1] for a graded one: ``n^2(rho) = n0^2 + (n_edge^2 - n0^2) (rho / a)^alpha``.

:class:`ProfiledGeometry` attaches a profile to a geometry of the package; both solvers then assemble with it
(``geometry.index_profile``), and :meth:`.fields.ModeFields.profile_grams` gives the Grams of such a solve.  The mesh
recipe stays the reference's: points are placed around ``positions`` / ``core_radii`` of the base geometry, not on the
rims of rings or jackets.

Under the layers a profile may carry a sampled **map** (:meth:`IndexProfile.sampled`): permittivities on a uniform pixel
grid -- a measured index profile, an elliptical or polygonal core, a fused waist, a thermal or Kerr-perturbed index.
Inside the closed extent of the grid the background is the bilinear interpolant of the map in eps = n^2 (not in n),
outside it the constant background; the layers are painted over both.  With ``inv_dx = 1 / dx`` formed once:

* ``tx = (x - x0) * inv_dx`` (``ty`` likewise), the point is inside when ``0 <= tx <= nx - 1`` and ``0 <= ty <= ny - 1``;
* ``i0 = min(floor(tx), nx - 2)``, ``a = tx - i0`` (``j0``, ``b`` likewise);
* ``lo = (1 - a) E[j0, i0] + a E[j0, i0 + 1]``, ``hi`` the same in row ``j0 + 1``, ``eps = lo (1 - b) + hi b``, every
  product rounded on its own (``plfem_set_index_map``).

``epsilon`` is linear in the VALUES of a profile at fixed shapes -- the background, ``eps_a`` and ``eps_b`` of every layer,
every pixel of the map.  A :class:`ProfileTangent` (``tangent_eps``, ``tangent_index``, ``unit_tangents``) is a first-order
change of them, evaluated with the same membership, ``t``, ``g`` and bilinear weights; group index, index sensitivities and
bend response of a profile solve are Grams of the modes under such tangents (:mod:`.profile_response`,
:meth:`.fields.ModeFields.profile_tangent_grams`).

A section that is not made of circles is resolved by refinement on the error indicators (:func:`.adapt.adaptive_solve`),
not by the mesh recipe.
"""
from __future__ import annotations

import hashlib
from typing import Optional

import numpy as np

MAX_LAYERS = 64                    # MAX_LAYERS of csrc/plan.h
MAP_MAX_SAMPLES = 1 << 24          # MAP_SAMPLES of csrc/plan.h
LAYER_DOUBLES = 8                  # (cx, cy, r_in, r_out, eps_a, eps_b, g, 0)


def _number(v, name: str) -> float:
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a finite number") from None
    if not np.isfinite(f):
        raise ValueError(f"{name} must be a finite number")
    return f


def _index(v, name: str) -> float:
    n = _number(v, name)
    if n <= 0:
        raise ValueError(f"{name} must be a positive refractive index")
    return n


class IndexProfile:
    """``IndexProfile(n_background)``, then layers in the order they are painted: ``.disc(center, radius, n)``,
    ``.ring(center, r_in, r_out, n)``, ``.graded(center, radius, n_center, n_edge, alpha)`` (each returns the profile, so
    calls chain).  Argument errors raise ``ValueError``."""

    def __init__(self, n_background):
        self.n_background = _index(n_background, "n_background")
        self.eps_background = self.n_background ** 2
        self._layers = []
        self._indices = [self.n_background]
        self._map = None                 # (eps (ny, nx), x0, y0, dx, dy) of .sampled, or None

    def __len__(self):
        return len(self._layers)

    def sampled(self, x, y, n):
        """The map under the layers: refractive indices ``n`` of shape ``(ny, nx)``, finite and positive, on the pixel
        axes ``x`` (nx) and ``y`` (ny) -- 2 to 8192 finite, ascending, uniformly spaced numbers each, at most 2^24 pixels
        in all.  It is stored as ``n * n`` and interpolated bilinearly in that.  Returns the profile; a second call
        replaces the map."""
        from .fields import _grid_axis
        x, dx = _grid_axis(x, "x")
        y, dy = _grid_axis(y, "y")
        if x.size * y.size > MAP_MAX_SAMPLES:
            raise ValueError(f"the map must have at most 2^24 pixels, not {x.size} x {y.size}")
        try:
            n = np.asarray(n, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("n must be an array of finite positive refractive indices") from None
        if n.shape != (y.size, x.size):
            raise ValueError(f"n must have shape (ny, nx) = ({y.size}, {x.size}), not {n.shape}")
        if not (np.all(np.isfinite(n)) and np.all(n > 0)):
            raise ValueError("n must be finite and positive everywhere")
        with np.errstate(over="ignore"):
            eps = np.ascontiguousarray(n * n)
        if not (np.all(np.isfinite(eps)) and np.all(eps > 0)):
            raise ValueError("n * n must be finite and positive everywhere")
        eps.setflags(write=False)
        self._map = (eps, float(x[0]), float(y[0]), float(dx), float(dy))
        return self

    @property
    def index_map(self):
        """``(eps, x0, y0, dx, dy)`` of the map as the C ABI takes it -- ``eps`` the (ny, nx) float64 permittivities,
        read-only -- or None."""
        return self._map

    def _add(self, center, r_in, r_out, n_a, n_b, g):
        try:
            cx, cy = (float(v) for v in np.asarray(center, dtype=np.float64).reshape(-1))
        except (TypeError, ValueError):
            raise ValueError("center must be two finite numbers (x, y)") from None
        if not (np.isfinite(cx) and np.isfinite(cy)):
            raise ValueError("center must be two finite numbers (x, y)")
        if r_in < 0:
            raise ValueError("r_in must be >= 0")
        if not r_out > r_in:
            raise ValueError("the outer radius must be larger than the inner one")
        if g < 0:
            raise ValueError("alpha must be >= 0")
        if len(self._layers) >= MAX_LAYERS:
            raise ValueError(f"at most {MAX_LAYERS} layers")
        self._layers.append((cx, cy, r_in, r_out, n_a ** 2, n_b ** 2, g, 0.0))
        self._indices += [n_a, n_b]
        return self

    def disc(self, center, radius, n):
        """A closed disc of index ``n``."""
        n = _index(n, "n")
        return self._add(center, 0.0, _number(radius, "radius"), n, n, 0.0)

    def ring(self, center, r_in, r_out, n):
        """A ring of index ``n``, closed on both rims."""
        n = _index(n, "n")
        return self._add(center, _number(r_in, "r_in"), _number(r_out, "r_out"), n, n, 0.0)

    def graded(self, center, radius, n_center, n_edge, alpha):
        """A graded disc: ``n^2(rho) = n_center^2 + (n_edge^2 - n_center^2) (rho / radius)^alpha``, alpha > 0."""
        alpha = _number(alpha, "alpha")
        if alpha <= 0:
            raise ValueError("alpha must be > 0 (a constant disc is .disc)")
        return self._add(center, 0.0, _number(radius, "radius"), _index(n_center, "n_center"), _index(n_edge, "n_edge"), alpha)

    @property
    def n_max(self) -> float:
        top = max(self._indices)
        return top if self._map is None else max(top, float(np.sqrt(self._map[0].max())))

    @property
    def n_min(self) -> float:
        low = min(self._indices)
        return low if self._map is None else min(low, float(np.sqrt(self._map[0].min())))

    def table(self) -> np.ndarray:
        """The layers as the C ABI takes them: (nlayer, 8) float64, rows ``(cx, cy, r_in, r_out, eps_a, eps_b, g, 0)``."""
        return np.ascontiguousarray(np.array(self._layers, dtype=np.float64).reshape(-1, LAYER_DOUBLES))

    def epsilon(self, x, y) -> np.ndarray:
        """Real relative permittivity at the points (float64, the shape of ``x``), by the operations of the device."""
        x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        eps = np.full(np.broadcast(x, y).shape, self.eps_background, dtype=np.float64)
        if self._map is not None:
            self._paint_map(eps, *np.broadcast_arrays(x, y))
        for cx, cy, r_in, r_out, eps_a, eps_b, g, _ in self._layers:
            dx, dy = x - cx, y - cy
            d2 = dx * dx + dy * dy
            inside = (r_in * r_in <= d2) & (d2 <= r_out * r_out)
            if g > 0:
                t = np.minimum(np.maximum((np.sqrt(d2[inside]) - r_in) / (r_out - r_in), 0.0), 1.0)
                eps[inside] = eps_a + (eps_b - eps_a) * np.power(t, g)
            else:
                eps[inside] = eps_a
        return eps

    # -- tangents: first-order changes of the values at fixed shapes ---------------------------------------------
    def tangent_eps(self, d_background=0.0, d_layers=0.0, d_map=None) -> "ProfileTangent":
        """The tangent with raw ``d eps``: ``d_background`` a number, ``d_layers`` a number, ``(nlayer,)`` or ``(nlayer,
        2)`` = (d_eps_a, d_eps_b) per layer (a constant layer has one value: both must agree), ``d_map`` None or
        ``(ny, nx)`` on the profile's own pixel grid (only if the profile has a map)."""
        return ProfileTangent(self, d_background, d_layers, d_map)

    def tangent_index(self, dn_background=0.0, dn_layers=0.0, dn_map=None) -> "ProfileTangent":
        """The tangent of an index change, ``d eps = 2 n dn``: centre and edge of a graded layer separately, the map by
        ``2 sqrt(E) dn_map`` (a scalar ``dn_map`` is broadcast).  Shapes as for :meth:`tangent_eps`."""
        n_layers = np.sqrt(self.table()[:, 4:6])
        d_layers = 2.0 * n_layers * _layer_pairs(dn_layers, len(self), "dn_layers")
        d_map = None
        if dn_map is not None:
            if self._map is None:
                raise ValueError("dn_map needs a profile with a map")
            E = self._map[0]
            try:
                dn = np.broadcast_to(np.asarray(dn_map, dtype=np.float64), E.shape)
            except (TypeError, ValueError):
                raise ValueError(f"dn_map must be a number or have shape (ny, nx) = {E.shape}") from None
            d_map = 2.0 * np.sqrt(E) * dn
        return ProfileTangent(self, 2.0 * self.n_background * _number(dn_background, "dn_background"), d_layers, d_map)

    def unit_tangents(self) -> list:
        """``nlayer + 1`` tangents: ``dn = 1`` on the background (with the map, when there is one), then on each layer in
        turn (a graded layer: a uniform offset of centre and edge)."""
        out = [self.tangent_index(dn_background=1.0, dn_map=None if self._map is None else 1.0)]
        for l in range(len(self)):
            dn = np.zeros(len(self))
            dn[l] = 1.0
            out.append(self.tangent_index(dn_layers=dn))
        return out

    def _placement(self, x, y):
        """Where the points lie: ``(top, tg, inside, cell)`` -- the index of the topmost layer that holds each point or
        -1, ``t ** g`` there (1 where the layer is constant or there is none), whether the point is inside the closed extent
        of the map, and ``(i0, j0, a, b)`` of the inside points (None without a map): the membership, ``t`` and the cell
        of :meth:`epsilon`."""
        x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
        top = np.full(x.shape, -1, dtype=np.int64)
        tg = np.ones(x.shape, dtype=np.float64)
        for l, (cx, cy, r_in, r_out, _, _, g, _) in enumerate(self._layers):
            dx, dy = x - cx, y - cy
            d2 = dx * dx + dy * dy
            inside = (r_in * r_in <= d2) & (d2 <= r_out * r_out)
            top[inside] = l
            if g > 0:
                t = np.minimum(np.maximum((np.sqrt(d2[inside]) - r_in) / (r_out - r_in), 0.0), 1.0)
                tg[inside] = np.power(t, g)
            else:
                tg[inside] = 1.0
        if self._map is None:
            return top, tg, np.zeros(x.shape, dtype=bool), None
        inside, cell = self._map_cells(x, y)
        return top, tg, inside, cell

    def _map_cells(self, x, y):
        """``inside`` (the points in the closed extent of the map) and ``(i0, j0, a, b)`` of those points."""
        E, x0, y0, dx, dy = self._map
        ny, nx = E.shape
        with np.errstate(invalid="ignore"):
            tx, ty = (x - x0) * (1.0 / dx), (y - y0) * (1.0 / dy)
            inside = (tx >= 0.0) & (tx <= nx - 1) & (ty >= 0.0) & (ty <= ny - 1)       # (False for a NaN)
        tx, ty = tx[inside], ty[inside]
        i0 = np.minimum(np.floor(tx).astype(np.int64), nx - 2)
        j0 = np.minimum(np.floor(ty).astype(np.int64), ny - 2)
        return inside, (i0, j0, tx - i0, ty - j0)

    def _paint_map(self, eps, x, y):
        """The bilinear interpolant of the map into ``eps`` at the points inside its closed extent."""
        E, x0, y0, dx, dy = self._map
        ny, nx = E.shape
        with np.errstate(invalid="ignore"):
            tx, ty = (x - x0) * (1.0 / dx), (y - y0) * (1.0 / dy)
            inside = (tx >= 0.0) & (tx <= nx - 1) & (ty >= 0.0) & (ty <= ny - 1)       # (False for a NaN)
        tx, ty = tx[inside], ty[inside]
        i0 = np.minimum(np.floor(tx).astype(np.int64), nx - 2)
        j0 = np.minimum(np.floor(ty).astype(np.int64), ny - 2)
        a, b = tx - i0, ty - j0
        a1, b1 = 1.0 - a, 1.0 - b
        lo = a1 * E[j0, i0] + a * E[j0, i0 + 1]
        hi = a1 * E[j0 + 1, i0] + a * E[j0 + 1, i0 + 1]
        eps[inside] = lo * b1 + hi * b


def _layer_pairs(v, nlayer: int, name: str) -> np.ndarray:
    """``v`` -- a number, ``(nlayer,)`` or ``(nlayer, 2)`` -- as a finite ``(nlayer, 2)`` float64 array."""
    try:
        a = np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number, ({nlayer},) or ({nlayer}, 2) finite numbers") from None
    if a.ndim == 0:
        a = np.full((nlayer, 2), float(a))
    elif a.shape == (nlayer,):
        a = np.repeat(a[:, None], 2, axis=1)
    elif a.shape != (nlayer, 2):
        raise ValueError(f"{name} must be a number, ({nlayer},) or ({nlayer}, 2) finite numbers, not shape {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name} must be finite")
    return np.ascontiguousarray(a, dtype=np.float64)


class ProfileTangent:
    """A first-order change of the permittivity VALUES of one :class:`IndexProfile` at fixed shapes: ``d_eps_background``,
    ``d_layers`` (nlayer, 2) = (d_eps_a, d_eps_b) per layer and, for a profile with a map, optionally ``d_map`` (ny, nx)
    on the profile's own pixel grid.  ``IndexProfile.epsilon`` is linear in exactly these values, so the tangent is
    itself a profile with the same layers and the same grid: :meth:`epsilon` is the change of ``profile.epsilon`` per
    unit step along it.  Made by ``IndexProfile.tangent_eps`` / ``tangent_index`` / ``unit_tangents``; bound to the profile
    that made it (``ValueError`` with another one).  A tangent without a map over a profile with one changes the
    interpolated background by ``d_eps_background`` inside the extent too."""

    def __init__(self, profile: IndexProfile, d_background=0.0, d_layers=0.0, d_map=None):
        if not isinstance(profile, IndexProfile):
            raise ValueError("profile must be an IndexProfile")
        self.profile = profile
        self._table_bytes = profile.table().tobytes()
        self._map_ref = profile.index_map
        self.d_eps_background = _number(d_background, "d_background")
        self.d_layers = _layer_pairs(d_layers, len(profile), "d_layers")
        for l, row in enumerate(profile.table()):
            if row[6] == 0 and self.d_layers[l, 0] != self.d_layers[l, 1]:
                raise ValueError(f"layer {l} is constant: its two tangent values must agree")
        self.d_map = None
        if d_map is not None:
            if profile.index_map is None:
                raise ValueError("d_map needs a profile with a map")
            shape = profile.index_map[0].shape
            try:
                m = np.array(d_map, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"d_map must have shape (ny, nx) = {shape}") from None
            if m.shape != shape:
                raise ValueError(f"d_map must have shape (ny, nx) = {shape}, not {m.shape}")
            if not np.all(np.isfinite(m)):
                raise ValueError("d_map must be finite")
            self.d_map = np.ascontiguousarray(m)
            self.d_map.setflags(write=False)
        self.d_layers.setflags(write=False)

    def check(self, profile: IndexProfile) -> "ProfileTangent":
        """``self`` if the tangent belongs to ``profile`` -- the same object, or the same table and map -- else
        ``ValueError``; also when the profile has gained a layer or another map since the tangent was made."""
        if not isinstance(profile, IndexProfile):
            raise ValueError("the tangent belongs to another index profile")
        m, mine = profile.index_map, self._map_ref
        same_map = (m is None and mine is None) or (m is not None and mine is not None and m[1:] == mine[1:] and
                                                    (m[0] is mine[0] or np.array_equal(m[0], mine[0])))
        if not (profile.table().tobytes() == self._table_bytes and same_map and
                profile.eps_background == self.profile.eps_background):
            raise ValueError("the tangent belongs to another index profile")
        return self

    def row(self) -> np.ndarray:
        """``(1 + 2 nlayer,)`` float64: ``d_eps_background``, then (d_eps_a, d_eps_b) per layer, as the C ABI takes it."""
        return np.concatenate([[self.d_eps_background], self.d_layers.reshape(-1)]).astype(np.float64)

    def scaled(self, factor: float) -> "ProfileTangent":
        """The tangent times ``factor``."""
        f = _number(factor, "factor")
        return ProfileTangent(self.profile, f * self.d_eps_background, f * self.d_layers,
                              None if self.d_map is None else f * self.d_map)

    def epsilon(self, x, y) -> np.ndarray:
        """``d eps`` at the points (float64, the shape of ``x``): ``d_a + (d_b - d_a) t ** g`` in the topmost layer that
        holds the point; otherwise the bilinear interpolant of ``d_map`` inside the extent of the map (or
        ``d_eps_background`` when the tangent has no map), and ``d_eps_background`` outside it -- membership, overwrite
        order, ``t``, ``g`` and bilinear weights of ``IndexProfile.epsilon``."""
        prof = self.check(self.profile).profile
        x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        top, tg, inside, cell = prof._placement(x, y)
        d = np.full(top.shape, self.d_eps_background, dtype=np.float64)
        if self.d_map is not None:
            i0, j0, a, b = cell
            a1, b1 = 1.0 - a, 1.0 - b
            E = self.d_map
            lo = a1 * E[j0, i0] + a * E[j0, i0 + 1]
            hi = a1 * E[j0 + 1, i0] + a * E[j0 + 1, i0 + 1]
            d[inside] = lo * b1 + hi * b
        lay = top >= 0
        da, db = self.d_layers[top[lay], 0], self.d_layers[top[lay], 1]
        d[lay] = da + (db - da) * tg[lay]
        return d


_PROFILED_CLASSES = {}


def _profiled_class(base_type):
    """The subclass of ``base_type`` that ProfiledGeometry objects of such a base belong to: one per base class."""
    if issubclass(base_type, ProfiledGeometry):
        return base_type
    kind = _PROFILED_CLASSES.get(base_type)
    if kind is None:
        kind = _PROFILED_CLASSES[base_type] = type("Profiled" + base_type.__name__, (ProfiledGeometry, base_type),
                                                    {"_base_type": base_type, "__module__": __name__})
    return kind


def _rebuild_profiled(base_type, state):
    """What copy and pickle call: an object of the profiled class of ``base_type`` with the attributes ``state``."""
    obj = object.__new__(_profiled_class(base_type))
    obj.__dict__.update(state)
    return obj


class ProfiledGeometry:
    """``ProfiledGeometry(base, profile, n_core=None, n_clad=None)``: a copy of the geometry ``base`` (an object of a
    subclass of its class: ``positions``, ``core_radii``, ``k0``, ``domain_radius``, the mesh recipe's inputs and the rest
    are kept) whose ``epsilon`` is the profile -- complex with zero imaginary part; the eigenpath reads the real part only
    -- and that carries it as ``index_profile``.  ``n_core`` (default: the profile's largest index) and ``n_clad``
    (default: its background) are what the reference's n_eff filters and the shift estimate read; ``positions`` /
    ``core_radii`` stay the discs that the in-core sums of the post-processing count.  ``base`` may itself be a
    ProfiledGeometry: the new profile replaces the old one.  The objects copy (``copy.copy``, ``copy.deepcopy``) and
    pickle like the base does.  A profile with neither layers nor a map is refused: that is no cross-section to solve."""

    def __new__(cls, base, profile=None, n_core=None, n_clad=None):
        obj = object.__new__(_profiled_class(type(base)))
        obj.__dict__.update(base.__dict__)                           # a shallow copy of the base, as copy.copy makes
        return obj

    def __reduce__(self):
        return _rebuild_profiled, (type(self)._base_type, dict(self.__dict__))

    def __init__(self, base, profile, n_core: Optional[float] = None, n_clad: Optional[float] = None):
        if not isinstance(profile, IndexProfile):
            raise ValueError("profile must be an IndexProfile")
        if len(profile) == 0 and profile.index_map is None:
            raise ValueError("the profile has no layers and no map")
        self.index_profile = profile
        self.n_core = profile.n_max if n_core is None else _index(n_core, "n_core")
        self.n_clad = profile.n_background if n_clad is None else _index(n_clad, "n_clad")
        self.delta_n = self.n_core - self.n_clad
        h = hashlib.sha256()
        h.update(str(getattr(base, "hash", "")).encode())
        h.update(profile.table().tobytes())
        h.update(f"{profile.eps_background!r}{self.n_core!r}{self.n_clad!r}".encode())
        if profile.index_map is not None:
            E, *grid = profile.index_map
            h.update(f"map{E.shape!r}{grid!r}".encode())
            h.update(E.tobytes())
        self._hash = h.hexdigest()[:20]

    def epsilon(self, x, y) -> np.ndarray:
        return self.index_profile.epsilon(x, y).astype(np.complex128)

    def __repr__(self) -> str:
        m = self.index_profile.index_map
        over = "" if m is None else f" over a {m[0].shape[1]} x {m[0].shape[0]} map"
        return (f"{type(self).__name__}({len(self.index_profile)} layers{over} on n={self.index_profile.n_background:.4f}, "
                f"n={self.n_core:.4f}/{self.n_clad:.4f})")


def index_profile_of(geometry) -> Optional[IndexProfile]:
    """The profile a geometry carries (``geometry.index_profile``), or None; ``ValueError`` if it is no IndexProfile."""
    prof = getattr(geometry, "index_profile", None)
    if prof is not None and not isinstance(prof, IndexProfile):
        raise ValueError("geometry.index_profile must be an IndexProfile")
    return prof


def reject_profile(geometry, what: str) -> None:
    """``ValueError`` when ``geometry`` carries an index profile: ``what`` splits the plane into core discs and cladding
    and would compute with the wrong material map."""
    if geometry is not None and getattr(geometry, "index_profile", None) is not None:
        raise ValueError(f"{what} assumes two material regions (core discs on a cladding) and the geometry carries an index "
                         "profile: use ModeFields.profile_grams, the Grams of a profile solve, and profile_dispersion, "
                         "profile_sensitivity, profile_bend_response of profile_response")


__all__ = ["IndexProfile", "ProfileTangent", "ProfiledGeometry", "index_profile_of", "reject_profile", "MAX_LAYERS"]
