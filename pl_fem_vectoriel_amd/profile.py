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
                         "profile: use ModeFields.profile_grams, the Grams of a profile solve")


__all__ = ["IndexProfile", "ProfiledGeometry", "index_profile_of", "reject_profile", "MAX_LAYERS"]
