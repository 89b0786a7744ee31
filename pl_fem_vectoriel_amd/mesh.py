"""Triangle meshes for the eigenmode path (host side, outside the timed hot path).

The solver only needs ``mesh.p`` (2, nv) float64 and ``mesh.t`` (3, ne) int; the
reference hands it a scikit-fem ``MeshTri`` built by ``MeshGenerator._generate_mesh``
(reference ``mesh.py:222-340``).  This module provides

* :class:`TriMesh`          — the duck-type (``p``, ``t``, ``refined()``), columns of ``t`` sorted
  ascending as ``MeshTri`` does on construction;
* :func:`lantern_point_cloud` — the reference point recipe ``mesh.py:232-297`` (Cartesian grid +
  per-core polar rings + PML ring, radius filter, round(8), unique);
* :func:`generate_mesh`     — recipe -> ``scipy.spatial.Delaunay('QJ Pp')`` (``mesh.py:303``) ->
  drop zero-area triangles -> ``levels`` uniform red refinements.

Deliberate deviations from the reference, both documented in DESIGN.md:

* zero-area triangles produced by ``QJ`` on collinear hull points are dropped
  (``|det J| < 1e-10``); the reference would feed them to the P2 assembly and obtain Inf/NaN;
* the number of uniform refinements is an explicit argument, because the thresholds the reference
  reads (``config.mesh_min_points`` / ``mesh_target_points``, ``mesh.py:313-314``) live in a
  ``SimulationConfig`` that is absent from the reference checkout.
"""
from __future__ import annotations

import hashlib
import logging
import pickle
from collections import OrderedDict
from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import numpy as np

logger = logging.getLogger(__name__)

_LOCAL_EDGES = ((0, 1), (1, 2), (0, 2))


class TriMesh:
    """``p`` (2, nv) float64, ``t`` (3, ne) int32 with every column sorted ascending."""

    def __init__(self, p, t):
        self.p = np.ascontiguousarray(np.asarray(p, dtype=np.float64))
        t = np.sort(np.asarray(t, dtype=np.int64), axis=0)
        if self.p.ndim != 2 or self.p.shape[0] != 2 or t.ndim != 2 or t.shape[0] != 3:
            raise ValueError("mesh.p must be (2, nv) and mesh.t (3, ne)")
        if t.size and (t.min() < 0 or t.max() >= self.p.shape[1]):
            raise ValueError("mesh.t refers to a vertex outside mesh.p")
        self.t = np.ascontiguousarray(t.astype(np.int32))

    @property
    def nvertices(self) -> int:
        return self.p.shape[1]

    @property
    def nelements(self) -> int:
        return self.t.shape[1]

    def edges(self):
        """Unique sorted vertex pairs (2, nedges) in lexicographic order and ``t2f`` (3, ne)."""
        t = self.t.astype(np.int64)
        pairs = np.hstack([t[[i, j]] for (i, j) in _LOCAL_EDGES])
        nv = self.p.shape[1]
        key = pairs[0] * np.int64(nv) + pairs[1]
        ukey, inv = np.unique(key, return_inverse=True)
        return np.vstack([ukey // nv, ukey % nv]), inv.reshape(3, t.shape[1])

    def refined(self, times: int = 1) -> "TriMesh":
        """Uniform red refinement; new vertex id = nv + edge id (as ``MeshTri.refined()``, ``mesh.py:321``)."""
        from . import _native

        m = self
        for _ in range(int(times)):
            p2, t2 = _native.mesh_refine(m.p, m.t)        # native host code (plfem_mesh_refine)
            m = TriMesh(p2, t2)
        return m

    def refined_marked(self, marked):
        """Longest-edge bisection of the elements flagged in ``marked`` (ne,) with a conformity closure
        (``plfem_mesh_refine_marked``): ``(TriMesh, parent)``, ``parent`` (ne2,) int32 the element each new one came from.
        Old vertices keep their ids; no flag set gives the mesh back."""
        from . import _native

        p2, t2, parent = _native.mesh_refine_marked(self.p, self.t, marked)
        return TriMesh(p2, t2), parent


def lantern_point_cloud(geometry, refinement: float = 1.0) -> np.ndarray:
    """Point recipe of ``MeshGenerator._generate_mesh`` (reference ``mesh.py:232-297``) -> (2, npts)."""
    R = float(geometry.domain_radius)
    n_base = max(int(25 + 20 * refinement), 16)
    g = np.linspace(-R, R, n_base, dtype=np.float64)
    X, Y = np.meshgrid(g, g)
    chunks = [np.vstack([X.ravel(), Y.ravel()])]

    theta = np.linspace(0, 2 * np.pi, max(int(16 * refinement), 12), endpoint=False)
    positions = np.atleast_2d(np.asarray(getattr(geometry, "positions",
                                                 getattr(geometry, "core_positions", np.zeros((1, 2))))))
    radii = np.asarray(geometry.core_radii)
    n_int = max(int(14 * refinement), 10)
    n_itf = max(int(18 * refinement), 14)
    for (cx, cy), r in zip(positions, radii):
        for rr in (np.linspace(0, r * 0.95, n_int), np.linspace(r * 0.90, r * 1.20, n_itf)):
            Rg, Tg = np.meshgrid(rr, theta)
            chunks.append(np.vstack([cx + Rg.ravel() * np.cos(Tg.ravel()),
                                     cy + Rg.ravel() * np.sin(Tg.ravel())]))
    pml_start = R - geometry.pml_thickness * 1.1
    if pml_start > 0:
        th = np.linspace(0, 2 * np.pi, max(int(36 * refinement), 24), endpoint=False)
        rr = np.linspace(pml_start, R * 0.98, max(int(18 * refinement), 12))
        Rg, Tg = np.meshgrid(rr, th)
        chunks.append(np.vstack([Rg.ravel() * np.cos(Tg.ravel()), Rg.ravel() * np.sin(Tg.ravel())]))
    pts = np.hstack(chunks)
    pts = pts[:, np.linalg.norm(pts, axis=0) <= R * 1.01]
    pts = np.round(pts.T, decimals=8).T
    return np.unique(pts, axis=1)


def generate_mesh(geometry, refinement: float = 1.0, levels: int = 1, drop_tol: float = 1e-10) -> TriMesh:
    """Synthetic lantern mesh: recipe -> Delaunay('QJ Pp') -> drop |det J| < tol -> red-refine."""
    from scipy.spatial import Delaunay

    pts = lantern_point_cloud(geometry, refinement)
    tri = Delaunay(pts.T, qhull_options="QJ Pp")
    p = tri.points.T
    t = tri.simplices.T
    p0, p1, p2 = p[:, t[0]], p[:, t[1]], p[:, t[2]]
    det = (p1[0] - p0[0]) * (p2[1] - p0[1]) - (p2[0] - p0[0]) * (p1[1] - p0[1])
    t = t[:, np.abs(det) >= drop_tol]
    return TriMesh(p, t).refined(levels)


@dataclass
class SimulationConfig:
    """Stand-in for the four fields ``MeshGenerator`` reads of the reference's ``SimulationConfig``
    (``mesh.py:109,126,186,313-314``).  The real class is absent from the reference checkout
    (SURVEY.md F6), so the VALUES below are this build's choice: with them the north-star geometry at
    ``refinement=1.0`` gets exactly one uniform refinement (5 691 -> 22 694 points = config C1)."""
    enable_mesh_cache: bool = True
    cache_max_size: int = 150
    mesh_min_points: int = 20000
    mesh_target_points: int = 60000


class MeshGenerator:
    """Mesh producer with the reference's class surface (``mesh.py:49-416``): ``generate`` returns
    ``(mesh, basis)`` and keeps a class-level cache keyed by geometry hash + refinement with FIFO
    eviction under an entry limit and a memory limit, moved to the end on a hit.

    Uniform refinements run in the library's native host code (``plfem_mesh_refine``); the
    ``mesh.refined(0.5)`` semi-refinement of ``mesh.py:330-332`` is not reproduced (a float is not a
    refinement count in scikit-fem)."""

    _cache: "OrderedDict" = OrderedDict()
    _cache_hits: int = 0
    _cache_misses: int = 0
    _cache_max_size: int = 150
    _cache_max_memory_mb: float = 500.0
    MAX_REFINEMENT_ITERATIONS = 5

    @classmethod
    def generate(cls, geometry, refinement: float = 1.0, config: Optional[SimulationConfig] = None):
        config = config or SimulationConfig()
        key = cls._create_cache_key(geometry, refinement)
        if config.enable_mesh_cache and key in cls._cache:
            cls._cache_hits += 1
            cls._cache.move_to_end(key)
            return cls._cache[key]
        cls._cache_misses += 1
        value = cls._generate_mesh(geometry, refinement, config)
        if config.enable_mesh_cache:
            cls._add_to_cache(key, value, config)
        return value

    @classmethod
    def _create_cache_key(cls, geometry, refinement: float) -> str:
        h = hashlib.sha256()                                          # mesh.py:144-165
        if hasattr(geometry, "hash"):
            h.update(geometry.hash.encode())
        else:
            pos = getattr(geometry, "positions", getattr(geometry, "core_positions", np.zeros((1, 2))))
            h.update(np.asarray(pos).tobytes())
            h.update(np.asarray(geometry.core_radii).tobytes())
            h.update(f"{getattr(geometry, 'n_core', getattr(geometry, 'core_index', 1.5)):.6f}".encode())
        h.update(f"{refinement:.4f}".encode())
        h.update(str(geometry.n_cores).encode())
        h.update(f"{geometry.pml_thickness:.2f}".encode())
        h.update(str(geometry.use_complex_pml).encode())
        return h.hexdigest()[:24]

    @classmethod
    def _estimate_cache_memory_mb(cls) -> float:
        return sum(m.p.nbytes + m.t.nbytes for m, _ in cls._cache.values()) / 1024 ** 2

    @classmethod
    def _add_to_cache(cls, key, value, config: SimulationConfig):
        mesh, _ = value
        size_mb = (mesh.p.nbytes + mesh.t.nbytes) / 1024 ** 2
        while cls._cache and (len(cls._cache) >= config.cache_max_size
                              or cls._estimate_cache_memory_mb() + size_mb > cls._cache_max_memory_mb):
            cls._cache.popitem(last=False)                            # FIFO eviction, mesh.py:186-198
        cls._cache[key] = value

    @classmethod
    def _generate_mesh(cls, geometry, refinement: float, config: SimulationConfig):
        from . import _native
        from .solver_fem import P2BasisView

        mesh = generate_mesh(geometry, refinement, levels=0)
        it = 0
        while mesh.nvertices < config.mesh_min_points and it < cls.MAX_REFINEMENT_ITERATIONS:   # mesh.py:317-327
            p2, t2 = _native.mesh_refine(mesh.p, mesh.t)
            mesh = TriMesh(p2, t2)
            it += 1
            if mesh.nvertices > config.mesh_target_points * 2.5:
                break
        basis = P2BasisView(_native.Symbolic(mesh.p, mesh.t))          # Basis(mesh, ElementTriP2()), mesh.py:335
        return mesh, basis

    @classmethod
    def clear_cache(cls):
        cls._cache.clear()
        cls._cache_hits = 0
        cls._cache_misses = 0

    @classmethod
    def get_cache_stats(cls) -> dict:
        total = cls._cache_hits + cls._cache_misses
        return {"size": len(cls._cache), "hits": cls._cache_hits, "misses": cls._cache_misses,
                "hit_rate": cls._cache_hits / total if total else 0.0, "memory_mb": cls._estimate_cache_memory_mb(),
                "max_size": cls._cache_max_size, "max_memory_mb": cls._cache_max_memory_mb}

    @classmethod
    def print_cache_stats(cls):
        """Cache statistics as a small table on stdout (``mesh.py:371-383``)."""
        st = cls.get_cache_stats()
        bar = "=" * 60
        print(bar)
        print("MESH CACHE")
        print(bar)
        print(f"entries  : {st['size']} / {st['max_size']}")
        print(f"memory   : {st['memory_mb']:.1f} / {st['max_memory_mb']:.1f} MB")
        print(f"hits     : {st['hits']:,}")
        print(f"misses   : {st['misses']:,}")
        print(f"hit rate : {st['hit_rate'] * 100:.1f}%")
        print(bar)

    @classmethod
    def save_cache(cls, filepath):
        """Writes the cached meshes and the hit / miss counters to ``filepath`` (``mesh.py:386-397``).  What goes to disk is
        the mesh arrays ``(p, t)`` per key: the P2 basis view of an entry wraps a handle of the native library and is
        rebuilt by ``load_cache``."""
        filepath = Path(filepath)
        with open(filepath, "wb") as f:
            pickle.dump({"meshes": {k: (np.asarray(m.p), np.asarray(m.t)) for k, (m, _) in cls._cache.items()},
                         "hits": cls._cache_hits, "misses": cls._cache_misses}, f, protocol=pickle.HIGHEST_PROTOCOL)
        logger.info("mesh cache written: %s (%.1f MB)", filepath, cls._estimate_cache_memory_mb())

    @classmethod
    def load_cache(cls, filepath):
        """Replaces the cache by the contents of a ``save_cache`` file; a missing file is a warning, not an error
        (``mesh.py:400-416``)."""
        from . import _native
        from .solver_fem import P2BasisView

        filepath = Path(filepath)
        if not filepath.exists():
            logger.warning("no mesh cache file at %s", filepath)
            return
        with open(filepath, "rb") as f:
            data = pickle.load(f)
        cache = OrderedDict()
        for k, (p, t) in data["meshes"].items():
            mesh = TriMesh(p, t)
            cache[k] = (mesh, P2BasisView(_native.Symbolic(mesh.p, mesh.t)))
        cls._cache = cache
        cls._cache_hits = data["hits"]
        cls._cache_misses = data["misses"]
        logger.info("mesh cache read: %d entries, %.1f MB", len(cls._cache), cls._estimate_cache_memory_mb())


class MeshQualityAnalyzer:
    """Triangle quality metrics (``mesh.py:419-496``)."""

    @staticmethod
    def analyze(mesh) -> dict:
        if mesh is None:
            return {}
        p, t = mesh.p, mesh.t
        v1 = p[:, t[1]] - p[:, t[0]]
        v2 = p[:, t[2]] - p[:, t[0]]
        areas = 0.5 * np.abs(v1[0] * v2[1] - v1[1] * v2[0])
        lens = np.array([np.linalg.norm(p[:, t[(i + 1) % 3]] - p[:, t[i]], axis=0) for i in range(3)])
        aspect = lens.max(0) / (lens.min(0) + 1e-12)
        quality = 4 * np.sqrt(3) * areas / (np.sum(lens ** 2, axis=0) + 1e-12)
        cosines = []
        for i in range(3):
            a2, b2, c2 = lens[(i + 1) % 3] ** 2, lens[(i + 2) % 3] ** 2, lens[i] ** 2
            cosines.append((a2 + b2 - c2) / (2 * np.sqrt(a2 * b2) + 1e-12))
        min_angle = np.degrees(np.arccos(np.clip(np.max(cosines, axis=0), -1, 1)))
        return {"n_points": p.shape[1], "n_elements": t.shape[1],
                "area_min": float(areas.min()), "area_max": float(areas.max()), "area_mean": float(areas.mean()),
                "aspect_min": float(aspect.min()), "aspect_max": float(aspect.max()), "aspect_mean": float(aspect.mean()),
                "quality_min": float(quality.min()), "quality_max": float(quality.max()),
                "quality_mean": float(quality.mean()), "min_angle_min": float(min_angle.min()),
                "min_angle_mean": float(min_angle.mean()),
                "poor_quality_frac": float(np.sum(quality < 0.35) / len(quality)),
                "bad_aspect_frac": float(np.sum(aspect > 8.0) / len(aspect)),
                "small_angle_frac": float(np.sum(min_angle < 20.0) / len(min_angle))}

    @staticmethod
    def print_analysis(mesh, logger_inst=None):
        """The metrics of ``analyze`` as log lines (``mesh.py:499-524``)."""
        log = logger_inst or logger
        m = MeshQualityAnalyzer.analyze(mesh)
        if not m:
            log.warning("invalid mesh: nothing to analyse")
            return
        bar = "=" * 70
        log.info(bar)
        log.info("MESH QUALITY")
        log.info(bar)
        log.info(f"points       : {m['n_points']:,}")
        log.info(f"triangles    : {m['n_elements']:,}")
        log.info(f"area         : [{m['area_min']:.2e}, {m['area_max']:.2e}] (mean {m['area_mean']:.2e})")
        log.info(f"aspect ratio : [{m['aspect_min']:.2f}, {m['aspect_max']:.2f}] (mean {m['aspect_mean']:.2f})")
        log.info(f"quality      : [{m['quality_min']:.3f}, {m['quality_max']:.3f}] (mean {m['quality_mean']:.3f}; 1 = equilateral)")
        log.info(f"smallest angle: {m['min_angle_min']:.1f} deg (mean {m['min_angle_mean']:.1f} deg)")
        log.info(f"quality < 0.35 : {m['poor_quality_frac'] * 100:.1f}%")
        log.info(f"aspect > 8     : {m['bad_aspect_frac'] * 100:.1f}%")
        log.info(f"angle < 20 deg : {m['small_angle_frac'] * 100:.1f}%")
        log.info(bar)

    @staticmethod
    def validate_mesh_quality(mesh, strict: bool = False):
        """``(ok, message)``: the acceptance rule of ``mesh.py:527-568`` -- smallest angle >= 10 deg, aspect ratio <= 20, at
        most 20 % of the elements below quality 0.35; with ``strict`` also smallest angle >= 20 deg, mean aspect ratio <= 3
        and mean quality >= 0.7."""
        m = MeshQualityAnalyzer.analyze(mesh)
        if not m:
            return False, "invalid mesh (analysis failed)"
        issues = []
        if m["min_angle_min"] < 10.0:
            issues.append(f"critical smallest angle: {m['min_angle_min']:.1f} deg < 10 deg")
        if m["aspect_max"] > 20.0:
            issues.append(f"excessive aspect ratio: {m['aspect_max']:.1f} > 20")
        if m["poor_quality_frac"] > 0.2:
            issues.append(f"too many poor-quality elements: {m['poor_quality_frac'] * 100:.0f}%")
        if strict:
            if m["min_angle_min"] < 20.0:
                issues.append(f"[strict] small smallest angle: {m['min_angle_min']:.1f} deg")
            if m["aspect_mean"] > 3.0:
                issues.append(f"[strict] high mean aspect ratio: {m['aspect_mean']:.1f}")
            if m["quality_mean"] < 0.7:
                issues.append(f"[strict] low mean quality: {m['quality_mean']:.2f}")
        if issues:
            return False, "; ".join(issues)
        return True, "mesh quality acceptable"


def unit_square_mesh(n: int = 4) -> TriMesh:
    """Structured test mesh of [0,1]^2 with 2 n^2 triangles (used by unit tests / smoke)."""
    g = np.linspace(0.0, 1.0, n + 1)
    X, Y = np.meshgrid(g, g)
    p = np.vstack([X.ravel(), Y.ravel()])
    idx = np.arange((n + 1) * (n + 1)).reshape(n + 1, n + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    t = np.hstack([np.vstack([a, b, d]), np.vstack([a, d, c])])
    return TriMesh(p, t)
