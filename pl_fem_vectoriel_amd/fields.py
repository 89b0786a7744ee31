"""Mode fields at arbitrary points, and overlaps of modes across meshes, on the GPU.

The solvers return their modes as P2 DOF vectors: ``TrueVectorialMaxwellSolver`` records hold ``Ex_dofs`` / ``Ey_dofs``
(Hx / Hy on the interior DOFs), ``ScalarHelmholtzSolver`` records ``field_vector`` on all N DOFs.  In the reference the
same vectors sit next to a scikit-fem ``Basis`` whose ``probes`` / ``interpolate`` turn them back into fields; here that
is done by ``libplfem_hip.so`` (``include/plfem.h``, "Mode fields at arbitrary points"):

* :class:`ModeFields` -- point location in the mesh (a uniform cell grid built lazily on the mesh's analysis) and P2
  evaluation of many modes at many points in one kernel (``plfem_sample_fields``);
* :func:`mode_overlap` -- ``O[i, j] = integral over mesh B of w(x) u_a,i . u_b,j`` with mesh B's six-point rule, A's
  values located and evaluated inside the kernel (``plfem_field_overlap``);
* :func:`mode_overlap_poses` -- the same under a table of poses (shift, rotation, magnification) of mesh A relative to
  mesh B, applied to B's quadrature points inside the kernel, the modes staged once (``plfem_field_overlap_posed``):
  what :mod:`.splice` builds splice maps and taper steps from;
* :meth:`ModeFields.grams` -- the k x k Grams of one mesh's modes under the assembly's element forms, split by material
  region (``plfem_mode_grams``): what :mod:`.dispersion` builds the group index and the k0-derivative coupling from;
* :meth:`ModeFields.moment_grams` -- the region Grams weighted by the coordinates of the quadrature point
  (``plfem_moment_grams``): what :mod:`.bend` builds bend-induced index shifts, mode mixing and beam widths from;
* :meth:`ModeFields.indicators` -- per-element a-posteriori error indicators of the modes, element residual plus flux
  jumps (``plfem_mode_indicators``): what :mod:`.adapt` marks and refines a mesh with;
* :meth:`ModeFields.sample_e`, :meth:`ModeFields.flux_grams` -- the electric field and axial Poynting flux of vectorial
  modes at points (``plfem_sample_efields``) and the Grams their cross powers are built from (``plfem_flux_grams``): what
  :mod:`.power` builds modal power, power confinement and power orthogonality from;
* :meth:`ModeFields.velocity_grams` -- the first-order change of the projected forms when the mesh moves with a vertex
  velocity field and carries its material along (``plfem_velocity_grams``): what :mod:`.shape` builds the sensitivities
  of n_eff to core position, radius and ellipticity from;
* :func:`flux_overlap_poses` -- the four beta-free sums of the E x H cross flux of two vectorial mode sets on two meshes
  under a table of poses (``plfem_flux_overlap_posed``): what :mod:`.splice` builds power-normalised splice maps and
  vectorial taper steps from;
* :meth:`ModeFields.quartic` -- the packed overlap of products of four modes on a 16-point degree-8 rule
  (``plfem_mode_quartic``): what :mod:`.nonlinear` builds the nonlinear coupling tensor, A_eff and gamma from;
* :meth:`ModeFields.project` -- the projection of the modes on plane waves and Gaussian beams, fields that separate in
  x and y, on the same rule (``plfem_mode_project``): what :mod:`.launch` builds far fields and launch maps from;
* :meth:`ModeFields.project_sampled` -- the projection of the modes on a batch of complex images on a pixel grid (PSF
  frames, speckle, measured near fields, beam-propagation output), interpolated bilinearly at the points of the same
  rule (``plfem_mode_project_sampled``): what :func:`.launch.field_coupling` builds response maps from;
* :meth:`ModeFields.index_map_densities` -- the derivative of the modes' weighted Grams in every pixel of a profile's
  sampled map, one pass over the quadrature points (``plfem_index_map_gradients``): what :mod:`.map_gradient` builds the
  gradient of every n_eff in every pixel from.

Containment (``PLFEM_LOC_TOL``): a point is inside an element when every barycentric coordinate is >= -1e-10 (minus
that coordinate's floating-point rounding bound, which matters on sliver elements only); when
several elements contain it the smallest element id wins; a point inside none gets element -1 and value 0.
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Dict, Optional, Sequence

import numpy as np

from . import _native
from .profile import ProfileTangent, index_profile_of, reject_profile
from .solver_fem import _core_table, mesh_key

LOC_TOL = 1e-10                    # PLFEM_LOC_TOL of include/plfem.h
GRAM_NAMES = {"vectorial": ("M_core", "M_clad", "K_core", "K_clad", "D"), "scalar": ("M_core", "M_clad", "S")}
CORE_GRAM_NAMES = {"vectorial": ("Mx", "My", "K"), "scalar": ("M",)}
PROFILE_GRAM_NAMES = {"vectorial": ("M", "M_w", "K_w", "D"), "scalar": ("M", "M_w", "S")}
FLUX_GRAM_NAMES = ("M_w_core", "M_w_rest", "G_w_core", "G_w_rest")      # vectorial records only
MOMENT_GRAM_NAMES = {"vectorial": ("M_core_X", "M_core_Y", "M_clad_X", "M_clad_Y", "K_core_X", "K_core_Y", "K_clad_X",
                                   "K_clad_Y", "M_XX", "M_XY", "M_YY"),
                     "scalar": ("M_core_X", "M_core_Y", "M_clad_X", "M_clad_Y", "M_XX", "M_XY", "M_YY")}
VELOCITY_GRAM_NAMES = {"vectorial": ("dK_w", "dD", "dM", "dM_w"), "scalar": ("dS", "dM", "dM_w")}
VELOCITY_MAX = 256                 # VG_MAX of csrc/kernels_fields.hip: velocities per call of plfem_velocity_grams
FLUX_OVERLAP_NAMES = ("MA", "GA", "MB", "GB")                           # plfem_flux_overlap_posed, per pose
POSE_MAX_CHUNK_PAIRS = 256         # POSE_MAX_PAIRS of csrc/kernels_fields.hip: pairs of 32-mode chunks per posed call
FLUX_POSE_MAX_CHUNK_PAIRS = 64     # FLUX_POSE_MAX_PAIRS: the same per posed flux call
TANGENT_MAX = 256                  # TAN_MAX of csrc/kernels_fields.hip: tangents per call of plfem_profile_tangent_grams
TANGENT_MAPS = 8                   # TAN_MAPS: tangent maps per call
MAP_GRADIENT_MAX = 256             # MAPG_KMAX: fields per call of plfem_index_map_gradients
MAP_GRADIENT_RESULT = 1 << 27      # MAPG_MAX_RESULT: doubles of one call's result
PROJECT_TILE = (8, 8)             # PJ_X, PJ_Y of csrc/kernels_fields.hip: x- and y-factors per workgroup tile
PROJECT_MAX_FACTORS = 4096         # PJ_LMAX
PROJECT_SAMPLED_TILE = 32          # PS_F: frames per workgroup tile of the sampled projection
PROJECT_SAMPLED_MAX_FRAMES = 4096  # PS_FRAMES: frames per call of plfem_mode_project_sampled
PROJECT_SAMPLED_MAX_PIXELS = 8192  # PS_NMAX: pixels per axis


def _grid_axis(v, name: str) -> tuple:
    """A pixel axis: 2 .. 8192 finite, ascending, uniformly spaced numbers (every step within 1e-12 of the span of the
    mean step).  Returns (axis, step) with ``step = (v[-1] - v[0]) / (n - 1)``."""
    try:
        a = np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a 1-D array of finite numbers") from None
    if a.ndim != 1 or not 2 <= a.size <= PROJECT_SAMPLED_MAX_PIXELS or not np.all(np.isfinite(a)):
        raise ValueError(f"{name} must be a 1-D array of 2 to {PROJECT_SAMPLED_MAX_PIXELS} finite numbers")
    span = float(a[-1] - a[0])
    step = span / (a.size - 1)
    if not (np.isfinite(span) and step > 0 and np.isfinite(1.0 / step)):
        raise ValueError(f"{name} must be ascending with a finite step whose inverse is finite")
    if np.any(np.abs(np.diff(a) - step) > 1e-12 * span):
        raise ValueError(f"{name} must be uniformly spaced and ascending: every step within 1e-12 (x[-1] - x[0]) of the mean step")
    return a, step


def _frames(frames, nx: int, ny: int) -> np.ndarray:
    """Sampled fields as complex128 (nf, ny, nx); a single (ny, nx) image is one frame."""
    try:
        f = np.asarray(frames)
        if f.dtype.kind not in "biufc":
            raise TypeError
        f = f.astype(np.complex128, copy=False)
    except (TypeError, ValueError):
        raise ValueError("frames must be a real or complex array of shape (nf, ny, nx) or (ny, nx)") from None
    if f.ndim == 2:
        f = f[None]
    if f.ndim != 3 or f.shape[1:] != (ny, nx):
        raise ValueError(f"frames must have shape (nf, {ny}, {nx}) or ({ny}, {nx}) for these axes, got {np.shape(frames)}")
    return f


def _mesh_arrays(mesh):
    p = np.asarray(getattr(mesh, "p", None) if mesh is not None else None)
    t = np.asarray(getattr(mesh, "t", None) if mesh is not None else None)
    if p.ndim != 2 or p.shape[0] != 2 or t.ndim != 2 or t.shape[0] != 3:
        raise ValueError("mesh must have p (2, nv) and t (3, ne)")
    return p, t


def _factors(fac, name: str) -> np.ndarray:
    """A factor table (l, 3) = (c, s, kappa) per row, 1 <= l <= 4096, finite, s >= 0, as contiguous float64."""
    try:
        f = np.ascontiguousarray(np.asarray(fac, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be an array of shape (l, 3): (c, s, kappa) per factor") from None
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"{name} must be an array of shape (l, 3): (c, s, kappa) per factor")
    if not 1 <= f.shape[0] <= PROJECT_MAX_FACTORS:
        raise ValueError(f"{name} must hold between 1 and {PROJECT_MAX_FACTORS} factors, got {f.shape[0]}")
    if not np.all(np.isfinite(f)) or np.any(f[:, 1] < 0):
        raise ValueError(f"every factor of {name} must be finite with s >= 0")
    return f


def _records(modes) -> tuple:
    """(kind, values (ncomp, k, n) float64, beta (k,)) of a list of mode records; kind is None for an empty list."""
    if isinstance(modes, dict):
        raise ValueError("modes must be a list of mode records, not one record")
    modes = list(modes)
    if not modes:
        return None, None, None
    kinds = set()
    for m in modes:
        if not hasattr(m, "keys"):
            raise ValueError("every mode must be a record (dict) of a solver")
        if "Ex_dofs" in m and "Ey_dofs" in m:
            kinds.add("vectorial")
        elif "field_vector" in m:
            kinds.add("scalar")
        else:
            raise ValueError("a mode record needs 'Ex_dofs' / 'Ey_dofs' (vectorial) or 'field_vector' (scalar)")
    if len(kinds) > 1:
        raise ValueError("vectorial and scalar mode records cannot be mixed")
    kind = kinds.pop()
    cols = ("Ex_dofs", "Ey_dofs") if kind == "vectorial" else ("field_vector",)
    comps = []
    for c in cols:
        vs = [np.asarray(m[c]) for m in modes]
        if any(v.ndim != 1 for v in vs) or len({v.shape[0] for v in vs}) != 1:
            raise ValueError(f"'{c}' vectors must be 1-D and of one length")
        if any(np.iscomplexobj(v) for v in vs):
            raise NotImplementedError("complex fields: the solvers of this package return real vectors")
        comps.append(np.stack(vs).astype(np.float64, copy=False))
    if comps[-1].shape != comps[0].shape:
        raise ValueError("'Ex_dofs' and 'Ey_dofs' must have the same length")
    vals = np.ascontiguousarray(np.stack(comps))
    beta = np.array([float(m.get("beta", np.nan)) for m in modes], dtype=np.float64)
    return kind, vals, beta


class ModeFields:
    """Point evaluation of the modes of one mesh.

    ``ModeFields(mesh, device=None, solver=None)``: the mesh-only analysis is taken from ``solver``'s cache when it
    holds this mesh (vectorial analysis), otherwise built here (host, a few ms); the locator grid is built on the host
    on first use and uploaded with the mesh's index arrays to the device (``plfem_locator_create``).  Argument errors
    raise ``ValueError`` before anything touches the device."""

    CHUNK_BYTES = 256 << 20        # device memory of one chunk of sampled values

    def __init__(self, mesh, device: Optional[int] = None, solver=None):
        p, t = _mesh_arrays(mesh)
        self.mesh = mesh
        self.device = device
        sym = None
        if solver is not None:
            ent = getattr(solver, "_cache", {}).get(mesh_key(mesh))
            if ent is not None and ent["sym"].dofs_per_node == 2 and ent["sym"].info["nsolve"] < ent["sym"].N:
                sym = ent["sym"]
        self.sym = sym if sym is not None else _native.Symbolic(p, t)
        self.N, self.nsolve, self.ne = self.sym.N, self.sym.nsolve, self.sym.ne
        self.nv = int(p.shape[1])
        self.bbox = (float(p[0].min()), float(p[0].max()), float(p[1].min()), float(p[1].max()))
        self._loc = None
        self._mem = None
        self._stats = None

    # -- host-side -------------------------------------------------------------------------------------------
    @property
    def stats(self) -> Dict:
        """Locator grid statistics (built on the host on first request): cells, mean / max candidates per cell."""
        if self._stats is None:
            g, s = self.sym.array("loc_grid"), self.sym.array("loc_stats")
            self._stats = {"nx": int(g[4]), "ny": int(g[5]), "cells": int(s[0]), "mean_candidates": float(s[1]),
                           "max_candidates": int(s[2]), "t_build": float(s[3])}
        return self._stats

    def _check_records(self, modes):
        kind, vals, beta = _records(modes)
        if kind == "vectorial" and vals.shape[2] != self.nsolve:
            raise ValueError(f"'Ex_dofs' / 'Ey_dofs' must have one entry per interior P2 DOF of the mesh ({self.nsolve}), "
                             f"got {vals.shape[2]}")
        if kind == "scalar" and vals.shape[2] != self.N:
            raise ValueError(f"'field_vector' must have one entry per P2 DOF of the mesh ({self.N}), got {vals.shape[2]}")
        return kind, vals, beta

    # -- device ----------------------------------------------------------------------------------------------
    def _ensure_locator(self):
        if self._loc is not None:
            return
        import torch
        lib = _native.load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: mode fields are evaluated on the GPU only")
        dev = torch.cuda.current_device() if self.device is None else int(self.device)
        self.tdev = torch.device("cuda", dev)
        self.stream = torch.cuda.current_stream(self.tdev)
        need = ctypes.c_int64(0)
        rc = lib.plfem_locator_bytes(self.sym._h, ctypes.byref(need))
        if rc != _native.PLFEM_OK:
            raise RuntimeError(f"plfem_locator_bytes failed ({rc})")
        self._mem = _native.device_scratch(int(need.value) + 256, self.tdev)
        aligned = (self._mem.data_ptr() + 255) & ~255
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        rc = lib.plfem_locator_create(self.sym._h, dev, ctypes.c_void_p(self.stream.cuda_stream), ctypes.c_void_p(aligned),
                                      ctypes.c_int64(int(need.value)), ctypes.byref(h), err, 512)
        if rc != _native.PLFEM_OK:
            raise RuntimeError(f"plfem_locator_create failed ({rc}): {err.value.decode()}")
        self._lib = lib
        self._loc = h
        self.device = dev

    def _check(self, rc, what):
        if rc != _native.PLFEM_OK:
            msg = self._lib.plfem_locator_last_error(self._loc).decode()
            raise (ValueError if rc == _native.PLFEM_EINVAL else RuntimeError)(f"{what} failed ({rc}): {msg}")

    def _stage(self, vals):
        """Host (ncomp, k, n) -> device, DOF-major (ncomp, n, k) (``plfem_stage_modes``)."""
        import torch
        ncomp, k, n = vals.shape
        with torch.cuda.stream(self.stream):
            src = torch.from_numpy(vals).to(self.tdev)
            dst = _native.device_output((ncomp, n, k), torch.float64, self.tdev)
            self._check(self._lib.plfem_stage_modes(self._loc, ncomp, k, n, ctypes.c_void_p(src.data_ptr()),
                                                    ctypes.c_void_p(dst.data_ptr())), "plfem_stage_modes")
        return dst, src

    def _checked(self, modes):
        """:meth:`_check_records` and the number of modes: ``(kind, vals, beta, k)``; nothing touches the device."""
        kind, vals, beta = self._check_records(modes)
        return kind, vals, beta, 0 if kind is None else vals.shape[1]

    def _staged(self, vals):
        """The modes on the device, the locator created if this is its first use."""
        self._ensure_locator()
        return self._stage(vals)[0]

    def _work_bytes(self, sizer: str, *sizes: Dict, loc=None) -> int:
        """What ``sizer`` asks for, the largest over the ``sizes`` (each the sizer's arguments by name, in order, ``loc``
        in front of them if it takes a locator); ``ValueError`` when it rejects them."""
        need, nbytes = ctypes.c_int64(0), 0
        for sz in sizes:
            if getattr(self._lib, sizer)(*(() if loc is None else (loc,)), *sz.values(), ctypes.byref(need)) != _native.PLFEM_OK:
                raise ValueError(f"{sizer} rejected " + ", ".join(f"{nm} = {v}" for nm, v in sz.items()))
            nbytes = max(nbytes, int(need.value))
        return nbytes

    def _work_buffer(self, sizer: str, nbytes: int, work=None):
        """``(buffer, aligned pointer)`` of a work buffer of ``nbytes``: fresh scratch, or the caller's ``work`` (a uint8
        device tensor of at least ``nbytes + 256`` bytes)."""
        if work is None:
            work = _native.device_scratch(nbytes + 256, self.tdev)
        elif work.numel() < nbytes + 256:
            raise ValueError(f"work buffer smaller than {sizer} + 256")
        return work, (work.data_ptr() + 255) & ~255

    def _work_call(self, sizer: str, sizes: Dict, fn: str, args, outs, work=None, loc=None) -> None:
        """One entry point that takes a work buffer: ``fn(*args, work, work_bytes, *outs)`` with the buffer sized by
        ``sizer(**sizes)``; ``outs`` are the host arrays it fills."""
        nbytes = self._work_bytes(sizer, sizes, loc=loc)
        work, aligned = self._work_buffer(sizer, nbytes, work)
        self._check(getattr(self._lib, fn)(*args, aligned, nbytes, *(_native._ptr(o) for o in outs)), fn)

    def _mode_call(self, sizer: str, sizes: Dict, fn: str, kind, staged, args, outs, work=None, loc=None) -> None:
        """:meth:`_work_call` of an entry point whose arguments begin ``(locator, ncomp, k, modes, indexed)``."""
        ncomp, _, k = staged.shape
        self._work_call(sizer, sizes, fn, (self._loc, ncomp, k, staged.data_ptr(), 1 if kind == "vectorial" else 0, *args), outs,
                        work=work, loc=loc)

    def sample(self, modes: Sequence[Dict], points, hz: bool = True) -> Dict[str, np.ndarray]:
        """Values of the modes at ``points`` (2, npts): ``{"Hx", "Hy"[, "Hz_im"]}`` (vectorial records; ``Hz_im`` =
        -(dHx/dx + dHy/dy) / beta when ``hz``) or ``{"u"}`` (scalar records), each (k, npts); ``"element"`` (npts,)
        int32, the element each point was found in or -1 (value 0)."""
        kind, vals, beta, k = self._checked(modes)
        pts = np.asarray(points, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[0] != 2:
            raise ValueError("points must be an array of shape (2, npts)")
        if kind == "vectorial" and hz and not np.all(np.isfinite(beta) & (beta != 0)):
            raise ValueError("Hz_im needs a finite, non-zero 'beta' in every vectorial record (or hz=False)")
        import torch
        npts = pts.shape[1]
        ncomp = 0 if kind is None else vals.shape[0]
        names = {"vectorial": ["Hx", "Hy"] + (["Hz_im"] if hz else []), "scalar": ["u"], None: []}[kind]
        nout = len(names)
        res = {nm: np.empty((k, npts), dtype=np.float64) for nm in names}
        res["element"] = np.empty(npts, dtype=np.int32)
        if npts == 0:
            return res
        self._ensure_locator()
        staged = beta_d = None
        if k:
            staged = self._staged(vals)
            if kind == "vectorial" and hz:
                beta_d = torch.from_numpy(beta).to(self.tdev)
        chunk = int(max(1024, min(npts, self.CHUNK_BYTES // (8 * max(1, nout * k) + 20), 1 << 30)))
        with torch.cuda.stream(self.stream):
            for s in range(0, npts, chunk):
                e = min(npts, s + chunk)
                n = e - s
                pd = torch.from_numpy(np.ascontiguousarray(pts[:, s:e])).to(self.tdev)
                od = _native.device_output((max(nout, 1), k, n), torch.float64, self.tdev)
                ed = _native.device_output((n,), torch.int32, self.tdev)
                self._check(self._lib.plfem_sample_fields(
                    self._loc, max(ncomp, 1), k, ctypes.c_void_p(staged.data_ptr() if staged is not None else 0),
                    1 if kind == "vectorial" else 0, ctypes.c_void_p(beta_d.data_ptr() if beta_d is not None else 0), n,
                    ctypes.c_void_p(pd.data_ptr()), ctypes.c_void_p(od.data_ptr()), ctypes.c_void_p(ed.data_ptr())),
                    "plfem_sample_fields")
                oh = od.cpu().numpy()
                for c, nm in enumerate(names):
                    res[nm][:, s:e] = oh[c]
                res["element"][s:e] = ed.cpu().numpy()
        return res

    def sample_grid(self, modes: Sequence[Dict], nx: int, ny: int, extent=None, hz: bool = True) -> Dict[str, np.ndarray]:
        """:meth:`sample` on the regular nx x ny grid over ``extent`` = (xmin, xmax, ymin, ymax) (default: the mesh's
        bounding box): every component (k, ny, nx), ``"element"`` (ny, nx), and the axes ``"x"`` (nx,), ``"y"`` (ny,)."""
        x, y, pts = self._grid_points(nx, ny, extent)
        res = self.sample(modes, pts, hz=hz)
        ny, nx = y.size, x.size
        out = {nm: (v.reshape(ny, nx) if nm == "element" else v.reshape(v.shape[0], ny, nx)) for nm, v in res.items()}
        out["x"], out["y"] = x, y
        return out

    def _grid_points(self, nx: int, ny: int, extent) -> tuple:
        """The axes ``x`` (nx,), ``y`` (ny,) of the regular grid over ``extent`` (default: the mesh's bounding box) and its
        points (2, ny nx), x fastest."""
        nx, ny = int(nx), int(ny)
        if nx < 1 or ny < 1:
            raise ValueError("nx and ny must be >= 1")
        ext = self.bbox if extent is None else tuple(float(v) for v in extent)
        if len(ext) != 4:
            raise ValueError("extent must be (xmin, xmax, ymin, ymax)")
        x = np.linspace(ext[0], ext[1], nx)
        y = np.linspace(ext[2], ext[3], ny)
        pts = np.empty((2, ny * nx), dtype=np.float64)
        pts[0] = np.tile(x, ny)
        pts[1] = np.repeat(y, nx)
        return x, y, pts

    def grams(self, modes: Sequence[Dict], geometry) -> Dict[str, np.ndarray]:
        """Same-mesh Grams of the modes under the element forms of the assembly, split by material region
        (``plfem_mode_grams``; the mesh's own six-point rule and the closed-disc core test of the assembly), each (k, k):
        vectorial records ``M_core``, ``M_clad``, ``K_core``, ``K_clad``, ``D`` (so that ``V^T A V = sum_r K_r / eps_r +
        alpha_p D - k0^2 (M_core + M_clad)`` and ``V^T B V = sum_r M_r / eps_r`` on the interior DOFs), scalar records
        ``M_core``, ``M_clad``, ``S`` (``V^T A V = S - k0^2 sum_r eps_r M_r``, ``V^T B V = M_core + M_clad``)."""
        reject_profile(geometry, "ModeFields.grams")
        kind, vals, _, k = self._checked(modes)
        cores = self._cores(geometry)
        if k == 0:
            return {nm: np.zeros((0, 0)) for nm in GRAM_NAMES.get(kind, ())}
        return self._grams_staged(kind, self._staged(vals), cores)

    @staticmethod
    def _cores(geometry) -> np.ndarray:
        """The (ncore, 3) table (x, y, r) of a geometry's cores; ``ValueError`` without them or with more than 64."""
        if not all(hasattr(geometry, a) for a in ("positions", "core_radii")):
            raise ValueError("geometry must have positions and core_radii")
        cores = _core_table(geometry)
        if cores.shape[0] > 64:
            raise ValueError("at most 64 cores")
        return cores

    def _grams_staged(self, kind, staged, cores) -> Dict[str, np.ndarray]:
        """``plfem_mode_grams`` on modes already staged (ncomp, n, k) on the device."""
        names = GRAM_NAMES[kind]
        ncomp, _, k = staged.shape
        out = np.empty((len(names), k, k), dtype=np.float64)
        self._mode_call("plfem_gram_work_bytes", {"ncomp": ncomp, "k": k}, "plfem_mode_grams", kind, staged,
                        (_native._ptr(cores), cores.shape[0]), (out,))
        return {nm: out[i] for i, nm in enumerate(names)}

    def profile_grams(self, modes: Sequence[Dict], geometry) -> Dict[str, np.ndarray]:
        """Grams of the modes of a profile solve (``plfem_profile_grams``): the forms of :meth:`grams` under the permittivity
        of the index profile that ``geometry`` carries (``geometry.index_profile``), evaluated at every quadrature point
        as the assembly evaluates it, each (k, k).  Vectorial records: ``M``, ``M_w``, ``K_w``, ``D`` with the weight
        ``w = 1 / eps``, so that ``V^T A V = K_w + alpha_p D - k0^2 M`` and ``V^T B V = M_w`` on the interior DOFs; scalar
        records: ``M``, ``M_w``, ``S`` with ``w = eps``, so that ``V^T A V = S - k0^2 M_w`` and ``V^T B V = M``."""
        profile = index_profile_of(geometry)
        if profile is None:
            raise ValueError("profile_grams needs a geometry that carries an index profile (ProfiledGeometry); "
                             "for core discs on a cladding use grams")
        kind, vals, _, k = self._checked(modes)
        if k == 0:
            return {nm: np.zeros((0, 0)) for nm in PROFILE_GRAM_NAMES.get(kind, ())}
        return self._profile_grams_staged(kind, self._staged(vals), profile.table(), profile.eps_background, index_map=profile.index_map)

    def _set_index_map(self, index_map) -> None:
        """``plfem_locator_set_index_map``: the map of the profile of the call in flight, or None: clear.  Every profile
        branch sets or clears it, so a cached locator never carries a map into the next call."""
        self._check(_native.set_index_map_call(self._lib.plfem_locator_set_index_map, self._loc, index_map),
                    "plfem_locator_set_index_map")

    def _profile_grams_staged(self, kind, staged, table, eps_bg, work=None, index_map=None) -> Dict[str, np.ndarray]:
        """``plfem_profile_grams`` on modes already staged (ncomp, n, k) on the device; ``work``: a uint8 device tensor to
        use as the work buffer (at least the library's size + 256 bytes) instead of a fresh one; ``index_map``: the
        profile's map (``IndexProfile.index_map``) or None."""
        self._set_index_map(index_map)
        names = PROFILE_GRAM_NAMES[kind]
        ncomp, _, k = staged.shape
        table = np.ascontiguousarray(np.asarray(table, dtype=np.float64).reshape(-1, 8))
        out = np.empty((len(names), k, k), dtype=np.float64)
        self._mode_call("plfem_profile_gram_work_bytes", {"ncomp": ncomp, "k": k}, "plfem_profile_grams", kind, staged,
                        (_native._ptr(table), table.shape[0], float(eps_bg)), (out,), work=work)
        return {nm: out[i] for i, nm in enumerate(names)}

    def profile_tangent_grams(self, modes: Sequence[Dict], geometry, tangents=(), moments: bool = False,
                              origin=(0.0, 0.0)) -> Dict[str, np.ndarray]:
        """Grams of the modes of a profile solve under first-order changes of the profile's values
        (``plfem_profile_tangent_grams``).  ``tangents``: :class:`.profile.ProfileTangent` objects of the profile that
        ``geometry`` carries.  With ``w`` the weight of :meth:`profile_grams` and ``dw_t`` its change along tangent t --
        ``-d eps_t / eps^2`` for vectorial records, ``d eps_t`` for scalar ones -- ``M_d`` (ntan, k, k) is ``M_w`` under
        ``dw_t`` and, for vectorial records, ``K_d`` is ``K_w`` under it: the derivatives of ``V^T B V`` and ``V^T A V``
        (vectorial) or, times ``-k0^2``, of ``V^T A V`` (scalar) along the tangent.  ``moments``: also ``M_wX``, ``M_wY``
        (k, k) and, for vectorial records, ``K_wX``, ``K_wY``: ``M_w`` and ``K_w`` under ``w X``, ``w Y`` with ``X = x -
        origin[0]``, ``Y = y - origin[1]`` -- what a bend moves the pencils by (:mod:`.profile_response`)."""
        profile = index_profile_of(geometry)
        if profile is None:
            raise ValueError("profile_tangent_grams needs a geometry that carries an index profile (ProfiledGeometry)")
        tangents = self._tangents(profile, tangents)
        o = self._origin(origin)
        kind, vals, _, k = self._checked(modes)
        if not tangents and not moments:
            raise ValueError("nothing to compute: no tangents and moments = False")
        if k == 0:
            return self._tangent_result(kind, np.zeros((len(tangents) + (2 if moments else 0), 2, 0, 0)), len(tangents), bool(moments))
        return self._profile_tangent_grams_staged(kind, self._staged(vals), profile, tangents, bool(moments), o)

    @staticmethod
    def _tangents(profile, tangents) -> list:
        """``tangents`` as a list of tangents of ``profile``, at most 256; ``ValueError`` otherwise."""
        if isinstance(tangents, ProfileTangent):
            tangents = [tangents]
        try:
            tangents = list(tangents)
        except TypeError:
            raise ValueError("tangents must be a sequence of ProfileTangent objects") from None
        if not all(isinstance(t, ProfileTangent) for t in tangents):
            raise ValueError("tangents must be a sequence of ProfileTangent objects")
        if len(tangents) > TANGENT_MAX:
            raise ValueError(f"at most {TANGENT_MAX} tangents per call")
        return [t.check(profile) for t in tangents]

    @staticmethod
    def _tangent_result(kind, out, ntan: int, moments: bool) -> Dict[str, np.ndarray]:
        """``out`` (ncol, nout, k, k) of ``plfem_profile_tangent_grams`` under the names of :meth:`profile_tangent_grams`."""
        names = {"vectorial": ("M", "K"), "scalar": ("M",), None: ()}[kind]
        res = {nm + "_d": np.ascontiguousarray(out[:ntan, i]) for i, nm in enumerate(names)}
        if moments:
            for i, nm in enumerate(names):
                res[nm + "_wX"], res[nm + "_wY"] = out[ntan, i].copy(), out[ntan + 1, i].copy()
        return res

    def _profile_tangent_grams_staged(self, kind, staged, profile, tangents, moments, origin, work=None) -> Dict[str, np.ndarray]:
        """``plfem_profile_tangent_grams`` on modes already staged (ncomp, n, k) on the device, in calls of at most
        ``TANGENT_MAPS`` tangent maps each (the moment columns ride on the first); ``work`` as for
        :meth:`_profile_grams_staged`."""
        self._set_index_map(profile.index_map)
        ncomp, _, k = staged.shape
        nout = 2 if ncomp == 2 else 1
        table = profile.table()
        ntan = len(tangents)
        out = np.empty((ntan + (2 if moments else 0), nout, k, k), dtype=np.float64)
        calls, cur, nmaps = [], [], 0                         # lists of tangent indices, each with at most TANGENT_MAPS maps
        for i, t in enumerate(tangents):
            if t.d_map is not None and nmaps == TANGENT_MAPS:
                calls.append(cur)
                cur, nmaps = [], 0
            cur.append(i)
            nmaps += t.d_map is not None
        if cur or not calls:
            calls.append(cur)
        for ci, idx in enumerate(calls):
            mom = bool(moments and ci == 0)
            if not idx and not mom:
                continue
            rows = np.ascontiguousarray(np.stack([tangents[i].row() for i in idx])) if idx else np.zeros((0, 1 + 2 * len(profile)))
            maps = [tangents[i].d_map for i in idx if tangents[i].d_map is not None]
            which, n = np.full(len(idx), -1, dtype=np.int32), 0
            for j, i in enumerate(idx):
                if tangents[i].d_map is not None:
                    which[j], n = n, n + 1
            maps_a = np.ascontiguousarray(np.stack(maps)) if maps else None
            part = np.empty((len(idx) + (2 if mom else 0), nout, k, k), dtype=np.float64)
            self._mode_call("plfem_profile_tangent_gram_work_bytes",
                            {"ncomp": ncomp, "k": k, "ntan": len(idx), "nmap": len(maps), "moments": int(mom)},
                            "plfem_profile_tangent_grams", kind, staged,
                            (_native._ptr(table), table.shape[0], float(profile.eps_background),
                             _native._ptr(rows) if idx else None, len(idx), None if maps_a is None else _native._ptr(maps_a),
                             len(maps), _native._ptr(which) if maps else None, int(mom), _native._ptr(origin)), (part,),
                            work=work, loc=self._loc)
            out[idx] = part[:len(idx)]
            if mom:
                out[ntan:] = part[len(idx):]
        return self._tangent_result(kind, out, ntan, moments)

    def index_map_densities(self, modes: Sequence[Dict], geometry, basis=None) -> Dict[str, np.ndarray]:
        """Pixel densities of the sampled map of a profile solve (``plfem_index_map_gradients``): the derivative of the
        diagonal of ``M_w`` (and ``K_w``) of :meth:`profile_grams` in the permittivity of EVERY pixel of the map, in one pass
        over the quadrature points whatever the size of the map.  ``M_px`` (k', ny, nx) is ``d (v_r^T B v_r) / d E`` for
        vectorial records and ``d (M_w)_rr / d E`` for scalar ones (so ``d (v_r^T A v_r) / d E = -k0^2 M_px``); ``K_px``
        (vectorial only) is ``d (v_r^T A v_r) / d E``; ``support`` (ny, nx) int32 counts the quadrature points that see the
        pixel -- inside the map's extent, under no layer, in a cell the pixel is a corner of: where it is 0 every plane is
        exactly 0.  For a tangent map D, ``(D * M_px[r]).sum()`` is ``M_d[0][r, r]`` of :meth:`profile_tangent_grams`.

        ``basis``: an optional (k', k) matrix; the fields are then ``v_r = sum_m basis[r, m] mode_m``, formed on the host
        before staging (default: the modes themselves, k' = k).  Off-diagonal densities of a pair of modes follow by
        polarisation: ``basis`` rows ``h_m + h_n`` and ``h_m - h_n`` give ``4 d (h_m^T B h_n) / d E`` as their difference.
        The fields go in calls of at most 256 that keep a call's result under 2^27 doubles."""
        profile = index_profile_of(geometry)
        if profile is None:
            raise ValueError("index_map_densities needs a geometry that carries an index profile (ProfiledGeometry)")
        if profile.index_map is None:
            raise ValueError("index_map_densities needs a profile with a sampled map (IndexProfile.sampled)")
        kind, vals, _, k = self._checked(modes)
        ny, nx = profile.index_map[0].shape
        if basis is not None:
            try:
                Bm = np.asarray(basis, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"basis must be a matrix of shape (k', {k}) of finite numbers") from None
            if Bm.ndim != 2 or Bm.shape[1] != k or not np.all(np.isfinite(Bm)):
                raise ValueError(f"basis must be a matrix of shape (k', {k}) of finite numbers")
            if k:
                vals = np.ascontiguousarray(np.einsum("pm,cmn->cpn", Bm, vals))
            k = Bm.shape[0] if k else 0
        if k == 0:
            res = {"M_px": np.zeros((0, ny, nx))}
            if kind != "scalar":
                res["K_px"] = np.zeros((0, ny, nx))
            res["support"] = np.zeros((ny, nx), dtype=np.int32)
            return res
        return self._index_map_densities_staged(kind, self._staged(vals), profile)

    def _index_map_densities_staged(self, kind, staged, profile, work=None) -> Dict[str, np.ndarray]:
        """``plfem_index_map_gradients`` on fields already staged (ncomp, n, k) on the device, in calls of at most
        ``MAP_GRADIENT_MAX`` fields whose result stays under ``MAP_GRADIENT_RESULT`` doubles; ``work`` as for
        :meth:`_profile_grams_staged`."""
        self._set_index_map(profile.index_map)
        ncomp, n, k = staged.shape
        nout = 2 if ncomp == 2 else 1
        ny, nx = profile.index_map[0].shape
        table = profile.table()
        per = max(1, min(MAP_GRADIENT_MAX, MAP_GRADIENT_RESULT // (nout * nx * ny)))
        out = np.empty((k, nout, ny, nx), dtype=np.float64)
        support = np.empty((ny, nx), dtype=np.int32)
        for f0 in range(0, k, per):
            f1 = min(k, f0 + per)
            part = staged if (f0, f1) == (0, k) else staged[:, :, f0:f1].contiguous()
            self._mode_call("plfem_index_map_gradient_work_bytes", {"ncomp": ncomp, "k": f1 - f0}, "plfem_index_map_gradients",
                            kind, part, (_native._ptr(table), table.shape[0], float(profile.eps_background)),
                            (out[f0:f1], support), work=work, loc=self._loc)
        res = {"M_px": np.ascontiguousarray(out[:, 0])}
        if nout == 2:
            res["K_px"] = np.ascontiguousarray(out[:, 1])
        res["support"] = support
        return res

    def indicators(self, modes: Sequence[Dict], geometry, alpha_p: float = 1.0) -> Dict[str, np.ndarray]:
        """A-posteriori error indicators of the modes on this mesh (``plfem_mode_indicators``): ``{"eta2": (k, ne),
        "total": (k,)}`` with ``eta2[m, T]`` = element residual plus flux jumps of mode m on element T under the pencil the
        mode was solved with -- the eigenvalue is taken from the record (``beta**2`` for vectorial records, ``-beta**2``
        for scalar ones), ``k0`` and the material map from ``geometry`` (its index profile if it carries one, otherwise
        its core discs at ``n_core`` on ``n_clad``), ``alpha_p`` the divergence penalty of the vectorial solve -- and
        ``total[m] = eta2[m].sum()``.  :mod:`.adapt` marks and refines with them."""
        kind, vals, beta, k = self._checked(modes)
        try:
            alpha_p = float(alpha_p)
            k0 = float(geometry.k0)
        except (AttributeError, TypeError, ValueError):
            raise ValueError("geometry must have k0, and alpha_p must be a number") from None
        if not (np.isfinite(alpha_p) and np.isfinite(k0)):
            raise ValueError("k0 and alpha_p must be finite")
        profile = index_profile_of(geometry)
        if profile is None:
            if not all(hasattr(geometry, a) for a in ("n_core", "n_clad")):
                raise ValueError("geometry must have n_core and n_clad (or carry an index profile)")
            cores = self._cores(geometry)
            table, eps, index_map = np.zeros((0, 8)), (float(geometry.n_core) ** 2, float(geometry.n_clad) ** 2, 1.0), None
        else:
            cores = np.zeros((0, 3))
            table, eps, index_map = profile.table(), (1.0, 1.0, float(profile.eps_background)), profile.index_map
        if k == 0:
            return {"eta2": np.zeros((0, self.ne)), "total": np.zeros(0)}
        if not np.all(np.isfinite(beta)):
            raise ValueError("every mode record needs a finite 'beta': the indicator is that of the eigenpair")
        lam = np.ascontiguousarray(beta * beta if kind == "vectorial" else -(beta * beta))
        eta2 = self._indicators_staged(kind, self._staged(vals), lam, k0, alpha_p, cores, eps, table, index_map=index_map)
        return {"eta2": eta2, "total": eta2.sum(axis=1)}

    def _indicators_staged(self, kind, staged, lam, k0, alpha_p, cores, eps, table, work=None, index_map=None) -> np.ndarray:
        """``plfem_mode_indicators`` on modes already staged (ncomp, n, k) on the device: (k, ne).  ``eps`` = (eps_core,
        eps_clad, eps_bg); ``work``: a uint8 device tensor to use as the work buffer instead of a fresh one; ``index_map``:
        the profile's map (``IndexProfile.index_map``) or None."""
        self._set_index_map(index_map)
        ncomp, _, k = staged.shape
        table = np.ascontiguousarray(np.asarray(table, dtype=np.float64).reshape(-1, 8))
        cores = np.ascontiguousarray(np.asarray(cores, dtype=np.float64).reshape(-1, 3))
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        out = np.empty((k, self.ne), dtype=np.float64)
        self._mode_call("plfem_indicator_work_bytes", {"ncomp": ncomp, "k": k}, "plfem_mode_indicators", kind, staged,
                        (_native._ptr(lam), float(k0), float(alpha_p), _native._ptr(cores), cores.shape[0], float(eps[0]),
                         float(eps[1]), _native._ptr(table), table.shape[0], float(eps[2])), (out,), work=work, loc=self._loc)
        return out

    # -- electric field and power --------------------------------------------------------------------------------
    def _material(self, geometry) -> SimpleNamespace:
        """The material arguments of the electric-field calls from ``geometry``: its index profile if it carries one
        (``use_profile = 1``), else its core discs at ``n_core`` on ``n_clad``.  ``cores`` (n, 3) are the region discs of
        :meth:`flux_grams` either way: the (base) geometry's ``positions`` / ``core_radii``, empty without them."""
        profile = index_profile_of(geometry)
        has_cores = all(hasattr(geometry, a) for a in ("positions", "core_radii"))
        if profile is None:
            if not (has_cores and all(hasattr(geometry, a) for a in ("n_core", "n_clad"))):
                raise ValueError("geometry must carry an index profile, or have positions, core_radii, n_core and n_clad")
            eps = (float(geometry.n_core) ** 2, float(geometry.n_clad) ** 2)
            if not all(np.isfinite(e) and e > 0 for e in eps):
                raise ValueError("n_core and n_clad must be finite and non-zero")
            return SimpleNamespace(cores=self._cores(geometry), eps_core=eps[0], eps_clad=eps[1], table=np.zeros((0, 8)),
                                   eps_bg=1.0, use_profile=0, index_map=None)
        cores = self._cores(geometry) if has_cores else np.zeros((0, 3))
        return SimpleNamespace(cores=cores, eps_core=1.0, eps_clad=1.0, table=profile.table(),
                               eps_bg=float(profile.eps_background), use_profile=1, index_map=profile.index_map)

    @staticmethod
    def _material_args(mat) -> tuple:
        """``mat`` as the entry points take it; the arrays stay alive in ``mat``."""
        mat.cores = np.ascontiguousarray(np.asarray(mat.cores, dtype=np.float64).reshape(-1, 3))
        mat.table = np.ascontiguousarray(np.asarray(mat.table, dtype=np.float64).reshape(-1, 8))
        return (_native._ptr(mat.cores), mat.cores.shape[0], float(mat.eps_core), float(mat.eps_clad), _native._ptr(mat.table),
                mat.table.shape[0], float(mat.eps_bg), int(mat.use_profile))

    def _checked_vectorial(self, modes, what: str):
        """:meth:`_checked` for the calls that need vectorial records with a usable ``beta``."""
        kind, vals, beta, k = self._checked(modes)
        if kind == "scalar":
            raise ValueError(f"{what}: the electric field needs vectorial records")
        if k and not np.all(np.isfinite(beta) & (beta != 0)):
            raise ValueError(f"{what} needs a finite, non-zero 'beta' in every vectorial record")
        return vals, beta, k

    def flux_grams(self, modes: Sequence[Dict], geometry) -> Dict[str, np.ndarray]:
        """Power Grams of vectorial modes (``plfem_flux_grams``), each (k, k): ``M_w_core``, ``M_w_rest``, ``G_w_core``,
        ``G_w_rest`` with ``M_w[m, n] = int w (hx_m hx_n + hy_m hy_n)``, ``G_w[m, n] = int w (gx_m hx_n + gy_m hy_n)``,
        ``w = 1 / eps`` and ``g = -grad (dx hx + dy hy)`` (element-wise second derivatives), over the mesh's own six-point
        rule, split by the closed core discs of ``geometry`` (of its base for a ``ProfiledGeometry``; none: everything is
        "rest").  The material is the geometry's index profile if it carries one, else its discs at ``n_core`` on
        ``n_clad``.  With ``e = E / Z0`` the cross power is ``P[m, n] = 1/2 int (Ex_m Hy_n - Ey_m Hx_n) = (beta_m M_w[m, n] +
        G_w[m, n] / beta_m) / (2 k0)``: :func:`.power.power_quantities_from_grams`."""
        mat = self._material(geometry)
        vals, _, k = self._checked_vectorial(modes, "ModeFields.flux_grams")
        if k == 0:
            return {nm: np.zeros((0, 0)) for nm in FLUX_GRAM_NAMES}
        return self._flux_grams_staged(self._staged(vals), mat)

    def _flux_grams_staged(self, staged, mat, work=None) -> Dict[str, np.ndarray]:
        """``plfem_flux_grams`` on modes already staged (2, n, k) on the device; ``mat``: what :meth:`_material` returns;
        ``work``: a uint8 device tensor to use as the work buffer instead of a fresh one."""
        self._set_index_map(mat.index_map)
        k = staged.shape[2]
        out = np.empty((len(FLUX_GRAM_NAMES), k, k), dtype=np.float64)
        self._mode_call("plfem_flux_gram_work_bytes", {"k": k}, "plfem_flux_grams", "vectorial", staged,
                        self._material_args(mat), (out,), work=work)
        return {nm: out[i] for i, nm in enumerate(FLUX_GRAM_NAMES)}

    def sample_e(self, modes: Sequence[Dict], points, geometry) -> Dict[str, np.ndarray]:
        """Electric field and axial Poynting flux of vectorial modes at ``points`` (2, npts) (``plfem_sample_efields``):
        ``{"Ex", "Ey", "Ez_im", "Sz"}`` each (k, npts), ``"eps"`` (npts,) the permittivity used and ``"element"`` (npts,)
        int32 (-1 and zeros for a point in no element).  Convention of :meth:`sample`: fields vary as exp(j (w t - beta
        z)), ``H = (Hx, Hy, j Hz_im)``, ``E = (Ex, Ey, j Ez_im)`` in units of ``Z0`` (``e = E / Z0``), from ``curl H = j w
        eps0 eps E`` with ``k0`` and the material of ``geometry`` (its index profile if it carries one, else its discs at
        ``n_core`` on ``n_clad``) and ``beta`` of each record; ``Sz = (Ex Hy - Ey Hx) / 2``.  The transverse E rests on
        element-wise second derivatives of the P2 field: first order in h."""
        mat = self._material(geometry)
        try:
            k0 = float(geometry.k0)
        except (AttributeError, TypeError, ValueError):
            raise ValueError("geometry must have k0") from None
        if not (np.isfinite(k0) and k0 > 0):
            raise ValueError("k0 must be finite and positive")
        vals, beta, k = self._checked_vectorial(modes, "ModeFields.sample_e")
        pts = np.asarray(points, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[0] != 2:
            raise ValueError("points must be an array of shape (2, npts)")
        npts = pts.shape[1]
        names = ("Ex", "Ey", "Ez_im", "Sz")
        res = {nm: np.empty((k, npts), dtype=np.float64) for nm in names}
        res["eps"] = np.empty(npts, dtype=np.float64)
        res["element"] = np.empty(npts, dtype=np.int32)
        if k == 0 or npts == 0:
            if k == 0:                               # nothing to evaluate: the device is not touched
                res["eps"][:] = 0.0
                res["element"][:] = -1
            return res
        import torch
        staged = self._staged(vals)
        self._set_index_map(mat.index_map)
        margs = self._material_args(mat)
        chunk = int(max(1024, min(npts, self.CHUNK_BYTES // (8 * 4 * k + 28), 1 << 30)))
        with torch.cuda.stream(self.stream):
            beta_d = torch.from_numpy(np.ascontiguousarray(beta)).to(self.tdev)
            for s in range(0, npts, chunk):
                e = min(npts, s + chunk)
                n = e - s
                pd = torch.from_numpy(np.ascontiguousarray(pts[:, s:e])).to(self.tdev)
                od = _native.device_output((4, k, n), torch.float64, self.tdev)
                epd = _native.device_output((n,), torch.float64, self.tdev)
                ed = _native.device_output((n,), torch.int32, self.tdev)
                self._check(self._lib.plfem_sample_efields(
                    self._loc, 2, k, staged.data_ptr(), 1, beta_d.data_ptr(), k0, *margs, n, pd.data_ptr(), od.data_ptr(),
                    epd.data_ptr(), ed.data_ptr()), "plfem_sample_efields")
                oh = od.cpu().numpy()
                for c, nm in enumerate(names):
                    res[nm][:, s:e] = oh[c]
                res["eps"][s:e] = epd.cpu().numpy()
                res["element"][s:e] = ed.cpu().numpy()
        return res

    def sample_grid_e(self, modes: Sequence[Dict], nx: int, ny: int, geometry, extent=None) -> Dict[str, np.ndarray]:
        """:meth:`sample_e` on the regular nx x ny grid of :meth:`sample_grid`: every component (k, ny, nx), ``"eps"`` and
        ``"element"`` (ny, nx), and the axes ``"x"`` (nx,), ``"y"`` (ny,)."""
        x, y, pts = self._grid_points(nx, ny, extent)
        res = self.sample_e(modes, pts, geometry)
        ny, nx = y.size, x.size
        out = {nm: (v.reshape(ny, nx) if v.ndim == 1 else v.reshape(v.shape[0], ny, nx)) for nm, v in res.items()}
        out["x"], out["y"] = x, y
        return out

    def core_grams(self, modes: Sequence[Dict], geometry) -> Dict[str, np.ndarray]:
        """Grams of the modes restricted to each core disc (``plfem_core_grams``), each (ncore, k, k): vectorial records
        ``Mx`` (sum over the core's quadrature points of hx_m hx_n), ``My`` and ``K`` (the form of ``K_core``), scalar
        records ``M``; and ``points`` (ncore,) int64, the quadrature points each core owns.  A point belongs to the
        highest-index core whose closed disc holds it, by the arithmetic of the assembly's core test, so summed over the
        cores ``Mx + My`` is ``M_core`` and ``K`` is ``K_core`` of :meth:`grams`; a core that owns no point gives zeros.
        With core c at eps_c instead of eps_core the pencils of :meth:`grams` become ``sum_c K_c / eps_c + ...``: these
        are the exact projections of a pencil with unequal core indices on the span of the modes."""
        reject_profile(geometry, "ModeFields.core_grams")
        kind, vals, _, k = self._checked(modes)
        cores = self._cores(geometry)
        ncore = cores.shape[0]
        if ncore < 1:
            raise ValueError("geometry has no cores")
        if k == 0:
            res = {nm: np.zeros((ncore, 0, 0)) for nm in CORE_GRAM_NAMES.get(kind, ())}
            res["points"] = np.zeros(ncore, dtype=np.int64)
            return res
        return self._core_grams_staged(kind, self._staged(vals), cores)

    def _core_grams_staged(self, kind, staged, cores) -> Dict[str, np.ndarray]:
        """``plfem_core_grams`` on modes already staged (ncomp, n, k) on the device."""
        names = CORE_GRAM_NAMES[kind]
        ncomp, _, k = staged.shape
        ncore = cores.shape[0]
        out = np.empty((ncore, len(names), k, k), dtype=np.float64)
        points = np.empty(ncore, dtype=np.int64)
        self._mode_call("plfem_core_gram_work_bytes", {"ncomp": ncomp, "k": k, "ncore": ncore}, "plfem_core_grams", kind, staged,
                        (_native._ptr(cores), ncore), (out, points), loc=self._loc)
        res = {nm: np.ascontiguousarray(out[:, i]) for i, nm in enumerate(names)}
        res["points"] = points
        return res

    def velocity_grams(self, modes: Sequence[Dict], geometry, velocities) -> Dict[str, np.ndarray]:
        """First-order change of the projected forms under mesh velocities (``plfem_velocity_grams``).  ``velocities``
        (nvel, nv, 2) or (nv, 2): per velocity a P1 field V on the mesh vertices, at most 256.  Under ``x -> x + t V``, every
        quadrature point keeping the material ``geometry`` gives it on the unmoved mesh (its index profile if it carries
        one, else its discs at ``n_core`` on ``n_clad``), the forms of :meth:`profile_grams` change at first order by the
        returned arrays, each (nvel, k, k) and bitwise symmetric: vectorial records ``dK_w``, ``dD``, ``dM``, ``dM_w``
        (``w = 1 / eps``; ``d(V^T A V) = dK_w + alpha_p dD - k0^2 dM``, ``d(V^T B V) = dM_w``), scalar records ``dS``,
        ``dM``, ``dM_w`` (``w = eps``; ``d(V^T A V) = dS - k0^2 dM_w``, ``d(V^T B V) = dM``); and ``count`` (nvel,) int64,
        the elements on which the velocity has a non-zero gradient -- the only ones that contribute."""
        mat = self._material(geometry)
        kind, vals, _, k = self._checked(modes)
        vel = np.asarray(velocities, dtype=np.float64)
        if vel.ndim == 2:
            vel = vel[None]
        if vel.ndim != 3 or vel.shape[1:] != (self.nv, 2):
            raise ValueError(f"velocities must have shape (nvel, {self.nv}, 2) or ({self.nv}, 2)")
        nvel = vel.shape[0]
        if not 1 <= nvel <= VELOCITY_MAX:
            raise ValueError(f"between 1 and {VELOCITY_MAX} velocities per call")
        if not np.all(np.isfinite(vel)):
            raise ValueError("every velocity entry must be finite")
        if k == 0:
            res = {nm: np.zeros((nvel, 0, 0)) for nm in VELOCITY_GRAM_NAMES.get(kind, ())}
            res["count"] = np.zeros(nvel, dtype=np.int64)
            return res
        return self._velocity_grams_staged(kind, self._staged(vals), mat, np.ascontiguousarray(vel))

    def _velocity_grams_staged(self, kind, staged, mat, vel, work=None) -> Dict[str, np.ndarray]:
        """``plfem_velocity_grams`` on modes already staged (ncomp, n, k) on the device; ``mat``: what :meth:`_material`
        returns; ``vel`` (nvel, nv, 2) contiguous float64; ``work``: a uint8 device tensor to use as the work buffer."""
        self._set_index_map(mat.index_map)
        names = VELOCITY_GRAM_NAMES[kind]
        ncomp, _, k = staged.shape
        nvel = vel.shape[0]
        out = np.empty((nvel, len(names), k, k), dtype=np.float64)
        count = np.empty(nvel, dtype=np.int64)
        self._mode_call("plfem_velocity_gram_work_bytes", {"ncomp": ncomp, "k": k, "nvel": nvel}, "plfem_velocity_grams", kind,
                        staged, (*self._material_args(mat), _native._ptr(vel), nvel), (out, count), work=work, loc=self._loc)
        res = {nm: np.ascontiguousarray(out[:, i]) for i, nm in enumerate(names)}
        res["count"] = count
        return res

    @staticmethod
    def _origin(origin) -> np.ndarray:
        """``origin`` as two finite float64; ``ValueError`` otherwise."""
        try:
            o = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(-1))
        except (TypeError, ValueError):
            raise ValueError("origin must be two finite numbers (x, y)") from None
        if o.size != 2 or not np.all(np.isfinite(o)):
            raise ValueError("origin must be two finite numbers (x, y)")
        return o

    def moment_grams(self, modes: Sequence[Dict], geometry, origin=(0.0, 0.0)) -> Dict[str, np.ndarray]:
        """The region Grams of :meth:`grams` weighted by the coordinates ``X = x - origin[0]``, ``Y = y - origin[1]`` of
        the quadrature point (``plfem_moment_grams``), each (k, k): ``M_core_X``, ``M_core_Y``, ``M_clad_X``, ``M_clad_Y``
        (``M_r_X[m, n] = sum over region r of X u_m . u_n``), for vectorial records also ``K_core_X``, ``K_core_Y``,
        ``K_clad_X``, ``K_clad_Y`` (the form of ``K_r``), and the second moments ``M_XX``, ``M_XY``, ``M_YY`` over both
        regions.  A bend enters both pencils linearly in the curvature through exactly these (:mod:`.bend`)."""
        reject_profile(geometry, "ModeFields.moment_grams")
        kind, vals, _, k = self._checked(modes)
        cores = self._cores(geometry)
        o = self._origin(origin)
        if k == 0:
            return {nm: np.zeros((0, 0)) for nm in MOMENT_GRAM_NAMES.get(kind, ())}
        return self._moment_grams_staged(kind, self._staged(vals), cores, o)

    def _moment_grams_staged(self, kind, staged, cores, origin) -> Dict[str, np.ndarray]:
        """``plfem_moment_grams`` on modes already staged (ncomp, n, k) on the device."""
        names = MOMENT_GRAM_NAMES[kind]
        ncomp, _, k = staged.shape
        out = np.empty((len(names), k, k), dtype=np.float64)
        self._mode_call("plfem_moment_gram_work_bytes", {"ncomp": ncomp, "k": k}, "plfem_moment_grams", kind, staged,
                        (_native._ptr(cores), cores.shape[0], _native._ptr(origin)), (out,))
        return {nm: out[i] for i, nm in enumerate(names)}

    def quartic(self, modes: Sequence[Dict], geometry=None, weights=(1.0, 1.0)) -> np.ndarray:
        """Packed quartic overlap of the modes over this mesh (``plfem_mode_quartic``), np x np with np = k (k + 1) / 2:
        ``Q[p(i,j), p(l,m)] = sum over the elements and the 16-point degree-8 rule of |det J| w_q wt(x_q) (u_i . u_j)
        (u_l . u_m)``, pairs i <= j numbered ``p(i,j) = i k - i (i - 1) / 2 + (j - i)`` (:func:`.nonlinear.pair_index`),
        transverse dot product for vectorial records.  ``geometry=None``: wt = 1; otherwise wt = ``weights[0]`` in the
        closed core discs of the assembly's core test and ``weights[1]`` outside.  At most 64 modes."""
        reject_profile(geometry, "ModeFields.quartic with a geometry")
        kind, vals, _, k = self._checked(modes)
        if kind is None:
            return np.zeros((0, 0))
        if k > 64:
            raise ValueError(f"at most 64 modes per quartic overlap, got {k}")
        try:
            wc, wl = (float(v) for v in weights)
        except (TypeError, ValueError):
            raise ValueError("weights must be two numbers (core, cladding)") from None
        if geometry is None:
            cores, ncore = np.zeros((0, 3)), -1
        else:
            if not all(hasattr(geometry, a) for a in ("positions", "core_radii")):
                raise ValueError("geometry must have positions and core_radii")
            if not (np.isfinite(wc) and np.isfinite(wl)):
                raise ValueError("weights must be finite")
            cores = _core_table(geometry)
            ncore = cores.shape[0]
            if ncore > 64:
                raise ValueError("at most 64 cores")
        npair = k * (k + 1) // 2
        out = np.empty((npair, npair), dtype=np.float64)
        self._mode_call("plfem_quartic_work_bytes", {"ncomp": vals.shape[0], "k": k}, "plfem_mode_quartic", kind,
                        self._staged(vals), (_native._ptr(cores), ncore, wc, wl), (out,))
        return out

    def project(self, modes: Sequence[Dict], x_factors, y_factors) -> np.ndarray:
        """Projection of the modes on separable analytic fields (``plfem_mode_project``), complex (ncomp, k, lb, la):
        ``P[c, m, b, a] = sum over the elements and the 16-point degree-8 rule of |det J| w_q u_c,m(x_q)
        phi(X_q; x_factors[a]) phi(Y_q; y_factors[b])`` with ``phi(t; c, s, kappa) = exp(-s (t - c)^2) exp(-i kappa t)``.
        A factor table has shape (l, 3), a row (c, s, kappa) with s >= 0: s = 0 is a plane wave, a Gaussian beam of 1/e
        field radius w has s = 1 / w^2.  Every component of a vectorial record (``Ex_dofs`` / ``Ey_dofs`` hold Hx / Hy) is
        projected on its own; ncomp = 1 for scalar records.  At most 64 modes and 4096 factors per axis; the y-factors
        are split into chunks so that one call's device result stays under ``CHUNK_BYTES``.  An empty mode list gives
        an empty array."""
        kind, vals, _, k = self._checked(modes)
        xf, yf = _factors(x_factors, "x_factors"), _factors(y_factors, "y_factors")
        la, lb = xf.shape[0], yf.shape[0]
        if kind is None:
            return np.zeros((0, 0, lb, la), dtype=np.complex128)
        ncomp = vals.shape[0]
        if k > 64:
            raise ValueError(f"at most 64 modes per projection, got {k}")
        self._ensure_locator()
        chunk = int(max(1, min(lb, self.CHUNK_BYTES // (16 * ncomp * k * la))))
        # one buffer for the full chunks and a shorter last one
        nbytes = self._work_bytes("plfem_project_work_bytes",
                                  *({"ncomp": ncomp, "k": k, "la": la, "lb": n} for n in {chunk, lb % chunk or chunk}))
        staged = self._staged(vals)
        work, aligned = self._work_buffer("plfem_project_work_bytes", nbytes)
        indexed = 1 if kind == "vectorial" else 0
        out = np.empty((ncomp, k, lb, la), dtype=np.complex128)
        for s in range(0, lb, chunk):
            yc = np.ascontiguousarray(yf[s:s + chunk])
            part = np.empty((ncomp, k, yc.shape[0], la), dtype=np.complex128)
            self._check(self._lib.plfem_mode_project(self._loc, ncomp, k, staged.data_ptr(), indexed, la, _native._ptr(xf),
                                                     yc.shape[0], _native._ptr(yc), aligned, nbytes, _native._ptr(part)),
                        "plfem_mode_project")
            out[:, :, s:s + chunk] = part
        return out

    def project_sampled(self, modes: Sequence[Dict], frames, x, y) -> np.ndarray:
        """Projection of the modes on sampled complex fields (``plfem_mode_project_sampled``), complex (ncomp, k, nf):
        ``P[c, m, f] = sum over the elements and the 16-point degree-8 rule of |det J| w_q u_c,m(x_q) F_f(x_q)`` (no
        conjugation), ``F_f`` the bilinear interpolant of ``frames[f]`` on the pixel grid ``x`` (nx,) x ``y`` (ny,) and 0
        outside its closed extent.  ``frames`` is complex or real, (nf, ny, nx) or one image (ny, nx); ``x`` and ``y``
        are ascending, uniformly spaced axes (every step within ``1e-12 (x[-1] - x[0])`` of the mean step; the ``"x"`` /
        ``"y"`` of :meth:`sample_grid` are such axes) of 2 to 8192 pixels; the grid step is ``(x[-1] - x[0]) / (nx - 1)``.
        Every component of a vectorial record is projected on its own.  The modes are staged once; the frames go to the
        device in chunks of at most ``CHUNK_BYTES`` and 4096 frames, and the bits of a frame's result do not depend on
        the chunking.  A NaN pixel gives NaN for its frame only.  At most 64 modes; an empty mode list gives an empty
        array, ``nf = 0`` gives (ncomp, k, 0).  Argument errors raise ``ValueError`` before any device call."""
        kind, vals, _, k = self._checked(modes)
        xa, dx = _grid_axis(x, "x")
        ya, dy = _grid_axis(y, "y")
        nx, ny = xa.size, ya.size
        fr = _frames(frames, nx, ny)
        nf = fr.shape[0]
        if kind is None:
            return np.zeros((0, 0, nf), dtype=np.complex128)
        ncomp = vals.shape[0]
        if k > 64:
            raise ValueError(f"at most 64 modes per projection, got {k}")
        out = np.empty((ncomp, k, nf), dtype=np.complex128)
        if nf == 0:
            return out
        self._ensure_locator()
        import torch
        chunk = int(max(1, min(nf, PROJECT_SAMPLED_MAX_FRAMES, self.CHUNK_BYTES // (16 * ny * nx))))
        # (a shorter last chunk needs no more)
        nbytes = self._work_bytes("plfem_project_sampled_work_bytes", {"ncomp": ncomp, "k": k, "nf": chunk})
        staged = self._staged(vals)
        work, aligned = self._work_buffer("plfem_project_sampled_work_bytes", nbytes)
        indexed = 1 if kind == "vectorial" else 0
        with torch.cuda.stream(self.stream):
            for s in range(0, nf, chunk):
                src = torch.from_numpy(np.ascontiguousarray(fr[s:s + chunk])).to(self.tdev)       # (n, ny, nx) complex
                n = src.shape[0]
                dev = torch.view_as_real(src).permute(1, 2, 0, 3).contiguous()                    # [ny][nx][n][2]
                del src
                part = np.empty((ncomp, k, n), dtype=np.complex128)
                self._check(self._lib.plfem_mode_project_sampled(
                    self._loc, ncomp, k, staged.data_ptr(), indexed, nx, ny, float(xa[0]), float(ya[0]), dx, dy, n,
                    dev.data_ptr(), aligned, nbytes, _native._ptr(part)), "plfem_mode_project_sampled")
                out[:, :, s:s + chunk] = part
        return out

    def close(self):
        if getattr(self, "_loc", None):
            self._lib.plfem_locator_destroy(self._loc)      # synchronises the stream before the memory goes back to torch
            self._loc = None
            self._mem = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _as_fields(m, device) -> ModeFields:
    return m if isinstance(m, ModeFields) else ModeFields(m, device=device)


def _overlap_pair(what: str, modes_a, mesh_a, modes_b, mesh_b, weight, device, posed: bool = False, poses=None,
                  normalize: bool = False):
    """The arguments of :func:`mode_overlap` / :func:`mode_overlap_poses` (``what``), checked in one order: the records'
    kinds, the pose table of a ``posed`` call (returned as ``P``), the weight, ``fa`` / ``fb`` (one :class:`ModeFields` when both meshes are
    the same), the records against each mesh (``va``, ``vb``, ``ka``, ``kb``).  With modes on both sides (``ready``) also
    the chunk pairs of a posed call, ``indexed``, ``weight`` = (core table or None, ncore, eps_core, eps_clad) as the
    entry points take it, both locators and that they share a device.  Only the locators touch the device."""
    ka_kind, va, _ = _records(modes_a)
    kb_kind, vb, _ = _records(modes_b)
    if ka_kind is not None and kb_kind is not None and ka_kind != kb_kind:
        raise ValueError("vectorial and scalar mode records cannot be mixed")
    P = _poses(poses) if posed else None
    if weight is not None and not all(hasattr(weight, a) for a in ("positions", "core_radii", "n_core", "n_clad")):
        raise ValueError("weight must be None or a geometry (positions, core_radii, n_core, n_clad)")
    reject_profile(weight, f"{what} with a weight")
    if posed and normalize and weight is not None:
        raise ValueError("normalize=True is defined for weight=None only")
    fa = _as_fields(mesh_a, device)
    fb = fa if (mesh_b is mesh_a or (not isinstance(mesh_b, ModeFields) and not isinstance(mesh_a, ModeFields)
                                     and mesh_key(mesh_b) == mesh_key(mesh_a))) else _as_fields(mesh_b, device)
    _, va, _ = fa._check_records(modes_a)
    _, vb, _ = fb._check_records(modes_b)
    pr = SimpleNamespace(fa=fa, va=va, fb=fb, vb=vb, P=P, ka=0 if va is None else va.shape[1],
                         kb=0 if vb is None else vb.shape[1])
    pr.ready = pr.ka > 0 and pr.kb > 0
    if not pr.ready:
        return pr
    if posed and ((pr.ka + 31) // 32) * ((pr.kb + 31) // 32) > POSE_MAX_CHUNK_PAIRS:
        raise ValueError(f"at most {POSE_MAX_CHUNK_PAIRS} pairs of 32-mode chunks per posed overlap, got ka = {pr.ka}, "
                         f"kb = {pr.kb}")
    pr.indexed = 1 if ka_kind == "vectorial" else 0
    if weight is None:
        pr.weight = (None, -1, 1.0, 1.0)
    else:
        cores = _core_table(weight)
        if cores.shape[0] > 64:
            raise ValueError("at most 64 cores")
        pr.weight = (_native._ptr(cores), cores.shape[0], float(weight.n_core) ** 2, float(weight.n_clad) ** 2)
    fa._ensure_locator()
    fb._ensure_locator()
    if fa.device != fb.device:
        raise ValueError("both meshes must be evaluated on one device")
    return pr


def mode_overlap(modes_a: Sequence[Dict], mesh_a, modes_b: Sequence[Dict], mesh_b, weight=None, normalize: bool = False,
                 device: Optional[int] = None) -> np.ndarray:
    """``O[i, j] = sum over the elements of mesh_b and its six-point rule |det J| w_q wt(x_q) u_a,i(x_q) . u_b,j(x_q)``
    (transverse dot product for vectorial records), (ka, kb).  ``weight``: None (wt = 1) or a geometry (wt = 1/eps(x),
    the closed-disc core test of the assembly: on one mesh O = V^T M_(1/eps) V, the B of the eigenproblem).
    ``normalize=True``: the power coupling |O_ij|^2 / (O^aa_ii O^bb_jj), each self-overlap on its own mesh.  ``mesh_a`` /
    ``mesh_b`` may be :class:`ModeFields` (their analyses and locators are reused)."""
    pr = _overlap_pair("mode_overlap", modes_a, mesh_a, modes_b, mesh_b, weight, device)
    if not pr.ready:
        return np.zeros((pr.ka, pr.kb), dtype=np.float64)
    fa, va, fb, vb = pr.fa, pr.va, pr.fb, pr.vb

    def overlap(f1, v1, f2, v2):
        s1, s2 = f1._stage(v1)[0], f2._stage(v2)[0]
        k1, k2 = v1.shape[1], v2.shape[1]
        out = np.empty((k1, k2), dtype=np.float64)
        f2.stream.synchronize()                 # (B's staging ran on B's stream; the overlap runs on A's)
        f1._work_call("plfem_overlap_work_bytes", {"ka": k1, "kb": k2}, "plfem_field_overlap",
                      (f1._loc, s1.data_ptr(), k1, pr.indexed, f2._loc, s2.data_ptr(), k2, pr.indexed, v1.shape[0], *pr.weight),
                      (out,))
        return out

    O = overlap(fa, va, fb, vb)
    if not normalize:
        return O
    daa = np.diag(overlap(fa, va, fa, va)).copy()
    dbb = np.diag(overlap(fb, vb, fb, vb)).copy()
    return O * O / (daa[:, None] * dbb[None, :])


def pose_table(dx=0.0, dy=0.0, angle=0.0, scale=1.0) -> np.ndarray:
    """The (T, 5) pose table ``(tx, ty, c, s, m)`` of :func:`mode_overlap_poses` from shifts ``dx``, ``dy`` (um), rotation
    ``angle`` (rad; ``c = cos(angle)``, ``s = sin(angle)``) and magnification ``scale`` > 0, broadcast against each other
    and flattened in C order.  A point xi of mesh A appears in B's frame at ``(dx, dy) + scale R(angle) xi``."""
    try:
        a = [np.asarray(v, dtype=np.float64) for v in (dx, dy, angle, scale)]
        tx, ty, ang, m = np.broadcast_arrays(*a)
    except (TypeError, ValueError):
        raise ValueError("dx, dy, angle and scale must be numbers or arrays that broadcast against each other") from None
    tab = np.stack([tx.ravel(), ty.ravel(), np.cos(ang).ravel(), np.sin(ang).ravel(), m.ravel()], axis=1)
    return _poses(tab)


def _poses(poses) -> np.ndarray:
    """A pose table (T, 5), T >= 1, every entry finite, m > 0, |c^2 + s^2 - 1| <= 1e-12, as contiguous float64."""
    try:
        p = np.ascontiguousarray(np.asarray(poses, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError("poses must be an array of shape (T, 5): (tx, ty, c, s, m) per pose") from None
    if p.ndim != 2 or p.shape[1] != 5 or p.shape[0] < 1:
        raise ValueError("poses must be an array of shape (T, 5) with T >= 1: (tx, ty, c, s, m) per pose")
    if not np.all(np.isfinite(p)):
        raise ValueError("every pose entry must be finite")
    if np.any(p[:, 4] <= 0):
        raise ValueError("the magnification m of every pose must be > 0")
    if np.any(np.abs(p[:, 2] ** 2 + p[:, 3] ** 2 - 1.0) > 1e-12):
        raise ValueError("(c, s) of every pose must be a rotation: |c^2 + s^2 - 1| <= 1e-12")
    return p


def mode_overlap_poses(modes_a: Sequence[Dict], mesh_a, modes_b: Sequence[Dict], mesh_b, poses, weight=None,
                       normalize: bool = False, device: Optional[int] = None) -> np.ndarray:
    """:func:`mode_overlap` under T poses of mesh A relative to mesh B in one call (``plfem_field_overlap_posed``), (T, ka,
    kb).  ``poses`` is a (T, 5) table of rows ``(tx, ty, c, s, m)`` (:func:`pose_table` builds one from shifts, angles and
    magnifications; a caller may also write exact rotations such as ``c = 0, s = 1``): a point xi of mesh A appears in
    B's frame at ``x = t + m R xi``, ``R = [[c, -s], [s, c]]``.  The sum runs over mesh B's six-point rule; each point is
    taken back into A's frame inside the kernel, located there, and A's value is turned by R for vectorial records.  A
    point outside the posed A contributes 0.  ``weight`` as in :func:`mode_overlap`, in B's frame.  The modes are staged
    once for all poses, and the bits of ``O[p]`` do not depend on the other poses.

    There is no amplitude factor for m: the self-overlap of the posed A is ``m^2`` times A's own.  ``normalize=True``
    (``weight=None`` only) gives the power coupling ``|O_ij|^2 / (m^2 O^aa_ii O^bb_jj)``.  Argument errors raise
    ``ValueError`` before anything touches the device."""
    pr = _overlap_pair("mode_overlap_poses", modes_a, mesh_a, modes_b, mesh_b, weight, device, posed=True, poses=poses,
                       normalize=normalize)
    P, ka, kb = pr.P, pr.ka, pr.kb
    T = P.shape[0]
    if not pr.ready:
        return np.zeros((T, ka, kb), dtype=np.float64)
    fa, fb = pr.fa, pr.fb
    sa, sb = fa._stage(pr.va)[0], fb._stage(pr.vb)[0]
    out = np.empty((T, ka, kb), dtype=np.float64)
    fb.stream.synchronize()                     # (B's staging ran on B's stream; the overlap runs on A's)
    fa._work_call("plfem_overlap_posed_work_bytes", {"ka": ka, "kb": kb, "nposes": T}, "plfem_field_overlap_posed",
                  (fa._loc, sa.data_ptr(), ka, pr.indexed, fb._loc, sb.data_ptr(), kb, pr.indexed, pr.va.shape[0], *pr.weight, T,
                   _native._ptr(P)), (out,), loc=fb._loc)
    if not normalize:
        return out
    daa = np.diag(mode_overlap(modes_a, fa, modes_a, fa)).copy()
    dbb = np.diag(mode_overlap(modes_b, fb, modes_b, fb)).copy()
    return out * out / (P[:, 4, None, None] ** 2 * daa[None, :, None] * dbb[None, None, :])


def flux_overlap_poses(modes_a: Sequence[Dict], mesh_a, geometry_a, modes_b: Sequence[Dict], mesh_b, geometry_b, poses,
                       device: Optional[int] = None) -> Dict[str, np.ndarray]:
    """The four raw matrices of the posed cross flux of two vectorial mode sets (``plfem_flux_overlap_posed``), each (T,
    ka, kb), under the pose table of :func:`mode_overlap_poses`: with ``hA' = R hA``, ``gA' = R gA`` at B's quadrature
    point taken into A's frame (``g = -grad (dx hx + dy hy)``, element-wise second derivatives as in
    :meth:`ModeFields.flux_grams`), B's own ``hB``, ``gB``, ``wA = 1 / eps`` of ``geometry_a`` at the point in A's frame and
    ``wB = 1 / eps`` of ``geometry_b`` at B's point,

    ``MA = sum wA hA'_i . hB_j``, ``GA = sum wA gA'_i . hB_j``, ``MB = sum wB hA'_i . hB_j``, ``GB = sum wB hA'_i . gB_j``

    over mesh B's six-point rule.  They are free of beta, k0 and the magnification:
    :func:`.splice.flux_transfer_from_grams` makes the power-normalised transfer from them.  Each geometry is marshalled as
    for :meth:`ModeFields.flux_grams` (its index profile if it carries one, else its discs at ``n_core`` on ``n_clad``); a
    profile with a sampled map is not supported.  Record checks and :class:`ModeFields` reuse as in
    :func:`mode_overlap_poses`; at most 64 pairs of 32-mode chunks.  A scalar record, a sampled map and every other
    argument error raise ``ValueError`` before any device call."""
    ka_kind, va, _ = _records(modes_a)
    kb_kind, vb, _ = _records(modes_b)
    if "scalar" in (ka_kind, kb_kind):
        raise ValueError("flux_overlap_poses: the electric field needs vectorial records")
    P = _poses(poses)
    fa = _as_fields(mesh_a, device)
    fb = fa if (mesh_b is mesh_a or (not isinstance(mesh_b, ModeFields) and not isinstance(mesh_a, ModeFields)
                                     and mesh_key(mesh_b) == mesh_key(mesh_a))) else _as_fields(mesh_b, device)
    mat_a, mat_b = fa._material(geometry_a), fb._material(geometry_b)
    if mat_a.index_map is not None or mat_b.index_map is not None:
        raise ValueError("flux_overlap_poses: an index profile with a sampled map is not supported")
    _, va, _ = fa._check_records(modes_a)
    _, vb, _ = fb._check_records(modes_b)
    ka, kb = (0 if v is None else v.shape[1] for v in (va, vb))
    T = P.shape[0]
    if ka == 0 or kb == 0:
        return {nm: np.zeros((T, ka, kb), dtype=np.float64) for nm in FLUX_OVERLAP_NAMES}
    if ((ka + 31) // 32) * ((kb + 31) // 32) > FLUX_POSE_MAX_CHUNK_PAIRS:
        raise ValueError(f"at most {FLUX_POSE_MAX_CHUNK_PAIRS} pairs of 32-mode chunks per posed flux overlap, got ka = {ka}, "
                         f"kb = {kb}")
    fa._ensure_locator()
    fb._ensure_locator()
    if fa.device != fb.device:
        raise ValueError("both meshes must be evaluated on one device")
    sa, sb = fa._stage(va)[0], fb._stage(vb)[0]
    fa._set_index_map(None)                      # a cached locator carries no map into this call
    fb._set_index_map(None)
    out = np.empty((T, len(FLUX_OVERLAP_NAMES), ka, kb), dtype=np.float64)
    fb.stream.synchronize()                     # (B's staging ran on B's stream; the overlap runs on A's)
    fa._work_call("plfem_flux_overlap_posed_work_bytes", {"ka": ka, "kb": kb, "nposes": T}, "plfem_flux_overlap_posed",
                  (fa._loc, sa.data_ptr(), ka, 1, *fa._material_args(mat_a), fb._loc, sb.data_ptr(), kb, 1,
                   *fb._material_args(mat_b), T, _native._ptr(P)), (out,), loc=fb._loc)
    return {nm: np.ascontiguousarray(out[:, i]) for i, nm in enumerate(FLUX_OVERLAP_NAMES)}


__all__ = ["ModeFields", "mode_overlap", "mode_overlap_poses", "pose_table", "flux_overlap_poses", "FLUX_OVERLAP_NAMES",
           "FLUX_POSE_MAX_CHUNK_PAIRS", "POSE_MAX_CHUNK_PAIRS", "LOC_TOL", "GRAM_NAMES", "CORE_GRAM_NAMES", "MOMENT_GRAM_NAMES", "PROFILE_GRAM_NAMES", "FLUX_GRAM_NAMES",
           "PROJECT_TILE", "PROJECT_MAX_FACTORS", "PROJECT_SAMPLED_TILE", "PROJECT_SAMPLED_MAX_FRAMES",
           "PROJECT_SAMPLED_MAX_PIXELS"]
