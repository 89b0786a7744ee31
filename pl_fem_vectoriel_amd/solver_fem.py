"""Drop-in for the vectorial half of the reference ``solver_fem.py`` on MI355X.

Class / method surface follows the reference code (``solver_fem.py:113-239``):

* ``TrueVectorialMaxwellSolver(geometry, use_pml=False)``; attributes ``geometry``, ``k0``, ``use_pml``;
* ``assemble_hfield_system(mesh) -> (A, B, basis, Dxx, Dyy, Dxy, M_inv)`` — SciPy CSR matrices
  (``A``, ``B`` 2N x 2N in the block order Hx then Hy; the others N x N) and a basis object exposing
  ``N``, ``doflocs``, ``element_dofs`` and ``get_dofs().all()``;
* ``solve_vectorial_modes(mesh, n_modes_target=20) -> List[Dict]`` with the dict keys of
  ``solver_fem.py:222-225`` (``Ex_dofs`` / ``Ey_dofs`` hold the Hx / Hy interior DOF vectors);

plus the documented convenience form of the reference README (``README.md:137-160``):
``TrueVectorialMaxwellSolver(geom, n_modes=10).solve()`` with attribute access on the modes.

All arithmetic of the path runs in ``libplfem_hip.so`` (``include/plfem.h``); this file only holds
the host logic the reference also keeps in Python: the shift estimate, the request size, the n_eff
window, the divergence / radiation filters and the ordering (``solver_fem.py:187-196,205-239``).
"""
from __future__ import annotations

import logging
import time
from typing import Dict, List, Optional

import numpy as np

from . import _native
from .mesh import TriMesh, generate_mesh
from .profile import index_profile_of

logger = logging.getLogger("pl_v18.solver_fem")   # same logger name as the reference (solver_fem.py:40)


try:                                   # 64-bit content hash of the mesh arrays: 40 us for C1 with xxh3
    from xxhash import xxh3_64_intdigest as _digest
except ImportError:                    # pragma: no cover  (zlib is ~10 x slower, still far below one analysis)
    from zlib import adler32 as _digest


def mesh_key(mesh):
    """Cache key of a mesh by CONTENT (shapes + a hash of the bytes of ``p`` and ``t``), not by object identity: a caller
    that edits ``mesh.p`` in place between two calls (same object, same shapes) must not get the analysis of the old
    coordinates back, and two equal meshes may share one (the reference keeps no state at all)."""
    p = np.ascontiguousarray(mesh.p, dtype=np.float64)
    t = np.ascontiguousarray(mesh.t)
    return (p.shape[1], t.shape[1], t.dtype.str, _digest(p), _digest(t))


def _copy_stream(device: int):
    """One side stream per device for the device-to-host copy of the mode vectors (created once: ~50 us)."""
    import torch
    s = _COPY_STREAMS.get(device)
    if s is None:
        s = _COPY_STREAMS[device] = torch.cuda.Stream(device=device)
    return s


class ModeDict(dict):
    """Mode record: a ``dict`` (code form) that also answers attribute access (README form)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


class _DofsView:
    def __init__(self, dofs):
        self._d = dofs

    def all(self):
        return self._d


class P2BasisView:
    """What the reference reads of ``Basis(mesh, ElementTriP2())`` (``solver_fem.py:127,179,183``)."""

    def __init__(self, sym: "_native.Symbolic"):
        self.N = sym.N
        self.nvertices = sym.nv
        self.doflocs = sym.array("doflocs").reshape(2, sym.N)
        self.element_dofs = sym.array("edof").reshape(6, sym.ne)
        self._boundary = np.nonzero(sym.array("bmask"))[0]
        self.interior_dofs = sym.array("interior").astype(np.int64)

    def get_dofs(self):
        return _DofsView(self._boundary)


def shift_estimate(geometry) -> float:
    """LP01 b-V estimate of the shift (``solver_fem.py:187-193``)."""
    n_core, n_clad = geometry.n_core, geometry.n_clad
    NA = np.sqrt(max(n_core ** 2 - n_clad ** 2, 1e-6))
    r_mean = np.mean(geometry.core_radii)
    V_geom = geometry.k0 * r_mean * NA
    b_approx = max((1.0 - 2.405 / max(V_geom, 2.41)) ** 2, 0.05)
    n_eff_est = np.sqrt(n_clad ** 2 + b_approx * (n_core ** 2 - n_clad ** 2))
    return float((geometry.k0 * float(np.clip(n_eff_est, n_clad + 0.05, n_core - 0.005))) ** 2)


def _n_eff_shift(n_eff_shift) -> Optional[float]:
    if n_eff_shift is None:
        return None
    try:
        n = float(n_eff_shift)
    except (TypeError, ValueError):
        raise ValueError("n_eff_shift must be a positive number") from None
    if not (np.isfinite(n) and n > 0):
        raise ValueError("n_eff_shift must be a positive number")
    return n


def _core_table(geometry) -> np.ndarray:
    pos = np.atleast_2d(np.asarray(geometry.positions, dtype=np.float64))
    rad = np.asarray(geometry.core_radii, dtype=np.float64).reshape(-1)
    return np.ascontiguousarray(np.column_stack([pos, rad]))


def _classify(ratio: float) -> str:
    # solver_fem.py:100-105
    if ratio > 10.0:
        return "TE-like"
    if ratio > 2.5:
        return "HE-like"
    if ratio > 0.4:
        return "Hybrid"
    if ratio > 0.1:
        return "EH-like"
    return "TM-like"


class TrueVectorialMaxwellSolver:
    """Vectorial H-field eigenmode solver, MI355X backend.

    Extra keyword arguments (not in the reference) are all optional: ``n_modes`` (README form),
    ``device`` (HIP device index), ``eig_tol`` (Ritz residual tolerance ``||r|| <= tol |theta|``, tested after every
    block step: default 1e-8, ten times tighter than the 1e-7 the reference hands to eigsh -- ARPACK only tests at its
    restarts and ends far below its tolerance, this driver stops at the first step that meets it; measured at C1 the
    fields then agree with ``eigsh`` to 3e-9, as they do at 1e-10, for two block steps less), ``leaf_elems`` (front-tree leaf
    size), ``reuse_symbolic`` (keep the mesh-only analysis and the device context between calls on
    the same mesh object — e.g. a wavelength sweep), ``mesh_levels`` / ``mesh_refinement`` for
    ``solve()``; ``n_eff_shift``: the shift is ``(k0 n_eff_shift)^2`` instead of the LP01 estimate, which means nothing for
    e.g. a jacketed low-contrast section.  A geometry that carries an index profile (``geometry.index_profile``,
    :class:`.profile.ProfiledGeometry`) is assembled with it; every entry that assembles sets or clears the profile of
    the cached context itself, so no solve inherits the previous one's.
    """

    ALPHA_P = 1.0            # solver_fem.py:158
    REF_TOL = 1e-7           # solver_fem.py:197
    MAXITER = 12000          # solver_fem.py:197
    OVERSAMPLE = 12          # solver_fem.py:196
    BASIS_FACTOR = 6         # Lanczos basis = 6 k columns (SciPy's default is 2k + 1): the driver tests convergence
    BASIS_MAX = 160          # after every block step, so a long basis costs memory, not work, and avoids restarts
    BASIS_BYTES = 16e9       # cap of the four basis panels (V, BV and their restart doubles)
    RESIDUAL_TOL = 1e-7      # a-posteriori bound on ||A v - lambda B v|| / ||A v|| of every returned pair

    def __init__(self, geometry, use_pml: bool = False, n_modes: Optional[int] = None, device: Optional[int] = None,
                 eig_tol: float = 1e-8, leaf_elems: int = 0, reuse_symbolic: bool = True, mesh_refinement: float = 1.0,
                 mesh_levels: int = 1, refine_steps: int = 0, profile_kernel: bool = False,
                 n_eff_shift: Optional[float] = None):
        _native.load_library()           # fail loudly: the reference raises RuntimeError when its backend is missing
        self.geometry = geometry
        self.n_eff_shift = _n_eff_shift(n_eff_shift)
        self.k0 = geometry.k0
        self.use_pml = use_pml           # stored, never read — as in the reference
        self.n_modes = n_modes
        self.device = device
        self.eig_tol = float(eig_tol)
        self.leaf_elems = int(leaf_elems)
        self.reuse_symbolic = bool(reuse_symbolic)
        self.mesh_refinement = mesh_refinement
        self.mesh_levels = mesh_levels
        self.refine_steps = int(refine_steps)
        self.profile_kernel = bool(profile_kernel)   # HIP-event timing of the dominant kernel (bench.py roofline)
        self._cache = {}
        self.last_stats: Dict = {}
        logger.info(f"Solveur H-field initialisé - k₀={self.k0:.4f} µm⁻¹")

    # -- symbolic / context management -------------------------------------------------------------
    def adopt_analysis(self, mesh, sym: "_native.Symbolic") -> None:
        """Install a mesh-only analysis built elsewhere (e.g. on a background thread while the GPU
        was busy with the previous cross-section of a sweep) for ``mesh``."""
        self._cache.clear()
        self._cache[mesh_key(mesh)] = {
            "sym": sym, "ctx": None, "basis": None, "t_symbolic": 0.0, "mesh": mesh}

    def _analysis(self, mesh, need_ctx: bool, max_ncv: int = 65):
        key = mesh_key(mesh) if self.reuse_symbolic else None
        ent = self._cache.get(key) if self.reuse_symbolic else None
        if ent is None:
            t0 = time.perf_counter()
            sym = _native.Symbolic(mesh.p, mesh.t, leaf_elems=self.leaf_elems)
            ent = {"sym": sym, "ctx": None, "basis": None, "t_symbolic": time.perf_counter() - t0, "mesh": mesh}
            if self.reuse_symbolic:
                self._cache.clear()          # one mesh at a time: contexts own GBs of HBM
                self._cache[key] = ent
        if need_ctx and (ent["ctx"] is None or ent["ctx"].max_ncv < max_ncv):
            if ent["ctx"] is not None:
                ent["ctx"].close()
            t0 = time.perf_counter()
            ent["ctx"] = _native.Context(ent["sym"], self.device, max_ncv=max(max_ncv, 65))
            ent["t_context"] = time.perf_counter() - t0
            ent["t_workspace"] = ent["ctx"].t_workspace
        return ent

    def _basis_size(self, k: int, n2: int) -> int:
        floor = max(2 * k + 1, 20)           # SciPy's ncv (scipy arpack.py:306-311): never below it
        if floor > _native.MAX_NCV:
            raise ValueError(f"n_modes_target too large: k = {k} eigenpairs need a Lanczos basis of {floor} columns, "
                             f"the device context holds at most {_native.MAX_NCV} (k <= {(_native.MAX_NCV - 1) // 2})")
        by_memory = int(self.BASIS_BYTES // (32 * max(n2, 1)))
        return max(floor, min(self.BASIS_FACTOR * k, self.BASIS_MAX, max(by_memory, floor)))

    def clear_cache(self):
        for ent in self._cache.values():
            if ent["ctx"] is not None:
                ent["ctx"].close()
        self._cache.clear()

    def _assemble_device(self, ctx):
        g = self.geometry
        ctx.set_index_profile(index_profile_of(g))
        ctx.assemble(_core_table(g), g.n_core ** 2, g.n_clad ** 2, self.k0, self.ALPHA_P)

    # -- reference surface ---------------------------------------------------------------------------
    def assemble_hfield_system(self, mesh):
        """Assemblage des matrices H-field 2N×2N (``solver_fem.py:122-169``), computed on the GPU."""
        import scipy.sparse as sp

        ent = self._analysis(mesh, need_ctx=True)
        sym, ctx = ent["sym"], ent["ctx"]
        self._assemble_device(ctx)
        N = sym.N
        rowptr = sym.array("rowptr")
        colind = sym.array("colind")

        def blk(name):
            # asm() -> COOData.tocsr() drops explicit zeros (e.g. the vertex / adjacent-edge
            # mass entries vanish on every element), so the structural zeros of the shared pattern go too
            # (eliminate_zeros works in place: every block gets its own copy of the shared index arrays)
            m = sp.csr_matrix((ctx.block_values(name), colind.copy(), rowptr.copy()), shape=(N, N))
            m.eliminate_zeros()
            return m

        A = sp.bmat([[blk("Axx"), blk("Axy")], [blk("Ayx"), blk("Ayy")]], format="csr")
        M_inv = blk("Minv")
        B = sp.bmat([[M_inv, None], [None, M_inv]], format="csr")
        if ent["basis"] is None:
            ent["basis"] = P2BasisView(sym)
        logger.info(f"Assemblage terminé - {N} DOFs P2, matrice {2 * N}×{2 * N}")
        return A, B, ent["basis"], blk("Dxx"), blk("Dyy"), blk("Dxy"), M_inv

    def solve_vectorial_modes(self, mesh, n_modes_target: int = 20) -> List[Dict]:
        """Résout [A]{Ht} = β² [B]{Ht} (``solver_fem.py:171-239``) on the GPU."""
        g = self.geometry
        t_start = time.perf_counter()
        # request size: solver_fem.py:196; Lanczos basis: see BASIS_FACTOR (never below scipy's max(2k+1, 20))
        nv, ne = mesh.p.shape[1], mesh.t.shape[1]
        n_req_guess = n_modes_target + self.OVERSAMPLE
        ent = self._analysis(mesh, need_ctx=True, max_ncv=self._basis_size(n_req_guess, 2 * (nv + 2 * ne)))
        sym, ctx = ent["sym"], ent["ctx"]
        N_solve = sym.nsolve
        n_req = min(n_modes_target + self.OVERSAMPLE, 2 * N_solve - 4)
        if n_req < 1:
            raise ValueError("mesh too small for the requested number of modes")
        ncv = min(self._basis_size(n_req, 2 * sym.N), 2 * N_solve, ctx.max_ncv)
        cores = _core_table(g)
        sigma = shift_estimate(g) if self.n_eff_shift is None else float((self.k0 * self.n_eff_shift) ** 2)
        ctx.set_index_profile(index_profile_of(g))
        import torch
        # (k, 2 N_solve) on the host: the caller owns NumPy arrays, as in the reference.  They live in pinned memory
        # from torch's caching host allocator, so a released mode list hands its 32 MB block to the next solve
        # (no first-touch page faults, no munmap) and the copy runs at full PCIe rate.
        t0 = time.perf_counter()
        host = torch.empty((n_req, 2 * N_solve), dtype=torch.float64, pin_memory=True)
        t_pinned = time.perf_counter() - t0
        if self.profile_kernel:
            ctx.profile_begin(4096)
        ctx.set_option("refine_steps", self.refine_steps)
        # ONE call into the library (plfem_solve_modes): assembly, factorisation, eigen-solve, post-processing, the
        # a-posteriori guard and the copy of the mode vectors.  The guard: the LDL^T pivots statically and the Lanczos
        # convergence test trusts K^-1, so every solve is checked against the ASSEMBLED pencil; a failed check (or a
        # perturbed pivot) re-runs the eigen-solve with iterative refinement inside the operator and a tighter Ritz
        # tolerance, and a second failure is an error (RuntimeError), never a silent result.
        t0 = time.perf_counter()
        evals, post, frac_core, resid, st = ctx.solve_modes(cores, g.n_core ** 2, g.n_clad ** 2, self.k0, self.ALPHA_P, sigma,
                                                            n_req, ncv, self.eig_tol, self.MAXITER, self.RESIDUAL_TOL, 1e-10,
                                                            modes_host=host)
        t1 = time.perf_counter()
        if st["refined"]:
            logger.warning(f"eigenpairs failed the a-posteriori check (residual {st['true_residual_first']:.2e}, "
                           f"{st['pivot_perturbations']} perturbed pivots): re-ran with refinement -> {st['true_residual']:.2e}")
        if self.profile_kernel:
            st = dict(st, kernel_profile=ctx.profile_end())
        vecs = host.numpy()
        st = dict(st, t_pinned=t_pinned, t_call=t1 - t0)
        if not self.reuse_symbolic:
            # nothing will reuse the analysis or the context: release them now, so the device workspace goes back
            # to the allocator before the next solve asks for one
            ctx.close()
            ent["ctx"] = None

        # The per-mode scalars of solver_fem.py:205-225 for all k pairs at once (the same IEEE operations as the reference's
        # scalar NumPy arithmetic; 22 x a dozen NumPy scalar calls cost 0.3 ms of a 21-ms solve when done one by one)
        n_core, n_clad = g.n_core, g.n_clad
        b2 = np.asarray(evals, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            beta = np.sqrt(np.where(b2 > 0, b2, 0.0))
            ne_ = beta / self.k0
            keep = (b2 > 0) & ~((ne_ <= n_clad) | (ne_ >= n_core * 1.01))          # :208, :210
            div_ratio = post[:, 1] / np.maximum(b2, 1e-12)                             # :214
            cx, cy, ax, ay = post[:, 2], post[:, 3], post[:, 4], post[:, 5]
            conf = (cx + cy) / (ax + ay)
            # _polarization_from_interp (solver_fem.py:88-107); whole-domain fallback if no core DOF
            P_x, P_y = ((cx, cy) if frac_core > 0 else (ax, ay))
            P_x, P_y = P_x + 1e-30, P_y + 1e-30
            PDL = np.clip(10.0 * np.log10(np.maximum(P_x, P_y) / np.minimum(P_x, P_y)), 0.0, 50.0)
            ratio = P_x / P_y
        cols = [c.tolist() for c in (ne_, beta, P_x, P_y, PDL, ratio, conf, div_ratio)]
        modes_raw = []
        for i in np.nonzero(keep)[0].tolist():
            conf_raw = cols[6][i]
            modes_raw.append(ModeDict({
                "n_eff": cols[0][i], "beta": cols[1][i],
                "Ex_dofs": vecs[i, :N_solve], "Ey_dofs": vecs[i, N_solve:],
                "P_x": cols[2][i], "P_y": cols[3][i], "PDL_dB": cols[4][i], "polarization": _classify(cols[5][i]),
                "confinement": conf_raw, "core_overlap": conf_raw, "div_ratio": cols[7][i],
                "is_vectorial": True, "method": "H-field_V18.10"}))
        # beta_sq: the n_req eigenvalues as the eigen-solver returned them (ascending), before the reference's filters
        self.last_stats = dict(st, sigma=sigma, n_req=n_req, ncv=ncv, N=sym.N, N_solve=N_solve, n=2 * N_solve,
                               beta_sq=np.array(evals, dtype=np.float64),
                               t_symbolic=ent.get("t_symbolic", 0.0), t_context=ent.get("t_context", 0.0),
                               t_workspace=ent.get("t_workspace", 0.0), frac_core=frac_core)
        if not modes_raw:
            self.last_stats["t_total"] = time.perf_counter() - t_start
            return []       # the reference would raise on np.median([]) (solver_fem.py:229); SURVEY.md §5
        # divergence filter, solver_fem.py:228-231
        dr = np.array([m["div_ratio"] for m in modes_raw])
        dr_thresh = max(np.median(dr) * 10, dr.min() * 50, 1e-6)
        modes_phys = [m for m in modes_raw if m["div_ratio"] <= dr_thresh]
        # radiation filter with fallback, solver_fem.py:234-236
        conf_threshold_rad = max(5.0 * frac_core, 0.05)
        modes_guided = [m for m in modes_phys if m["confinement"] >= conf_threshold_rad]
        if not modes_guided:
            modes_guided = modes_phys
        modes_guided.sort(key=lambda x: x["n_eff"], reverse=True)
        self.last_stats["t_total"] = time.perf_counter() - t_start
        return modes_guided

    # -- documented convenience form (reference README.md:149-160) -----------------------------------
    def solve(self, mesh=None) -> List[Dict]:
        if mesh is None:
            mesh = generate_mesh(self.geometry, self.mesh_refinement, self.mesh_levels)
        n = self.n_modes if self.n_modes is not None else 20
        return self.solve_vectorial_modes(mesh, n_modes_target=n)


class ScalarHelmholtzSolver:
    """Scalar P2 solver of the reference (``solver_fem.py:245-276``) on the same device machinery
    with ONE unknown per node: ``(K - k0^2 M_eps) u = lambda M u`` on all P2 DOFs (natural boundary), ``lambda = -beta^2``,
    ``sigma = -(k0 (n_core - 0.008))^2``, ``k = min(n_modes_target + 8, N - 4)``.

    ``ScalarHelmholtzSolver(geometry).solve(mesh, n_modes_target=20)`` returns the reference's list of dicts
    (``n_eff, beta, field_vector, confinement, core_overlap, PDL_dB = 0.0, polarization = 'scalar',
    is_vectorial = False``), n_eff descending.  Optional keywords as for the vectorial class (``device``, ``eig_tol``:
    the reference passes ``tol=1e-6`` to eigsh; the default here stays at 1e-10 -- the shift of this pencil is far from
    its eigenvalues in relative terms, so a Ritz residual of 1e-8 |theta| already is an eigen-residual of 5e-7 against
    the assembled pencil, above the bound of the a-posteriori check; ``leaf_elems``; ``n_eff_shift``: ``sigma =
    -(k0 n_eff_shift)^2``).  A geometry with an index profile is assembled with it, as in the vectorial class."""

    REF_TOL = 1e-6           # solver_fem.py:261
    MAXITER = 6000           # solver_fem.py:261
    OVERSAMPLE = 8           # solver_fem.py:261
    RESIDUAL_TOL = 1e-7
    BASIS_FACTOR, BASIS_MAX, BASIS_BYTES = TrueVectorialMaxwellSolver.BASIS_FACTOR, TrueVectorialMaxwellSolver.BASIS_MAX, TrueVectorialMaxwellSolver.BASIS_BYTES

    def __init__(self, geometry, device: Optional[int] = None, eig_tol: float = 1e-10, leaf_elems: int = 0,
                 n_eff_shift: Optional[float] = None):
        _native.load_library()
        self.geometry = geometry
        self.n_eff_shift = _n_eff_shift(n_eff_shift)
        self.k0 = geometry.k0
        self.device = device
        self.eig_tol = float(eig_tol)
        self.leaf_elems = int(leaf_elems)
        self._cache = {}
        self.last_stats: Dict = {}

    _basis_size = TrueVectorialMaxwellSolver._basis_size

    def clear_cache(self):
        for ent in self._cache.values():
            if ent["ctx"] is not None:
                ent["ctx"].close()
        self._cache.clear()

    def solve(self, mesh, n_modes_target: int = 20) -> List[Dict]:
        g = self.geometry
        t_start = time.perf_counter()
        key = mesh_key(mesh)
        ent = self._cache.get(key)
        if ent is None:
            self.clear_cache()
            t0 = time.perf_counter()
            sym = _native.Symbolic(mesh.p, mesh.t, leaf_elems=self.leaf_elems, dofs_per_node=1, dirichlet=False)
            ent = self._cache[key] = {"sym": sym, "ctx": None, "mesh": mesh, "t_symbolic": time.perf_counter() - t0}
        sym = ent["sym"]
        N = sym.N
        n_req = min(n_modes_target + self.OVERSAMPLE, N - 4)                 # solver_fem.py:261
        if n_req < 1:
            raise ValueError("mesh too small for the requested number of modes")
        ncv = min(self._basis_size(n_req, N), N)
        if ent["ctx"] is None or ent["ctx"].max_ncv < ncv:
            if ent["ctx"] is not None:
                ent["ctx"].close()
            ent["ctx"] = _native.Context(sym, self.device, max_ncv=max(ncv, 65))
        ctx = ent["ctx"]
        cores = _core_table(g)
        sigma = float(-(self.k0 * (g.n_core - 0.008 if self.n_eff_shift is None else self.n_eff_shift)) ** 2)   # solver_fem.py:260
        ctx.set_index_profile(index_profile_of(g))
        import torch
        host = torch.empty((n_req, N), dtype=torch.float64, pin_memory=True)
        # one call (plfem_solve_modes on a scalar context): K - k0^2 M_eps and M, factorisation, eigen-solve, the
        # M-normalisation of solver_fem.py:268, the a-posteriori guard (second pass at 1e-12) and the copy of the fields
        evals, post, _frac, resid, st = ctx.solve_modes(cores, g.n_core ** 2, g.n_clad ** 2, self.k0, 0.0, sigma, n_req, ncv,
                                                        self.eig_tol, self.MAXITER, self.RESIDUAL_TOL, 1e-12, modes_host=host)
        if st["refined"]:
            logger.warning(f"scalar eigenpairs failed the a-posteriori check (residual {st['true_residual_first']:.2e}): "
                           f"re-ran with refinement -> {st['true_residual']:.2e}")
        vecs = host.numpy()
        modes = []
        for i in range(len(evals)):
            lam = float(evals[i])
            if lam >= 0:                                                     # solver_fem.py:265
                continue
            ne_ = np.sqrt(-lam) / self.k0
            if ne_ <= g.n_clad or ne_ >= g.n_core * 1.005:                   # solver_fem.py:267
                continue
            conf = float(post[i, 2] / post[i, 4])                            # sum_core v^2 / sum v^2
            modes.append(ModeDict({"n_eff": float(ne_), "beta": float(self.k0 * ne_), "field_vector": vecs[i],
                                   "confinement": conf, "core_overlap": conf, "PDL_dB": 0.0, "polarization": "scalar",
                                   "is_vectorial": False}))
        modes.sort(key=lambda x: x["n_eff"], reverse=True)
        self.last_stats = dict(st, sigma=sigma, n_req=n_req, ncv=ncv, N=N, t_symbolic=ent.get("t_symbolic", 0.0),
                               t_total=time.perf_counter() - t_start)
        return modes


__all__ = ["TrueVectorialMaxwellSolver", "ScalarHelmholtzSolver", "ModeDict", "P2BasisView", "shift_estimate", "TriMesh"]
