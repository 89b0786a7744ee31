"""The cases, the fixed script of ABI calls and the probes of test_gpu_workspace_contents.py: what a context computes must
not depend on what its device memory held before (``_native.SCRATCH_FILL``), on the calls made on it earlier, or on the
pinned blocks, streams and events it inherits from the process-wide pools.  Every result is collected as an array, so
that two runs are compared with ``np.array_equal`` (bit for bit; a NaN equals nothing).

The cases are those of operator_cases.py / pivot_cases.py that reach each structure (no mesh of their own); the driver
settings are those of lanczos_cases.py and test_gpu_lanczos_drivers.py (max_ncv = 65, the tight basis (12, 28) at tol 1e-10:
several thick restarts).  Run as a program (``python workspace_cases.py OUT.npz DEVICE``) this module runs the small probe of the
recycling test as the first context of a fresh process."""
from __future__ import annotations

import functools
import hashlib
import os
import sys

import numpy as np

if __name__ == "__main__":          # the child process of the recycling test: the paths tests/conftest.py sets up
    _here = os.path.dirname(os.path.abspath(__file__))
    for _p in (os.path.dirname(_here), _here):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import front_emulation as fe
import lanczos_cases as lc
import operator_cases as oc
import pivot_cases as pc
from front_checks import right_hand_sides

FILLS = {"zero": 0.0, "zero_again": 0.0, "nan": float("nan"), "huge": 3.0e100}
MAX_NCV = 65                        # lanczos_cases.py: the "c1" and "sca16m65" contexts
K, NCV, TOL = 12, 28, 1e-10         # test_gpu_lanczos_drivers.py: TIGHT[0] at TOL
RESIDUAL_TOL = 1e-7                 # the solvers' a-posteriori bound
PAD_TREE = "sq16_l32_sca"           # pivot_cases.py: scalar, 31 fronts, root with a (true DOF, padding DOF) pair
CASES = ("c1_h05_l24_vec", "c1_h05_l24_sca", "c1_h05_l8_vec", "sq12_one_vec", "sq12_one_sca", PAD_TREE)
SMALL, SMALL_NCV, SMALL_K = "sq12_one_vec", 12, 4       # context B of the recycling tests
LARGE = "c1_h10_vec"                                     # context A
# another mesh with the 6272 elements of the C1 mesh at h = 0.5: the same upload size to within the front-level arrays
SAME_SIZE_SQUARE = oc.Case("sq56_l24_vec", ("square", 56), 24, 2, False, "staging block of c1_h05_l24_vec")


def maxiter_of(dpn):
    return 12000 if dpn == 2 else 6000      # test_gpu_lanczos_drivers.maxiter_of: the solvers' defaults


def c1_geometry():
    """The suite's C1 geometry (tests/conftest.py), for the child process."""
    from pl_fem_vectoriel_amd import MCFGeometry
    return MCFGeometry(7, 8.0, 1.5, 1.535, 1.0, wavelength_um=1.55)


class Data:
    """Host side of a case: mesh, analysis, front tree, pencil parameters, right-hand sides (no device)."""

    def __init__(self, name, geometry):
        from oracle import scalar
        from pl_fem_vectoriel_amd.solver_fem import _core_table, shift_estimate
        self.name = name
        if name in {t.name for t in pc.TREES}:
            self.tree = next(t for t in pc.TREES if t.name == name)
            self.case = self.tree.case
        else:
            self.tree = None
            self.case = next(c for c in oc.CASES + (SAME_SIZE_SQUARE,) if c.name == name)
        self.dpn = self.case.dpn
        self.mesh = oc.mesh_of(self.case, geometry)
        self.sym = oc.symbolic_of(self.case, self.mesh)
        if self.case.mesh[0] == "c1":
            self.g = geometry
            self.sigma = shift_estimate(geometry) if self.dpn == 2 else scalar.shift(geometry)
        else:                               # the squares: the two discs and the shift of lanczos_cases.py
            self.g = lc.SquareGeometry(lc.SQUARE_CORES)
            self.sigma = lc.sigma_of(self.dpn)
        self.cores = _core_table(self.g)
        self.eps_core, self.eps_clad, self.k0 = self.g.n_core ** 2, self.g.n_clad ** 2, self.g.k0
        self.alpha_p = 1.0 if self.dpn == 2 else 0.0
        self.tol_refined = 1e-10 if self.dpn == 2 else 1e-12
        self.N, self.n2, self.nsolve = self.sym.N, self.dpn * self.sym.N, self.sym.nsolve
        self.T = fe.FrontTree(self.sym)
        interior = self.sym.array("interior")
        self.idx = np.concatenate([interior, interior + self.N]) if self.dpn == 2 else np.arange(self.N)
        self.rhs = right_hand_sides(self.T, self.idx, self.N)
        if self.tree is not None and self.tree.pad_pair:
            f, k = self.tree.pad_pair
            fn = self.T.nodes(f)
            assert fn[k] >= 0 and fn[k + 1] < 0 and k + 1 < self.T.s2(f)       # an owned (true DOF, padding DOF) pair

    @functools.cached_property
    def pencil(self):
        """A - sigma B on the unknowns from the ORACLE's assembly (nothing of the device in it)."""
        from oracle import hfield, scalar
        from oracle.p2 import MeshTriLite
        om = MeshTriLite(self.mesh.p, self.mesh.t)
        if self.dpn == 2:
            A, B, basis = hfield.assemble_hfield_system_fused(self.g, om, eliminate_zeros=False)[:3]
            A_int, B_int, interior = hfield.restrict_interior(A, B, basis)
            assert np.array_equal(interior, self.sym.array("interior"))
            return (A_int - self.sigma * B_int).tocsc()
        Ks, M, Me, _ = scalar.assemble(self.g, om, eliminate_zeros=False)
        return (Ks - self.k0 ** 2 * Me - self.sigma * M).tocsc()

    # -- device ----------------------------------------------------------------------------------------------------
    def context(self, device, max_ncv=MAX_NCV):
        from pl_fem_vectoriel_amd import _native
        return _native.Context(self.sym, device, max_ncv=max_ncv)

    def assemble(self, ctx, cores=None, eps_core=None, k0=None):
        cores = self.cores if cores is None else cores
        eps_core = self.eps_core if eps_core is None else eps_core
        k0 = self.k0 if k0 is None else k0
        if self.dpn == 2:
            ctx.assemble(cores, eps_core, self.eps_clad, k0, self.alpha_p)
        else:
            ctx.assemble_scalar(cores, eps_core, self.eps_clad, k0)

    def solve_modes(self, ctx, k=K, ncv=NCV, cores=None, eps_core=None, k0=None, sigma=None):
        """plfem_solve_modes with the solvers' bounds; the pinned host block of the interior vectors starts as NaN."""
        import torch
        host = torch.full((k, self.dpn * self.nsolve), float("nan"), dtype=torch.float64).pin_memory()
        res = ctx.solve_modes(self.cores if cores is None else cores, self.eps_core if eps_core is None else eps_core,
                              self.eps_clad, self.k0 if k0 is None else k0, self.alpha_p,
                              self.sigma if sigma is None else sigma, k, ncv, TOL, maxiter_of(self.dpn), RESIDUAL_TOL,
                              self.tol_refined, modes_host=host)
        return res + (host.numpy().copy(),)


_cache = {}


def data(name, geometry):
    """(cached: the geometry is the suite's one C1 geometry)"""
    if name not in _cache:
        _cache[name] = Data(name, geometry)
    return _cache[name]


def dev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(ctx.tdev)


LANCZOS_STATS = ("nconv", "n_opinv", "restarts", "max_rel_res", "n_block_solves")       # of Context.lanczos


def modes_stats_names():
    """The entries of the stats of Context.solve_modes that are no timings."""
    from pl_fem_vectoriel_amd import _native
    return tuple(k for k in _native.SOLVE_STATS if not k.endswith("_us"))


def stats_array(st, names):
    return np.array([float(st[k]) for k in names])


def named(values, names):
    assert len(values) == len(names)
    return dict(zip(names, values))


def factor_internals(T, ctx):
    """What the emulation defines of the factor (front_emulation.FrontTree.device_front: [F11; F21] and Z^T of every
    front; D^-1 of its owned rows), one digest per front -- never the raw buffers with their unwritten padding.  Returns
    {"factor_digest": (nf, 16) uint8, "factor_nonfinite": number of non-finite entries}."""
    dump = ctx.debug_copy("front", 0, int(T.sym.info["front_doubles"]))
    delta = ctx.debug_copy("delta", 0, 4 * int(T.fptr[T.nf]))
    digest = np.zeros((T.nf, 16), dtype=np.uint8)
    bad = 0
    for f in range(T.nf):
        s2 = T.s2(f)
        F = T.device_front(ctx, f, dump=dump)
        parts = np.concatenate([F[:, :s2].ravel(), F[:s2, s2:].ravel(), delta[4 * int(T.fptr[f]):4 * int(T.fptr[f]) + 2 * s2]])
        bad += int((~np.isfinite(parts)).sum())
        digest[f] = np.frombuffer(hashlib.blake2b(parts.tobytes(), digest_size=16).digest(), dtype=np.uint8)
    return {"factor_digest": digest, "factor_nonfinite": np.array([bad])}


def run_script(d, device):
    """The fixed script on a NEW context of case d (created under whatever _native.SCRATCH_FILL holds): every result."""
    from pl_fem_vectoriel_amd import _native
    import torch
    out = {}
    ctx = d.context(device)
    try:
        d.assemble(ctx)                                                               # 1
        for b in _native.BLOCKS:
            out[f"block_{b}"] = ctx.block_values(b)
        b0 = dev(ctx, d.rhs["random"])
        out["spmv_A"] = ctx.spmv("A", b0).cpu().numpy()                               # 2
        out["spmv_B"] = ctx.spmv("B", b0).cpu().numpy()
        ctx.factor(d.sigma)                                                           # 3
        out.update(factor_internals(d.T, ctx))
        out["perturbations"] = np.array([ctx.timings()["pivot_perturbations"]])       # 4
        out["solve_r0"] = ctx.solve(b0, 0).cpu().numpy()                              # 5
        out["solve_r1"] = ctx.solve(b0, 1).cpu().numpy()
        P = fe.BLOCK_P
        bd = dev(ctx, np.concatenate([d.rhs[k] for k in ("random", "leaf", "root", "random2")]))
        xd = _native.device_output((P * d.n2,), torch.float64, ctx.tdev)
        ctx.debug_solve_block(bd, xd, d.n2)                                           # 6
        out["solve_block"] = xd.cpu().numpy()
        out["solve_r0_again"] = ctx.solve(b0, 0).cpu().numpy()                        # 7: P = 1 layout of d_fvec after P = 4
        evals, evecs, st = ctx.lanczos(K, NCV, TOL, maxiter_of(d.dpn), d.sigma)       # 8
        out["lanczos_evals"], out["lanczos_evecs"], out["lanczos_stats"] = evals, evecs.cpu().numpy(), stats_array(st, LANCZOS_STATS)
        post, frac, mint = ctx.postprocess(evecs, d.cores, True)                      # 9 (scales evecs in place)
        out["post"], out["post_frac"], out["post_interior"] = post, np.array([frac]), mint.cpu().numpy()
        post2, frac2, _ = ctx.postprocess(evecs, d.cores, False)
        out["post_again"], out["post_frac_again"], out["evecs_scaled"] = post2, np.array([frac2]), evecs.cpu().numpy()
        out["residuals"] = ctx.residuals(evals, evecs)                                # 10
        evals, post, frac, resid, st, host = d.solve_modes(ctx)                       # 11
        out["modes_evals"], out["modes_post"], out["modes_frac"], out["modes_resid"] = evals, post, np.array([frac]), resid
        out["modes_int"], out["modes_dev"] = host, ctx.modes_dev().cpu().numpy()
        out["modes_stats"] = stats_array(st, modes_stats_names())
    finally:
        ctx.close()
    return out


def differences(a, b):
    """[(key, entries that differ, first index)] of two result dictionaries (bit for bit, NaN unequal to everything)."""
    out = []
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b or a[k].shape != b[k].shape:
            out.append((k, "missing or shape", None))
        elif not np.array_equal(a[k], b[k]):
            ne = np.asarray(a[k] != b[k])
            out.append((k, int(ne.sum()), tuple(int(v) for v in np.argwhere(ne)[0])))
    return out


# ---- probes of the call-history and recycling tests ---------------------------------------------------------------------
def probe_modes(ctx, d, k=K, ncv=NCV, **pencil):
    evals, post, frac, resid, st, host = d.solve_modes(ctx, k, ncv, **pencil)
    return {"evals": evals, "post": post, "frac": np.array([frac]), "resid": resid, "modes_int": host, "stats": stats_array(st, modes_stats_names()),
            "modes_dev": ctx.modes_dev().cpu().numpy()}, st


def probe_eigs(ctx, d, sigma=None, k=K, ncv=NCV):
    """factor + lanczos + postprocess on the assembled pencil."""
    sigma = d.sigma if sigma is None else sigma
    ctx.factor(sigma)
    evals, evecs, st = ctx.lanczos(k, ncv, TOL, maxiter_of(d.dpn), sigma)
    raw = evecs.cpu().numpy()
    post, frac, mint = ctx.postprocess(evecs, d.cores, True)
    return {"evals": evals, "evecs": raw, "stats": stats_array(st, LANCZOS_STATS), "post": post, "frac": np.array([frac]),
            "modes_int": mint.cpu().numpy(), "perturbations": np.array([ctx.timings()["pivot_perturbations"]])}


def probe_solves(ctx, d, order):
    """Single (P = 1) and block (P = 4) solves on the factor the context holds, in the given order of "single" / "block"."""
    from pl_fem_vectoriel_amd import _native
    import torch
    out = {}
    b0 = dev(ctx, d.rhs["random"])
    bd = dev(ctx, np.concatenate([d.rhs[k] for k in ("random", "leaf", "root", "random2")]))
    for what in order:
        if what == "single":
            out["single"] = ctx.solve(b0, 0).cpu().numpy()
        else:
            xd = _native.device_output((fe.BLOCK_P * d.n2,), torch.float64, ctx.tdev)
            ctx.debug_solve_block(bd, xd, d.n2)
            out["block"] = xd.cpu().numpy()
    return out


def small_probe(device, geometry):
    """The probe of the recycling tests on a new small context (closed before returning)."""
    d = data(SMALL, geometry)
    ctx = d.context(device, max_ncv=SMALL_NCV)
    try:
        return probe_modes(ctx, d, SMALL_K, SMALL_NCV)[0]
    finally:
        ctx.close()


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available()
    np.savez(sys.argv[1], **small_probe(int(sys.argv[2]), c1_geometry()))
