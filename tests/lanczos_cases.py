"""The contexts the Lanczos tests run on, shared by test_gpu_lanczos_kernels.py and test_gpu_lanczos_drivers.py (the
``cases`` fixture is imported by both), and the host side of the same problems: the oracle's pencils of the 16-square
and of its triple, for the host tests of the driver restatement (test_lanczos_emulation_host.py)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import lanczos_emulation as le

P = le.BLOCK_P
SQUARE_CORES = np.array([[0.5, 0.5, 0.2937], [0.21, 0.77, 0.1113]])      # no DOF of the squares on a circle
K0 = 2 * np.pi / 1.55
N_CORE, N_CLAD = 1.535, 1.0
NCOLS = (1, 2, 3, 4, 5, 15, 16, 17, 33, 129)            # + max_ncv + P
NCOLS_LARGE = (1, 5, 17, 33)
CASES = ("sca16", "vec16", "sca255", "c1")
# the driver tests' own contexts: the 16-square under max_ncv = 65 and three copies of it in one mesh (every eigenvalue
# three times)
SQUARES = {"sca16": (16, 1, 160, 1), "vec16": (16, 2, 160, 1), "sca255": (255, 1, 65, 1), "sca16m65": (16, 1, 65, 1),
           "sca16x3": (16, 1, 160, 3), "vec16x3": (16, 2, 160, 3)}
ALL_CASES = CASES + ("sca16m65", "sca16x3", "vec16x3")


def sigma_of(dpn):
    """The shift of the driver tests: +(1.3 k0)^2 (lambda = beta^2) vectorial, -(1.3 k0)^2 (lambda = -beta^2) scalar."""
    return (K0 * 1.3) ** 2 * (1 if dpn == 2 else -1)


def square_mesh(n, copies=1):
    """(p, t, cores) of the n-square, or of ``copies`` of it side by side (le.triple_mesh)."""
    from pl_fem_vectoriel_amd.mesh import unit_square_mesh
    mesh = unit_square_mesh(n)
    if copies == 1:
        return mesh.p, mesh.t, SQUARE_CORES
    return le.triple_mesh(mesh.p, mesh.t, SQUARE_CORES, shifts=tuple(2.0 * i for i in range(copies)))


class Case:
    """A context whose n2 reaches a tail, its pencil and its shape property."""

    def __init__(self, name, device, geometry):
        import torch
        from pl_fem_vectoriel_amd import _native
        from pl_fem_vectoriel_amd.mesh import generate_mesh
        from pl_fem_vectoriel_amd.solver_fem import _core_table
        self.torch, self.name = torch, name
        if name == "c1":
            mesh = generate_mesh(geometry, 1.0, 1)
            self.sym = _native.Symbolic(mesh.p, mesh.t)
            self.ctx = _native.Context(self.sym, device, max_ncv=65)
            self.ctx.assemble(_core_table(geometry), geometry.n_core ** 2, geometry.n_clad ** 2, geometry.k0, 1.0)
            self.cores = _core_table(geometry)
        else:
            n, dpn, max_ncv, copies = SQUARES[name]
            p, t, self.cores = square_mesh(n, copies)
            self.sym = _native.Symbolic(p, t, dofs_per_node=dpn, dirichlet=dpn == 2)
            self.ctx = _native.Context(self.sym, device, max_ncv=max_ncv)
            if dpn == 2:
                self.ctx.assemble(self.cores, N_CORE ** 2, N_CLAD ** 2, K0, 1.0)
            else:
                self.ctx.assemble_scalar(self.cores, N_CORE ** 2, N_CLAD ** 2, K0)
        self.N, self.dpn, self.n2 = self.sym.N, self.sym.dofs_per_node, self.ctx.n2
        self.pencil = le.Pencil(self.sym, self.ctx)
        self.front = le.FrontOrder(self.sym)
        self.ncols = (NCOLS if name in ("sca16", "vec16") else NCOLS_LARGE) + (self.ctx.max_ncv + P,)
        self.rng = np.random.default_rng(ALL_CASES.index(name) + 11)
        self.assert_shape()

    def assert_shape(self):
        n2, tail = self.n2, self.n2 % le.PANEL_CHUNK
        bm = self.sym.array("bmask")
        if self.name in ("sca16", "sca16m65"):
            assert n2 == 1089 and tail == 65 and 64 < tail < 128 and not bm.any()
        elif self.name == "vec16":
            assert n2 == 2178 and tail == 130 and bm.any()
        elif self.name == "sca255":
            assert n2 == 261121 == 255 * 1024 + 1 and tail == 1
            assert -(-n2 // le.PANEL_CHUNK) > 56 and -(-self.N * 8 // 256) > 448     # both unrolled loops run
        elif self.name == "sca16x3":
            assert n2 == 3 * 1089 and n2 % 2 == 1 and not bm.any()
        elif self.name == "vec16x3":
            assert n2 == 3 * 2178 == 6534 and bm.any()
        else:
            assert n2 == 181278 and tail == 30 and -(-self.N * 8 // 256) == 2833 and bm.any()

    # -- device buffers
    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).cuda(self.ctx.device)

    @staticmethod
    def host(t):
        return t.cpu().numpy().astype(np.float64)

    def block(self, X, ld):
        """(n2, q) -> flat columns ld apart, gaps NaN."""
        n, q = X.shape
        buf = np.full((q, ld), np.nan)
        buf[:, :n] = X.T
        return self.dev(buf)

    def unblock(self, t, q, ld):
        """flat columns ld apart -> (n2, q); asserts the gaps are still NaN."""
        buf = self.host(t).reshape(q, ld)
        assert np.isnan(buf[:, self.n2:]).all(), "a gap between the columns was written"
        return buf[:, :self.n2].T.copy()

    def random(self, *shape, live=False):
        """O(1) random data (every row matters); live = Dirichlet rows zero, as in a Lanczos vector."""
        X = self.rng.uniform(0.5, 1.5, shape) * self.rng.choice((-1.0, 1.0), shape)
        if live:
            X[~self.live_rows()] = 0.0
        return X

    def live_rows(self):
        bm = self.sym.array("bmask").astype(bool)
        return ~np.tile(bm, self.dpn)

    # -- what the driver tests compute once per context and share (never modified)
    @functools.cached_property
    def sigma(self):
        return sigma_of(self.dpn)

    @functools.cached_property
    def op(self):
        """OP through SuperLU on the pencil read from the context."""
        return le.ShiftInvert(self.pencil.matrix("A"), self.pencil.matrix("B"), self.sigma, self.live_rows())

    @functools.cached_property
    def dense(self):
        """(lam, X, components) of le.dense_reference on the pencil read from the context."""
        return le.dense_reference(self.pencil.matrix("A"), self.pencil.matrix("B"), self.live_rows(), self.sigma)


@pytest.fixture(scope="module")
def cases(c1_geometry, gpu_device, built_library):
    @functools.lru_cache(maxsize=None)
    def get(name):
        return Case(name, gpu_device, c1_geometry)
    return get


# ---- the host side: the oracle's pencils of the same meshes -----------------------------------------------------------
class SquareGeometry:
    """Geometry duck type of the oracle's assemblies: closed discs of eps = n_core^2 on n_clad^2 (MCFGeometry.epsilon
    without the PML factor)."""
    k0, n_core, n_clad = K0, N_CORE, N_CLAD

    def __init__(self, cores):
        cores = np.asarray(cores, dtype=np.float64).reshape(-1, 3)
        self.positions = self.core_positions = cores[:, :2]
        self.core_radii = cores[:, 2]

    def epsilon(self, x, y):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        eps = np.full(x.shape, self.n_clad ** 2, dtype=complex)
        for (cx, cy), r in zip(self.positions, self.core_radii):
            eps[(x - cx) ** 2 + (y - cy) ** 2 <= r ** 2] = self.n_core ** 2
        return eps


class HostCase:
    """The oracle's pencil of a square case on full-length vectors (Dirichlet rows and columns dropped from the operator),
    its analysis (no device) and the drivers' start block."""

    def __init__(self, name):
        from oracle import hfield, scalar
        from oracle.p2 import MeshTriLite
        from pl_fem_vectoriel_amd import _native
        n, dpn, _, copies = SQUARES[name]
        p, t, cores = square_mesh(n, copies)
        self.name, self.dpn, self.cores = name, dpn, cores
        self.sym = _native.Symbolic(p, t, dofs_per_node=dpn, dirichlet=dpn == 2)
        g, om = SquareGeometry(cores), MeshTriLite(p, t)
        if dpn == 2:
            self.A, self.B, basis = hfield.assemble_hfield_system_fused(g, om, eliminate_zeros=False)[:3]
            interior = np.setdiff1d(np.arange(basis.N), basis.get_dofs().all())
            self.live = np.zeros(2 * basis.N, dtype=bool)
            self.live[np.concatenate([interior, interior + basis.N])] = True
        else:
            K, M, Me, basis = scalar.assemble(g, om, eliminate_zeros=False)
            self.A, self.B = (K - K0 ** 2 * Me).tocsr(), M.tocsr()
            self.live = np.ones(basis.N, dtype=bool)
        assert basis.N == self.sym.N
        self.n2 = dpn * basis.N
        self.sigma = sigma_of(dpn)
        self.op = le.ShiftInvert(self.A, self.B, self.sigma, self.live)
        self.start = le.start_field(self.sym, P)

    @functools.cached_property
    def dense(self):
        return le.dense_reference(self.A, self.B, self.live, self.sigma)

    def start_block(self, nvec, seed=None):
        """The drivers' own start block (seed None) or a random interior one."""
        if seed is None:
            return self.start[:, :nvec]
        X = np.random.default_rng(seed).uniform(-1, 1, (self.n2, nvec))
        X[~self.live] = 0.0
        return X


@functools.lru_cache(maxsize=None)
def host_case(name):
    return HostCase(name)
