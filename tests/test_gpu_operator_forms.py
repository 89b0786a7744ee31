"""Every launch form of the multifrontal factor and solve sweeps on the GPU, at P = 1 (plfem_solve) and P = 4 (the block
sweeps of the block Lanczos driver, plfem_debug_solve_block), for both pencils, against a high-precision reference:
the NumPy emulation of the same front tree (front_emulation.py) and SuperLU.  The cases (operator_cases.py) are chosen
so that together they launch every kernel form the plan rules can pick; the plan hook proves which ones each ran."""
import functools

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import front_emulation as fe
import operator_cases as oc
from front_checks import BERR_FLOOR, FACTOR_RATIO, FACTOR_TOL, FWD_TOL, backward_error  # noqa: F401
from front_checks import front_check as _front_check, owned_dofs, right_hand_sides
from oracle import hfield, scalar
from oracle.p2 import MeshTriLite, P2Basis
from pl_fem_vectoriel_amd import _native
from pl_fem_vectoriel_amd.solver_fem import _core_table, shift_estimate

pytestmark = pytest.mark.gpu


class Operator:
    """One case: mesh, analysis, assembled and factored context, the pencil K on the unknowns, SuperLU, right-hand sides."""

    def __init__(self, case, g, device, emulate=True):
        import torch
        self.torch, self.case, self.g = torch, case, g
        mesh = oc.mesh_of(case, g)
        self.sym = oc.symbolic_of(case, mesh)
        self.ctx = _native.Context(self.sym, device, max_ncv=65)
        self.N, self.dpn = self.sym.N, case.dpn
        self.n2 = self.dpn * self.N
        om = MeshTriLite(mesh.p, mesh.t)
        if self.dpn == 2:
            self.ctx.assemble(_core_table(g), g.n_core ** 2, g.n_clad ** 2, g.k0, 1.0)
            self.sigma = shift_estimate(g)
            A, B, _, _, _, _, _ = hfield.assemble_hfield_system_fused(g, om, eliminate_zeros=False)
            basis = P2Basis(om)
            A_int, B_int, interior = hfield.restrict_interior(A, B, basis)
            self.idx = np.concatenate([interior, interior + self.N])
            self.K = (A_int - self.sigma * B_int).tocsr()
            Ke = fe.element_K(hfield.element_matrices(g, basis), g.k0 ** 2, self.sigma) if emulate else None
        else:
            self.ctx.assemble_scalar(_core_table(g), g.n_core ** 2, g.n_clad ** 2, g.k0)
            self.sigma = scalar.shift(g)
            K, M, Me, basis = scalar.assemble(g, om, eliminate_zeros=False)
            self.idx = np.arange(self.N)
            self.K = (K - g.k0 ** 2 * Me - self.sigma * M).tocsr()
            Ke = fe.element_K_scalar(scalar.element_matrices(g, basis), g.k0 ** 2, self.sigma) if emulate else None
        self.lu = spla.splu(self.K.tocsc())
        self.T = fe.FrontTree(self.sym)
        self.forms = fe.level_forms(self.sym)
        self.rhs = self._right_hand_sides()
        if emulate:
            self.Fs, self.Ds = fe.factor(self.T, Ke)
            # the emulation's backward error over the case's right-hand sides: the yardstick of the GPU's
            self.emul_berr = max(backward_error(self.K, fe.solve(self.T, self.Fs, self.Ds, b)[self.idx], b[self.idx])
                                 for b in self.rhs.values())
            if not case.factor:             # (the fronts of the large-leaf cases take gigabytes)
                del self.Fs, self.Ds
            else:                           # the reference of the front-by-front checks: extended precision
                self.kinds = {}
                self.Fx, self.Dx = fe.factor(self.T, Ke.astype(np.longdouble), self.kinds)

    def _owned_dofs(self, f):
        """Global DOFs owned by front f (component-major vectors of length dpn N)."""
        return owned_dofs(self.T, f, self.N)

    def _right_hand_sides(self):
        return right_hand_sides(self.T, self.idx, self.N)

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda(self.ctx.device)

    def check_column(self, x, b, bound, what):
        """x: a GPU solution of b (full length).  Backward error within the bound, forward error against SuperLU,
        Dirichlet rows exactly zero.  Returns the backward error."""
        assert np.isfinite(x).all(), what
        berr = backward_error(self.K, x[self.idx], b[self.idx])
        assert berr <= bound, (what, berr, bound)
        xs = self.lu.solve(b[self.idx])
        assert np.linalg.norm(x[self.idx] - xs) / np.linalg.norm(xs) < FWD_TOL, what
        rest = np.delete(x, self.idx)
        assert rest.size == 0 or np.abs(rest).max() == 0.0, what
        return berr


@pytest.fixture(scope="module")
def operators(c1_geometry, gpu_device, built_library):
    @functools.lru_cache(maxsize=None)
    def get(name):
        case = next(c for c in oc.CASES + (oc.FULL_SIZE,) if c.name == name)
        return Operator(case, c1_geometry, gpu_device, emulate=case is not oc.FULL_SIZE)
    return get


CASE_IDS = [c.name for c in oc.CASES]
FACTOR_IDS = [c.name for c in oc.CASES if c.factor]


@pytest.mark.parametrize("name", CASE_IDS)
def test_device_plan_is_the_rules(operators, name):
    """The plan the context launches from = level_forms: the coverage claimed on the host is what runs."""
    op = operators(name)
    got = op.ctx.debug_level_plan()
    assert len(got) == len(op.forms)
    for lev, (g, r) in enumerate(zip(got, op.forms)):
        assert g == {k: r[k] for k in _native.PLAN_FIELDS}, (lev, g, r)
    print(f"\n{name}: " + "; ".join(f"L{lev} {r['count']} {r['fwd']} / {r['bwd']}" for lev, r in enumerate(op.forms)))


@pytest.mark.parametrize("name", CASE_IDS)
def test_single_vector_solve(operators, name):
    op = operators(name)
    op.ctx.factor(op.sigma)
    assert op.ctx.timings()["pivot_perturbations"] == 0
    bound = max(10.0 * op.emul_berr, BERR_FLOOR)
    worst = 0.0
    for key, b in op.rhs.items():
        bd = op.dev(b)
        x = op.ctx.solve(bd, 0).cpu().numpy()
        worst = max(worst, op.check_column(x, b, bound, key))
        assert np.array_equal(bd.cpu().numpy(), b), key                        # the right-hand side is not written
        assert np.array_equal(op.ctx.solve(bd, 0).cpu().numpy(), x), key       # the same bits every run
    assert not op.ctx.solve(op.dev(np.zeros(op.n2)), 0).cpu().numpy().any()
    if op.dpn == 2:            # huge values on the Dirichlet entries never enter the solve
        b = op.rhs["random"]
        bh = b.copy()
        bh[np.setdiff1d(np.arange(op.n2), op.idx)] = 1e300
        assert np.array_equal(op.ctx.solve(op.dev(bh), 0).cpu().numpy(), op.ctx.solve(op.dev(b), 0).cpu().numpy())
    print(f"\n{name} P=1: backward error {worst:.2e} (emulation {op.emul_berr:.2e})")


@pytest.mark.parametrize("name", CASE_IDS)
def test_block_solve(operators, name):
    op = operators(name)
    op.ctx.factor(op.sigma)
    assert all(r["max_block_p"] == fe.BLOCK_P for r in op.ctx.debug_level_plan())
    P, n2 = fe.BLOCK_P, op.n2
    bound = max(10.0 * op.emul_berr, BERR_FLOOR)
    cols = [op.rhs[k] for k in ("random", "leaf", "root", "random2")]       # four different right-hand sides
    Bm = np.concatenate(cols)
    bd = op.dev(Bm)
    xd = op.torch.zeros(P * n2, dtype=op.torch.float64, device=bd.device)
    op.ctx.debug_solve_block(bd, xd, n2)
    X = xd.cpu().numpy().reshape(P, n2)
    assert np.array_equal(bd.cpu().numpy(), Bm)
    worst = 0.0
    for u in range(P):
        worst = max(worst, op.check_column(X[u], cols[u], bound, u))
        x1 = op.ctx.solve(op.dev(cols[u]), 0).cpu().numpy()
        assert np.linalg.norm(X[u] - x1) / np.linalg.norm(x1) < FWD_TOL, u          # agrees with the P = 1 sweeps
    xd2 = op.torch.full((P * n2,), np.nan, dtype=op.torch.float64, device=bd.device)
    op.ctx.debug_solve_block(bd, xd2, n2)
    assert np.array_equal(xd2.cpu().numpy(), X.ravel())                         # deterministic; every entry written
    # columns ldx > n2 apart: NaN in the gaps of the input, NaN pre-filled in the gaps of the output
    ldx = n2 + 37
    Bg = np.full((P, ldx), np.nan)
    Bg[:, :n2] = Bm.reshape(P, n2)
    bg = op.dev(Bg.ravel())
    xg = op.torch.full((P * ldx,), np.nan, dtype=op.torch.float64, device=bd.device)
    op.ctx.debug_solve_block(bg, xg, ldx)
    Xg = xg.cpu().numpy().reshape(P, ldx)
    assert np.isnan(Xg[:, n2:]).all()
    assert np.array_equal(Xg[:, :n2], X)
    # one pass of block refinement (the block SpMVs of the refined Lanczos operator) keeps the solution as good
    xr = op.torch.zeros(P * ldx, dtype=op.torch.float64, device=bd.device)
    op.ctx.debug_solve_block(bg, xr, ldx, refine_steps=1)
    Xr = xr.cpu().numpy().reshape(P, ldx)
    for u in range(P):
        op.check_column(Xr[u, :n2], cols[u], bound, ("refined", u))
    # zero block -> exactly zero
    z = op.torch.zeros(P * n2, dtype=op.torch.float64, device=bd.device)
    xz = op.torch.full((P * n2,), np.nan, dtype=op.torch.float64, device=bd.device)
    op.ctx.debug_solve_block(z, xz, n2)
    assert not xz.cpu().numpy().any()
    with pytest.raises(ValueError):
        op.ctx.debug_solve_block(bd, xd, n2 - 1)
    print(f"\n{name} P=4: backward error {worst:.2e} (emulation {op.emul_berr:.2e})")


@pytest.mark.parametrize("name", FACTOR_IDS)
def test_every_front_matches_the_emulation(operators, name):
    """F11 / Z / Z^T and D^-1 of every front, the pivot kind of every pair, and the Schur complements level by level."""
    op = operators(name)
    T, ctx = op.T, op.ctx
    ctx.factor(op.sigma)
    assert ctx.timings()["pivot_perturbations"] == 0
    seen = []                                       # (error, the emulation's error) of every block checked
    for f in range(T.nf):
        s2 = T.s2(f)
        Fg, Fe, Fx = T.device_front(ctx, f), op.Fs[f], op.Fx[f]
        seen.append(_front_check(Fg[:s2, :s2], Fe[:s2, :s2], Fx[:s2, :s2], (f, "F11")))
        seen.append(_front_check(Fg[s2:, :s2], Fe[s2:, :s2], Fx[s2:, :s2], (f, "Z")))
        seen.append(_front_check(Fg[:s2, s2:], Fe[:s2, s2:], Fx[:s2, s2:], (f, "ZT")))
        if s2:
            dg = ctx.debug_copy("delta", 2 * 2 * T.fptr[f], 2 * s2).reshape(s2, 2)     # D^-1: (diagonal, off-diagonal) per row
            seen.append(_front_check(dg, op.Ds[f], op.Dx[f], (f, "Dinv")))
            gpu_2x2 = dg[0::2, 1] != 0.0                # a 2 x 2 pivot keeps its off-diagonal entry of D^-1
            for q, (xp_2x2, margin) in enumerate(op.kinds[f]):
                if gpu_2x2[q] != xp_2x2:                # only where the kind test is a tie to rounding
                    assert margin < 1e-12, (f, q, margin)
    # Schur complements (lower triangle): the factorisation stopped after each level, every front of that level
    for lev in range(T.L, 0, -1):
        ctx.debug_factor_until(op.sigma, lev, 0, 5)
        for f in range((1 << lev) - 1, min(T.nf, (1 << (lev + 1)) - 1)):
            s2 = T.s2(f)
            if T.m(f) > s2:
                Sg = np.tril(T.device_front(ctx, f, with_schur=True)[s2:, s2:])
                seen.append(_front_check(Sg, np.tril(op.Fs[f][s2:, s2:]), np.tril(op.Fx[f][s2:, s2:]), (lev, f, "S")))
    ctx.factor(op.sigma)
    print(f"\n{name}: {len(seen)} blocks of {T.nf} fronts, worst error {max(e for e, _ in seen):.2e} "
          f"(emulation {max(r for _, r in seen):.2e})")


def test_both_pivot_kinds_occur(operators):
    n = {False: 0, True: 0}
    for name in FACTOR_IDS:
        op = operators(name)
        op.ctx.factor(op.sigma)
        for f in range(op.T.nf):
            s2 = op.T.s2(f)
            if s2:
                dg = op.ctx.debug_copy("delta", 2 * 2 * op.T.fptr[f], 2 * s2).reshape(s2, 2)
                k = dg[0::2, 1] != 0.0
                n[True] += int(k.sum())
                n[False] += int((~k).sum())
    assert n[True] > 0 and n[False] > 0, n


def test_block_solve_refuses_what_the_context_rules_out(c1_geometry, gpu_device, built_library):
    import torch
    from pl_fem_vectoriel_amd.mesh import unit_square_mesh
    case = oc.Case("x", ("square", 12), 10 ** 6, 2, False, "")
    sym = oc.symbolic_of(case, unit_square_mesh(12))
    ctx = _native.Context(sym, gpu_device, max_ncv=65)
    b = torch.zeros(4 * ctx.n2, dtype=torch.float64, device=ctx.tdev)
    x = torch.zeros_like(b)
    with pytest.raises(RuntimeError):          # PLFEM_ESTATE before plfem_factor
        ctx.debug_solve_block(b, x, ctx.n2)
    ctx.close()
    # a tree whose largest front is beyond the P = 4 LDS budget: the hook launches no P = 4 sweep
    big = oc.Case("y", ("square", 30), 10 ** 6, 2, False, "")
    sym = oc.symbolic_of(big, unit_square_mesh(30))
    assert fe.level_forms(sym)[0]["max_block_p"] == 1
    ctx = _native.Context(sym, gpu_device, max_ncv=65)
    ctx.assemble(_core_table(c1_geometry), c1_geometry.n_core ** 2, c1_geometry.n_clad ** 2, c1_geometry.k0, 1.0)
    ctx.factor(shift_estimate(c1_geometry))
    assert ctx.debug_level_plan()[0]["max_block_p"] == 1
    b = torch.zeros(4 * ctx.n2, dtype=torch.float64, device=ctx.tdev)
    with pytest.raises(ValueError):
        ctx.debug_solve_block(b, torch.zeros_like(b), ctx.n2)
    ctx.close()


def test_full_size_solves_match_splu(operators):
    """C1 at full size (N = 90 639), P = 1 and P = 4, against SuperLU."""
    op = operators(oc.FULL_SIZE.name)
    assert op.N == 90639
    op.ctx.factor(op.sigma)
    assert op.ctx.timings()["pivot_perturbations"] == 0
    cols = [op.rhs[k] for k in ("random", "leaf", "root", "random2")]
    X1 = [op.ctx.solve(op.dev(b), 0).cpu().numpy() for b in cols]
    b1 = [op.check_column(x, b, 1e-10, k) for x, b, k in zip(X1, cols, range(4))]
    bd = op.dev(np.concatenate(cols))
    xd = op.torch.zeros(4 * op.n2, dtype=op.torch.float64, device=bd.device)
    op.ctx.debug_solve_block(bd, xd, op.n2)
    X = xd.cpu().numpy().reshape(4, op.n2)
    b4 = [op.check_column(X[u], cols[u], 1e-10, u) for u in range(4)]
    for u in range(4):
        assert np.linalg.norm(X[u] - X1[u]) / np.linalg.norm(X1[u]) < FWD_TOL
    print(f"\nfull size: backward error P=1 {max(b1):.2e}, P=4 {max(b4):.2e}")
