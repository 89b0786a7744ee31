"""The static-pivot replacement of the block LDL^T on the GPU (kernels_front.hip, pair_step / ldl_pivot_block) against the
front emulation that states the same rule (front_emulation.ldl_partial), on element matrices written so that chosen
pairs of chosen fronts meet their elimination step with a chosen 2 x 2 block (pivot_cases.py; the host half is
test_pivot_replacement_host.py).  Per case: the count, D^-1 of every planted pair against its closed form, every front
and Schur complement against the extended-precision emulation, the solves (P = 1, P = 4, with and without a refinement
pass) against SuperLU of the planted matrix, and the same bits from a second factorisation."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import front_emulation as fe
import pivot_cases as pc
from front_checks import BERR_FLOOR, FACTOR_RATIO, FWD_TOL, backward_error, front_check, right_hand_sides
from pl_fem_vectoriel_amd import _native
from pl_fem_vectoriel_amd.solver_fem import _core_table

pytestmark = pytest.mark.gpu
SOLVE_IDS = [cid for cid in pc.CASE_IDS if pc.find(cid)[1].solves]


class Planted:
    """One tree on the device: the context, and the case whose element matrices it currently holds."""

    def __init__(self, data, device):
        import torch
        self.torch, self.data = torch, data
        g = data.g
        self.ctx = _native.Context(data.sym, device, max_ncv=65)
        if data.dpn == 2:
            self.ctx.assemble(_core_table(g), g.n_core ** 2, g.n_clad ** 2, g.k0, 1.0)
        else:
            self.ctx.assemble_scalar(_core_table(g), g.n_core ** 2, g.n_clad ** 2, g.k0)
        self.rhs = right_hand_sides(data.T, data.idx, data.N)
        self.holds = None

    def factor(self, ref):
        """The case's element matrices written (once per case) and factored at sigma = 0; returns the count."""
        if self.holds != ref.case.name:
            self.ctx.debug_set_elements(self.data.device_elements(ref.Ke))
            self.holds = ref.case.name
        self.ctx.factor(0.0)
        return self.ctx.timings()["pivot_perturbations"]

    def delta(self, f):
        T = self.data.T
        s2 = T.s2(f)
        return self.ctx.debug_copy("delta", 2 * 2 * T.fptr[f], 2 * s2).reshape(s2, 2)    # D^-1: (diagonal, off-diagonal) per row

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda(self.ctx.device)


@pytest.fixture(scope="module")
def planted(c1_geometry, gpu_device, built_library):
    made = {}

    def get(case_id):
        tree, _ = pc.find(case_id)
        if tree.name not in made:
            made[tree.name] = Planted(pc.tree_data(tree.name, c1_geometry), gpu_device)
        return made[tree.name], pc.reference(case_id, c1_geometry)
    return get


@pytest.mark.parametrize("case_id", pc.CASE_IDS)
def test_count_and_planted_pairs(planted, case_id):
    """pivot_perturbations is the emulation's count exactly (0 for the unplanted write and the controls), a second
    factorisation neither adds to it nor changes a bit of D^-1 or of the fronts; D^-1 of every decoupled plant is its closed
    form to DELTA_TOL (an exact zero off the diagonal of scalar pivots), its pivot kind the planned one."""
    dev, ref = planted(case_id)
    T = dev.data.T
    count = dev.factor(ref)
    deltas = {f: dev.delta(f) for f in range(T.nf) if T.s2(f)}
    fronts = dev.ctx.debug_copy("front", 0, int(dev.data.sym.info["front_doubles"]))
    for p, f, k, rows in ref.plant_rows():
        print(f"\n{case_id} front {f} pair {k // 2} {p.kind}{'+' if p.sign > 0 else '-'}: D^-1 {deltas[f][k:k + 2].tolist()} "
              f"error {pc.delta_error(deltas[f][k:k + 2], rows):.2e}")
    print(f"\n{case_id}: pivot_perturbations {count} (emulation {ref.count})")
    assert count == ref.count
    assert pc.device_findings(ref, count, deltas.__getitem__) == []
    assert dev.factor(ref) == ref.count                  # reset, not accumulated
    for f, d in deltas.items():
        assert np.array_equal(dev.delta(f), d), f
    assert np.array_equal(dev.ctx.debug_copy("front", 0, fronts.size), fronts)


@pytest.mark.parametrize("case_id", pc.CASE_IDS)
def test_every_front_matches_the_emulation(planted, case_id):
    """F11 / Z / Z^T and D^-1 of every front, the pivot kind of every pair, and the Schur complements level by level, under
    the rule of test_gpu_operator_forms.py.  (Measured on the MI355X: the coupled case (i), multipliers of 1e8, is 1.0 - 2.7
    times as far from the extended-precision emulation as the float64 emulation is, errors up to 4.5e-8 of a block's
    largest entry; no case needs a ratio of its own.)"""
    dev, ref = planted(case_id)
    T, ctx = dev.data.T, dev.ctx
    assert dev.factor(ref) == ref.count
    worst = {}

    def check(got, dbl, xp, what):
        err, emu = front_check(got, dbl, xp, what)
        key = what[-1]
        if err > worst.get(key, (0.0, 0.0))[0]:
            worst[key] = (err, emu)

    for f in range(T.nf):
        s2 = T.s2(f)
        Fg, Fe, Fx = T.device_front(ctx, f), ref.Fs[f], ref.Fx[f]
        check(Fg[:s2, :s2], Fe[:s2, :s2], Fx[:s2, :s2], (f, "F11"))
        check(Fg[s2:, :s2], Fe[s2:, :s2], Fx[s2:, :s2], (f, "Z"))
        check(Fg[:s2, s2:], Fe[:s2, s2:], Fx[:s2, s2:], (f, "ZT"))
        if s2:
            dg = dev.delta(f)
            check(dg, ref.Ds[f], ref.Dx[f], (f, "Dinv"))
            gpu_2x2 = dg[0::2, 1] != 0.0                # a 2 x 2 pivot keeps its off-diagonal entry of D^-1
            for q, (xp_2x2, margin) in enumerate(ref.kinds[f]):
                if gpu_2x2[q] != xp_2x2:                # only where the kind test is a tie to rounding
                    assert margin < 1e-12, (f, q, margin)
    # Schur complements (lower triangle): the factorisation stopped after each level, every front of that level
    for lev in range(T.L, 0, -1):
        ctx.debug_factor_until(0.0, lev, 0, 5)
        for f in range((1 << lev) - 1, min(T.nf, (1 << (lev + 1)) - 1)):
            s2 = T.s2(f)
            if T.m(f) > s2:
                Sg = np.tril(T.device_front(ctx, f, with_schur=True)[s2:, s2:])
                check(Sg, np.tril(ref.Fs[f][s2:, s2:]), np.tril(ref.Fx[f][s2:, s2:]), (lev, f, "S"))
    ctx.factor(0.0)
    print(f"\n{case_id}: " + ", ".join(f"{k} {e:.1e} (emulation {r:.1e}, ratio {e / max(r, 1e-300):.1f})" for k, (e, r) in worst.items()))


def _emulated(data, ref, K, b, passes):
    x = fe.solve(data.T, ref.Fs, ref.Ds, b)
    for _ in range(passes):
        r = np.zeros_like(b)
        r[data.idx] = b[data.idx] - K @ x[data.idx]
        x = x + fe.solve(data.T, ref.Fs, ref.Ds, r)
    return x


@pytest.mark.parametrize("case_id", SOLVE_IDS)
def test_solves_with_replaced_pivots(planted, case_id):
    """plfem_solve and the block sweeps (P = 4) with 0 and 1 refinement passes, on the four right-hand sides of the operator
    tests, against the planted K: backward error within 10 times the emulation's at the same number of passes (or
    BERR_FLOOR), forward error after one pass within FACTOR_RATIO times the emulation's (or FWD_TOL), finite values, zero
    Dirichlet rows, P = 4 equal to P = 1 as in test_block_solve."""
    dev, ref = planted(case_id)
    data, ctx, torch = dev.data, dev.ctx, dev.torch
    assert dev.factor(ref) == ref.count
    K = data.matrix(ref.Ke)
    lu = spla.splu(K.tocsc())
    idx, n2, P = data.idx, data.dpn * data.N, fe.BLOCK_P
    keys = ("random", "leaf", "root", "random2")
    cols = [dev.rhs[k] for k in keys]
    xs = [lu.solve(b[idx]) for b in cols]

    def fwd(x, u):
        return float(np.linalg.norm(x[idx] - xs[u]) / np.linalg.norm(xs[u]))

    emul = {n: [_emulated(data, ref, K, b, n) for b in cols] for n in (0, 1)}
    emul_berr = {n: max(backward_error(K, x[idx], b[idx]) for x, b in zip(emul[n], cols)) for n in (0, 1)}
    emul_fwd = {n: max(fwd(x, u) for u, x in enumerate(emul[n])) for n in (0, 1)}
    bd = dev.dev(np.concatenate(cols))
    got_berr, got_fwd = {0: 0.0, 1: 0.0}, {0: 0.0, 1: 0.0}
    for n in (0, 1):
        xd = torch.zeros(P * n2, dtype=torch.float64, device=bd.device)
        ctx.debug_solve_block(bd, xd, n2, refine_steps=n)
        X4 = xd.cpu().numpy().reshape(P, n2)
        for u, b in enumerate(cols):
            x1 = ctx.solve(dev.dev(b), n).cpu().numpy()
            for what, x in (("P=1", x1), ("P=4", X4[u])):
                assert np.isfinite(x).all(), (what, n, keys[u])
                rest = np.delete(x, idx)
                assert rest.size == 0 or np.abs(rest).max() == 0.0, (what, n, keys[u])
                got_berr[n] = max(got_berr[n], backward_error(K, x[idx], b[idx]))
                got_fwd[n] = max(got_fwd[n], fwd(x, u))
            assert np.linalg.norm(X4[u] - x1) / np.linalg.norm(x1) < FWD_TOL, (n, keys[u])     # agrees with the P = 1 sweeps
    print(f"\n{case_id}: backward error {got_berr[0]:.2e} / {got_berr[1]:.2e} after 0 / 1 passes (emulation {emul_berr[0]:.2e} / "
          f"{emul_berr[1]:.2e}), forward error {got_fwd[0]:.2e} / {got_fwd[1]:.2e} (emulation {emul_fwd[0]:.2e} / {emul_fwd[1]:.2e})")
    for n in (0, 1):
        assert got_berr[n] <= max(10.0 * emul_berr[n], BERR_FLOOR), (n, got_berr[n], emul_berr[n])
    assert got_fwd[1] <= max(FACTOR_RATIO * emul_fwd[1], FWD_TOL), (got_fwd[1], emul_fwd[1])
