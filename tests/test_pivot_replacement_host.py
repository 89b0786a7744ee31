"""Host checks of the static-pivot replacement rule as front_emulation.ldl_partial restates it (kernels_front.hip,
pair_step / ldl_pivot_block) and of the planted cases of pivot_cases.py: every case replaces exactly the planned pivots,
in float64 and in extended precision alike -- the condition under which comparing the GPU with the emulation means
something --, the rule changes no bit of a factorisation in which nothing vanishes, one refinement pass repairs the
coupled replacement, and each of five plausible mistakes in the rule would fail the GPU tests by a wide margin."""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse.linalg as spla

import front_emulation as fe
import operator_cases as oc
import pivot_cases as pc
from front_checks import right_hand_sides

NB = fe.NB


def _ldl_partial_without_rule(Fm, s2):
    """front_emulation.ldl_partial as it was before it knew the replacement rule (kept verbatim, for the bit comparison)."""
    F = Fm.copy()
    Dinv = np.zeros((s2, 2), dtype=F.dtype)
    for k0 in range(0, s2, NB):
        k1 = min(k0 + NB, s2)
        Cp = np.zeros((F.shape[0] - k1, k1 - k0), dtype=F.dtype)
        for k in range(k0, k1, 2):
            a, b, c = F[k, k], F[k + 1, k], F[k + 1, k + 1]
            det = a * c - b * b
            s = max(abs(a), abs(b), abs(c))
            lhs, rhs = b * b * abs(det), a * a * s * s
            if lhs <= rhs:
                for j in (k, k + 1):
                    d = F[j, j]
                    col = F[j + 1:, j].copy()
                    l = col / d
                    F[j + 1:, j + 1:k1] -= np.outer(l, col[:k1 - j - 1])
                    F[j + 1:, j] = l
                    Cp[:, j - k0] = col[k1 - j - 1:]
                    Dinv[j] = (1.0 / d, 0.0)
            else:
                e11, e12, e22 = c / det, -b / det, a / det
                Dinv[k] = (e11, e12)
                Dinv[k + 1] = (e22, e12)
                C = F[k + 2:, k:k + 2].copy()
                Lc = np.stack([C[:, 0] * e11 + C[:, 1] * e12, C[:, 0] * e12 + C[:, 1] * e22], 1)
                F[k + 2:, k + 2:k1] -= Lc @ C[:k1 - k - 2].T
                F[k + 2:, k:k + 2] = Lc
                F[k + 1, k] = 0.0
                Cp[:, k - k0:k - k0 + 2] = C[k1 - k - 2:]
        F[k1:, k1:] -= F[k1:, k0:k1] @ Cp.T
    L11 = np.tril(F[:s2, :s2], -1) + np.eye(s2)
    if F.dtype == np.float64:
        X = sla.solve_triangular(L11, np.eye(s2), lower=True, unit_diagonal=True) if s2 else np.zeros((0, 0))
    else:
        X = np.eye(s2, dtype=F.dtype)
        for j in range(s2 - 1):
            X[j + 1:, :j + 1] -= np.outer(L11[j + 1:, j], X[j, :j + 1])
    out = F.copy()
    out[:s2, :s2] = np.tril(X) + np.tril(X, -1).T
    Z = F[s2:, :s2] @ np.tril(X)
    out[s2:, :s2] = Z
    out[:s2, s2:] = Z.T
    return out, Dinv


def _same_bits(x, y):
    """(an extended-precision number has padding bytes: values and signs of zero instead of the raw bytes)"""
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) and np.array_equal(np.signbit(x), np.signbit(y))


# the FACTOR cases of operator_cases.py on the meshes the host tests emulate anyway (C1 at refinement 0.5, the one-front square)
BIT_CASES = ("c1_h05_l24_vec", "c1_h05_l24_sca", "c1_h05_l8_sca", "sq12_one_vec", "sq12_one_sca")


@pytest.mark.parametrize("name", BIT_CASES)
def test_the_rule_changes_no_bit_where_nothing_vanishes(built_library, c1_geometry, name):
    from oracle import hfield, scalar
    from oracle.p2 import MeshTriLite, P2Basis
    from pl_fem_vectoriel_amd.solver_fem import shift_estimate
    g = c1_geometry
    case = next(c for c in oc.CASES if c.name == name)
    assert case.factor
    mesh = oc.mesh_of(case, g)
    sym = oc.symbolic_of(case, mesh)
    basis = P2Basis(MeshTriLite(mesh.p, mesh.t))
    if case.dpn == 2:
        Ke = fe.element_K(hfield.element_matrices(g, basis), g.k0 ** 2, shift_estimate(g))
    else:
        Ke = fe.element_K_scalar(scalar.element_matrices(g, basis), g.k0 ** 2, scalar.shift(g))
    T = fe.FrontTree(sym)
    for K in (Ke, Ke.astype(np.longdouble)) if name == "sq12_one_sca" else (Ke,):      # (extended precision where it is cheap)
        S = [None] * T.nf
        npairs = 0
        for f in range(T.nf - 1, -1, -1):
            s2 = T.s2(f)
            Fm = fe.assemble_front(T, f, K, S)
            log = []
            F1, D1 = fe.ldl_partial(Fm, s2, None, log)
            F0, D0 = _ldl_partial_without_rule(Fm, s2)
            S[f] = F1[s2:, s2:]
            assert not log, f
            assert _same_bits(F0, F1) and _same_bits(D0, D1), f
            npairs += s2 // 2
        assert npairs > 100
    sym.close()


@pytest.mark.parametrize("case_id", pc.CASE_IDS)
def test_every_case_replaces_exactly_what_it_plans(built_library, c1_geometry, case_id):
    """The same pairs, sites and signs in float64 and in extended precision, nothing unplanned; the largest row entry
    the rule saw; the planted values themselves; and the extended-precision D^-1 of every decoupled plant is the closed
    form of the rule."""
    ref = pc.reference(case_id, c1_geometry)
    l64, lx = ref.flat(ref.logs), ref.flat(ref.logx)
    assert [r[:4] for r in l64] == [r[:4] for r in lx] == [r[:4] for r in ref.expect], (l64, lx, ref.expect)
    for got in (l64, lx):
        for r, e in zip(got, ref.expect):
            assert abs(r[4] - e[4]) <= 4e-16 * e[4], (r, e)
    assert ref.count == len(ref.expect)
    tree, case = pc.find(case_id)
    for p, f, k, rows in ref.plant_rows():
        (a, b, c), site, sgn = pc.block_of(p.kind, p.sign)
        q = k // 2
        for logs in (ref.logs, ref.logx):
            hit = [r for r in logs.get(f, []) if r[0] == q]
            assert len(hit) == (1 if site else 0)
            if site:
                value = {"a": a, "d2": c - 4.5, "det": -b * b}[site]
                assert hit[0][1] == site and abs(hit[0][2] - value) <= 1e-15 * abs(value), (p, hit)
        assert ref.kinds[f][q][0] == (p.kind in ("det", "ctl_2x2")), p
        want = pc.closed_form(p.kind, p.sign, p.pad)
        assert pc.delta_error(rows, want) <= 1e-18, (p, rows, want)
    # the float64 emulation in the device's place passes what the GPU tests assert
    assert pc.device_findings(ref, ref.count, lambda f: ref.Ds[f]) == []


@pytest.mark.parametrize("tree", [t.name for t in pc.TREES])
def test_controls_log_nothing(built_library, c1_geometry, tree):
    for name in ("unplanted", "controls", "controls_swapped", "coupled_sliver"):
        ref = pc.reference(f"{tree}:{name}", c1_geometry)
        assert not ref.logs and not ref.logx and ref.count == 0, name


def _refined(data, ref, K, b, passes):
    x = fe.solve(data.T, ref.Fs, ref.Ds, b)
    for _ in range(passes):
        r = np.zeros_like(b)
        r[data.idx] = b[data.idx] - K @ x[data.idx]
        x = x + fe.solve(data.T, ref.Fs, ref.Ds, r)
    return x


@pytest.mark.parametrize("tree", [t.name for t in pc.TREES])
def test_one_refinement_pass_repairs_the_coupled_replacement(built_library, c1_geometry, tree):
    """Coupled case (i): the factor is that of a matrix 1e-8 away (multipliers of 1e8); against SuperLU of the planted K
    the emulated solve is poor before refinement and better after one pass."""
    ref = pc.reference(f"{tree}:coupled_fire", c1_geometry)
    data = ref.data
    K = data.matrix(ref.Ke)
    lu = spla.splu(K.tocsc())
    for key, b in right_hand_sides(data.T, data.idx, data.N).items():
        xs = lu.solve(b[data.idx])
        e = [float(np.linalg.norm(_refined(data, ref, K, b, n)[data.idx] - xs) / np.linalg.norm(xs)) for n in (0, 1)]
        print(f"\n{tree} {key}: forward error {e[0]:.2e} before, {e[1]:.2e} after one refinement pass")
        assert e[1] < e[0], (key, e)


@pytest.mark.parametrize("mistake", fe.MISTAKES)
def test_the_gpu_assertions_catch_a_mistaken_rule(built_library, c1_geometry, mistake):
    """A mistaken emulation (float64) plays the device: over the cases, at least one of the assertions of
    test_gpu_pivot_replacement.py on the count, the pivot kind and D^-1 of the plants fails -- a tolerance by at least
    100 times."""
    caught = {}
    for case_id in pc.CASE_IDS:
        ref = pc.reference(case_id, c1_geometry)
        wrong = pc.Reference(ref.data, ref.case, mistake)
        found = pc.device_findings(ref, wrong.count, lambda f: wrong.Ds[f])
        if found:
            caught[case_id] = max(m for _, m in found)
            assert caught[case_id] >= 100.0, (case_id, found)
    assert caught, mistake
    worst = max(caught, key=caught.get)
    print(f"\n{mistake}: fails {len(caught)} of {len(pc.CASE_IDS)} cases, by at least {min(caught.values()):.3g} times the tolerance "
          f"(e.g. {worst}: {caught[worst]:.3g})")
