"""Host checks of the operator case matrix (operator_cases.py) and of the scalar emulation: the cases reach every kernel
form the launch plan can pick, at P = 1 and P = 4, and each fits the LDS budget of the block sweeps."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import front_emulation as fe
import operator_cases as oc
from oracle import scalar
from oracle.p2 import MeshTriLite, P2Basis
from pl_fem_vectoriel_amd.mesh import generate_mesh


@pytest.fixture(scope="module")
def case_forms(built_library, c1_geometry):
    meshes, out = {}, {}
    for case in oc.CASES:
        if case.mesh not in meshes:
            meshes[case.mesh] = oc.mesh_of(case, c1_geometry)
        sym = oc.symbolic_of(case, meshes[case.mesh])
        out[case.name] = fe.level_forms(sym)
        sym.close()
    return out


def test_case_matrix_covers_every_form(case_forms):
    possible = oc.forms_possible()
    assert len(possible) == 22           # forward: 4 forms x {leaf, inner}; backward: leaf tile, inner rows 8 / 16; x 2 pencils
    by_p = {1: set(), 4: set()}
    for case in oc.CASES:
        forms = case_forms[case.name]
        reached = oc.forms_reached(forms, case.dpn)
        assert reached <= possible, (case.name, reached - possible)
        by_p[1] |= reached
        if forms[0]["max_block_p"] == fe.BLOCK_P:
            by_p[4] |= reached
    for P, reached in by_p.items():
        assert reached == possible, (P, sorted(possible - reached))


def test_every_case_fits_the_block_lds_budget(case_forms):
    for case in oc.CASES:
        forms = case_forms[case.name]
        worst = max(r["max_m"] for r in forms)
        assert fe.lds_need(fe.BLOCK_P, worst) <= fe.LDS_LIMIT, (case.name, worst)
        assert all(r["max_block_p"] == fe.BLOCK_P for r in forms)
        # the forms the case is in the matrix for
        if "one front" in case.reaches:
            assert len(forms) == 1 and forms[0]["leaf"] and forms[0]["fwd"] == "k_fwd_rows<P,1,4>" and forms[0]["bwd"] == "k_bwd"
        if "leaf-level mixed" in case.reaches:
            assert forms[-1]["fwd"] == "k_fwd_mix"
        if "inner-level mixed" in case.reaches:
            assert any(r["fwd"] == "k_fwd_mix" for r in forms[:-1])
        if "8 leaves" in case.reaches:
            assert len(forms) == 4 and forms[-1]["fwd"] == "k_fwd_rows<P,1,4>"
    # the largest front the block sweeps accept, and one past it
    worst_ok = (fe.LDS_LIMIT - 8 * 8 * fe.BLOCK_P * 64) // (8 * fe.BLOCK_P) - 2
    assert fe.lds_need(fe.BLOCK_P, worst_ok) <= fe.LDS_LIMIT < fe.lds_need(fe.BLOCK_P, worst_ok + 1)


def test_level_forms_restate_the_plan(case_forms):
    """Internal consistency of the restatement: workgroup counts and kernel names follow the row counts."""
    for case in oc.CASES:
        for lev, r in enumerate(case_forms[case.name]):
            assert r["count"] == 1 << lev
            # a workgroup per front with rows (forward) / per inner front, and per leaf with owned DOFs (backward); only a
            # mesh in several parts (topology_cases.py) has a front without rows: its empty root
            assert r["fwd_n"] >= r["fronts_m"] and r["bwd_n"] >= (r["fronts_s2"] if r["leaf"] else r["count"])
            assert r["fronts_m"] == r["count"] or (case in oc.TOPOLOGY_CASES and lev == 0 and r["max_m"] == 0)
            assert (r["fwd"] == "k_fwd_mix") == bool(r["fwd_mixed"])
            assert r["steps"] == -(-r["max_s2"] // fe.NB)


@pytest.mark.parametrize("leaf", [24, 8])
def test_scalar_emulation_matches_splu(built_library, c1_geometry, leaf):
    """The scalar pencil (one unknown per node, no Dirichlet rows) through the emulated front tree solves
    (K - k0^2 M_eps - sigma M) x = b to the accuracy of SuperLU, with both pivot kinds tested on every pair."""
    g = c1_geometry
    mesh = generate_mesh(g, 0.5, 0)
    case = oc.Case("s", ("c1", 0.5, 0), leaf, 1, False, "")
    sym = oc.symbolic_of(case, mesh)
    om = MeshTriLite(mesh.p, mesh.t)
    em = scalar.element_matrices(g, P2Basis(om))
    K, M, Me, _ = scalar.assemble(g, om, eliminate_zeros=False)
    sigma = scalar.shift(g)
    T = fe.FrontTree(sym)
    assert T.dpn == 1 and T.m(0) == int(T.fs[0] + T.fb[0])
    kinds = {}
    Fs, Ds = fe.factor(T, fe.element_K_scalar(em, g.k0 ** 2, sigma), kinds)
    assert sum(len(k) for k in kinds.values()) * 2 == sum(T.s2(f) for f in range(T.nf))
    Kt = (K - g.k0 ** 2 * Me - sigma * M).tocsc()
    b = np.random.default_rng(0).standard_normal(sym.N)
    x = fe.solve(T, Fs, Ds, b)
    xs = spla.splu(Kt).solve(b)
    assert np.linalg.norm(x - xs) / np.linalg.norm(xs) < 1e-8
    berr = np.abs(Kt @ x - b).max() / (abs(Kt) @ np.abs(x) + np.abs(b)).max()
    assert berr < 1e-14
    sym.close()
