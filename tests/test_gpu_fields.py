"""Mode fields on the GPU (k_sample_fields, k_field_overlap) on solver output at C1: DOF values at the mesh's own DOF
locations, agreement with the NumPy emulation (tests/fields_emulation.py), the nested-refinement identity, the
B = M_(1/eps) inner product on one mesh, mesh convergence L = 0 -> 1, and bit-identical repeats."""
import numpy as np
import pytest
import scipy.sparse as sp

from fields_emulation import Emulation, LOOSE
from oracle.p2 import PHI_Q
from pl_fem_vectoriel_amd import ModeFields, generate_mesh, mode_overlap
from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver, mesh_key

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c1_l0(c1_geometry, gpu_device, built_library):
    mesh = generate_mesh(c1_geometry, 1.0, 0)
    solver = TrueVectorialMaxwellSolver(c1_geometry, device=gpu_device)
    vec = solver.solve_vectorial_modes(mesh, 20)
    scal = ScalarHelmholtzSolver(c1_geometry, device=gpu_device).solve(mesh, 10)
    mf = ModeFields(mesh, device=gpu_device, solver=solver)
    assert mf.sym is solver._cache[mesh_key(mesh)]["sym"]
    yield {"mesh": mesh, "solver": solver, "vec": vec, "scal": scal, "mf": mf, "em": Emulation(mesh.p, mesh.t)}
    mf.close()                                  # the device memory goes back before the next test module
    solver.clear_cache()
    import torch
    torch.cuda.empty_cache()


OWN_DOF_TOL = 1e-13     # a DOF location sampled in an element of that DOF, of the largest DOF value
ANY_DOF_TOL = 1e-8      # ... in a neighbouring element (slivers)


def _stack(modes, key):
    return np.array([m[key] for m in modes])


def test_sampling_at_own_doflocs_returns_dof_values(c1_l0):
    mf, vec, scal = c1_l0["mf"], c1_l0["vec"], c1_l0["scal"]
    dl = mf.sym.array("doflocs").reshape(2, mf.N)
    interior = mf.sym.array("interior")
    bnd = np.setdiff1d(np.arange(mf.N), interior)
    out = mf.sample(vec, dl)
    assert (out["element"] >= 0).all()
    edof = mf.sym.array("edof").reshape(6, mf.ne)
    own = (edof[:, out["element"]] == np.arange(mf.N)[None]).any(0)       # the point went to an element of its own DOF
    p, t = c1_l0["mesh"].p, c1_l0["mesh"].t
    e = out["element"]
    det = np.abs((p[0, t[1, e]] - p[0, t[0, e]]) * (p[1, t[2, e]] - p[1, t[0, e]])
                 - (p[0, t[2, e]] - p[0, t[0, e]]) * (p[1, t[1, e]] - p[1, t[0, e]]))
    for comp, key in (("Hx", "Ex_dofs"), ("Hy", "Ey_dofs")):
        ref = np.zeros((len(vec), mf.N))
        ref[:, interior] = _stack(vec, key)
        err = np.abs(out[comp] - ref).max(0) / np.abs(ref).max()
        w = int(np.argmax(err))
        print(f"{comp}: worst relative error {err[w]:.2e} at DOF {w} (boundary {w in set(bnd.tolist())}, element {e[w]}, "
              f"own element {own[w]}, |det J| {det[w]:.2e}); DOFs above 1e-13: {int((err > 1e-13).sum())} of {mf.N}")
        assert (err[own] <= OWN_DOF_TOL).all()
        assert err.max() <= ANY_DOF_TOL
    u = mf.sample(scal, dl)["u"]
    ref = _stack(scal, "field_vector")
    err = np.abs(u - ref).max(0) / np.abs(ref).max()
    print(f"u: worst relative error {err.max():.2e}; DOFs above 1e-13: {int((err > 1e-13).sum())}")
    assert (err[own] <= OWN_DOF_TOL).all() and err.max() <= ANY_DOF_TOL


def _compare(out, ref, elem_gpu, elem_em, near, comps):
    same = elem_gpu == elem_em
    assert (same | (near >= 2)).all(), np.nonzero(~same & (near < 2))[0][:10]
    outside = (elem_em < 0) & (near == 0)
    assert (elem_gpu[outside] == -1).all()
    for c, nm in enumerate(comps):
        scale = np.abs(ref[c]).max()
        if nm == "Hz_im":                      # the gradient jumps across elements: compare where both chose one element
            assert np.abs(out[nm][:, same] - ref[c][:, same]).max() <= 1e-12 * scale
        else:
            assert np.abs(out[nm] - ref[c]).max() <= 1e-12 * scale
        assert (out[nm][:, outside] == 0).all()


def test_sampling_matches_emulation(c1_l0):
    mf, em, vec, scal = c1_l0["mf"], c1_l0["em"], c1_l0["vec"], c1_l0["scal"]
    x0, x1, y0, y1 = mf.bbox
    rng = np.random.default_rng(7)
    pts = np.vstack([rng.uniform(x0 - 2, x1 + 2, 100_000), rng.uniform(y0 - 2, y1 + 2, 100_000)])
    grid = mf.sample_grid(vec, 160, 120)
    gpts = np.vstack([np.tile(grid["x"], 120), np.repeat(grid["y"], 160)])
    vals = np.stack([_stack(vec, "Ex_dofs"), _stack(vec, "Ey_dofs")])
    beta = np.array([m["beta"] for m in vec])
    svals = _stack(scal, "field_vector")[None]
    for P in (pts, gpts):
        loc = em.locate(P)
        ref, elem_em = em.sample(vals, P, True, beta=beta, located=loc)
        out = mf.sample(vec, P)
        _compare(out, ref, out["element"], elem_em, loc[3], ("Hx", "Hy", "Hz_im"))
        ref_s, _ = em.sample(svals, P, False, located=loc)
        out_s = mf.sample(scal, P)
        _compare(out_s, ref_s, out_s["element"], elem_em, loc[3], ("u",))
    flat = {k: (v.reshape(v.shape[0], -1) if k in ("Hx", "Hy", "Hz_im") else v) for k, v in grid.items()}
    again = mf.sample(vec, gpts)
    for k in ("Hx", "Hy", "Hz_im"):
        assert np.array_equal(flat[k], again[k])
    assert np.array_equal(grid["element"].reshape(-1), again["element"])


def _mass(em, interior):
    b = em.basis
    Me = np.einsum("aq,bq,eq->eab", PHI_Q, PHI_Q, b.dx)
    rows = np.repeat(b.element_dofs.T[:, :, None], 6, axis=2)
    cols = np.repeat(b.element_dofs.T[:, None, :], 6, axis=1)
    M = sp.csr_matrix((Me.ravel(), (rows.ravel(), cols.ravel())), shape=(b.N, b.N))
    return M[interior][:, interior]


def test_nested_refinement_identity(c1_l0):
    mesh, mf, vec, em = c1_l0["mesh"], c1_l0["mf"], c1_l0["vec"], c1_l0["em"]
    fine = mesh.refined()
    mf1 = ModeFields(fine, device=mf.device)
    dl1 = mf1.sym.array("doflocs").reshape(2, mf1.N)[:, mf1.sym.array("interior")]
    s = mf.sample(vec, dl1, hz=False)
    vec_fine = [{"Ex_dofs": s["Hx"][i], "Ey_dofs": s["Hy"][i], "beta": m["beta"]} for i, m in enumerate(vec)]
    O = mode_overlap(vec, mf, vec_fine, mf1)
    M = _mass(em, mf.sym.array("interior"))
    V = [_stack(vec, "Ex_dofs"), _stack(vec, "Ey_dofs")]
    ref = sum(v @ (M @ v.T) for v in V)
    assert np.abs(O - ref).max() <= 1e-12 * np.abs(ref).max()


def test_geometry_weight_reproduces_the_b_inner_product(c1_l0, c1_geometry):
    mesh, mf, vec, solver = c1_l0["mesh"], c1_l0["mf"], c1_l0["vec"], c1_l0["solver"]
    ent = solver._cache[mesh_key(mesh)]
    sym, ctx = ent["sym"], ent["ctx"]
    B = sp.csr_matrix((ctx.block_values("Minv"), sym.array("colind"), sym.array("rowptr")), shape=(sym.N, sym.N))
    interior = sym.array("interior")
    B = B[interior][:, interior]
    V = [_stack(vec, "Ex_dofs"), _stack(vec, "Ey_dofs")]
    ref = sum(v @ (B @ v.T) for v in V)
    O = mode_overlap(vec, mf, vec, mf, weight=c1_geometry)
    assert np.abs(O - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(O, mode_overlap(vec, mf, vec, mf, weight=c1_geometry))


def test_mesh_convergence_l0_to_l1(c1_l0, c1_geometry, gpu_device):
    """C1 at L = 0 against L = 1 with normalize=True.  The L = 1 mesh is the L = 0 mesh refined, so the products are
    integrated exactly and every power coupling is <= 1.  The modes the solver returns near its shift (n_eff ~ 1.26, a
    dense spectrum) are NOT the same modes at the two refinements: the measured coupling is
    printed, and the >= 0.99 bar is checked on the L = 0 modes carried onto the L = 1 mesh (nested spaces), where it
    must hold whatever the physics."""
    mesh0, vec0, mf0 = c1_l0["mesh"], c1_l0["vec"], c1_l0["mf"]
    mesh1 = generate_mesh(c1_geometry, 1.0, 1)
    solver1 = TrueVectorialMaxwellSolver(c1_geometry, device=gpu_device)
    vec1 = solver1.solve_vectorial_modes(mesh1, 20)
    mf1 = ModeFields(mesh1, device=gpu_device, solver=solver1)
    P = mode_overlap(vec0, mf0, vec1, mf1, normalize=True)
    n1 = np.array([m["n_eff"] for m in vec1])

    def cluster_power(P, n):
        out = []
        for i in range(P.shape[0]):
            j = int(np.argmax(P[i]))
            out.append(float(P[i, np.abs(n - n[j]) < 1e-6].sum()))
        return np.array(out)

    measured = cluster_power(P, n1)
    print("C1 L0 -> L1 solver modes, power in the degenerate cluster: min %.3e max %.3e; n_eff L0 %.6f..%.6f, L1 %.6f..%.6f"
          % (measured.min(), measured.max(), vec0[-1]["n_eff"], vec0[0]["n_eff"], n1[-1], n1[0]))
    assert P.max() <= 1 + 1e-9 and P.min() >= 0
    assert np.array_equal(P, mode_overlap(vec0, mf0, vec1, mf1, normalize=True))
    dl1 = mf1.sym.array("doflocs").reshape(2, mf1.N)[:, mf1.sym.array("interior")]
    s = mf0.sample(vec0, dl1, hz=False)
    carried = [{"Ex_dofs": s["Hx"][i], "Ey_dofs": s["Hy"][i]} for i in range(len(vec0))]
    Pc = mode_overlap(vec0, mf0, carried, mf1, normalize=True)
    n0 = np.array([m["n_eff"] for m in vec0])
    assert cluster_power(Pc, n0).min() >= 0.99
    assert np.abs(np.diag(Pc) - 1).max() <= 1e-9
    mf1.close()
    solver1.clear_cache()
