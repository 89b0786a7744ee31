"""Mode Grams and group index on the GPU (k_mode_grams) on solver output at C1 L = 0: the kernel against the NumPy emulation
(tests/gram_emulation.py), against the existing overlap kernel, the Rayleigh check against the solver's pencil, bit-identical
repeats, and n_g against finite differences of three GPU solves on one mesh object."""
import copy

import numpy as np
import pytest

from gram_emulation import GramEmulation
from pl_fem_vectoriel_amd import ModeFields, generate_mesh, mode_dispersion, mode_overlap
from pl_fem_vectoriel_amd.solver_fem import ScalarHelmholtzSolver, TrueVectorialMaxwellSolver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c1(c1_geometry, gpu_device, built_library):
    mesh = generate_mesh(c1_geometry, 1.0, 0)
    vsol = TrueVectorialMaxwellSolver(c1_geometry, device=gpu_device, eig_tol=1e-10)
    ssol = ScalarHelmholtzSolver(c1_geometry, device=gpu_device)
    vec = vsol.solve_vectorial_modes(mesh, 20)
    scal = ssol.solve(mesh, 10)
    mf = ModeFields(mesh, device=gpu_device, solver=vsol)
    yield {"mesh": mesh, "vsol": vsol, "ssol": ssol, "vec": vec, "scal": scal, "mf": mf}
    mf.close()
    vsol.clear_cache()
    ssol.clear_cache()
    import torch
    torch.cuda.empty_cache()


def _vals(modes):
    if "Ex_dofs" in modes[0]:
        return np.stack([np.array([m["Ex_dofs"] for m in modes]), np.array([m["Ey_dofs"] for m in modes])])
    return np.array([m["field_vector"] for m in modes])[None]


def test_kernel_grams_match_emulation_and_overlap(c1, c1_geometry):
    mesh, mf = c1["mesh"], c1["mf"]
    em = GramEmulation(mesh.p, mesh.t)
    g = c1_geometry
    for modes, indexed in ((c1["vec"], True), (c1["scal"], False)):
        G = mf.grams(modes, g)
        ref = em.grams(_vals(modes), indexed, g)
        assert set(G) == set(ref)
        for nm in ref:
            err = np.abs(G[nm] - ref[nm]).max() / np.abs(ref[nm]).max()
            print(f"{'vectorial' if indexed else 'scalar'} {nm}: {err:.2e} relative to max |G|")
            assert err <= 1e-12, nm
        # the existing overlap kernel on the same mesh: M = M_core + M_clad, B-weight = sum_r M_r / eps_r
        O = mode_overlap(modes, mf, modes, mf)
        assert np.abs(G["M_core"] + G["M_clad"] - O).max() <= 1e-12 * np.abs(O).max()
        Ow = mode_overlap(modes, mf, modes, mf, weight=g)
        Bw = G["M_core"] / g.n_core ** 2 + G["M_clad"] / g.n_clad ** 2
        assert np.abs(Bw - Ow).max() <= 1e-12 * np.abs(Ow).max()
        again = mf.grams(modes, g)
        assert all(np.array_equal(G[nm], again[nm]) for nm in G)


def test_rayleigh_defect_and_records_untouched(c1, c1_geometry):
    for modes in (c1["vec"], c1["scal"]):
        before = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in m.items()} for m in modes]
        res = mode_dispersion(modes, c1["mf"], c1_geometry)
        print(f"rayleigh defect max {res['rayleigh_defect'].max():.2e}; n_g {res['n_g'].min():.6f}..{res['n_g'].max():.6f}; "
              f"DMGD {res['dmgd_ps_per_m']:.3e} ps/m; clusters {int(res['cluster'].max()) + 1}")
        assert res["rayleigh_defect"].max() <= 1e-10
        for a, b in zip(modes, before):
            assert set(a) == set(b)
            for k in a:
                assert np.array_equal(a[k], b[k]) if isinstance(b[k], np.ndarray) else a[k] == b[k]
        again = mode_dispersion(modes, c1["mf"], c1_geometry)
        assert np.array_equal(res["n_g"], again["n_g"]) and np.array_equal(res["coupling"], again["coupling"])


def _fd(solver, solve, mesh, geometry, modes, delta=1e-5):
    """beta at k0 (1 +- delta) of each mode, matched by a unique |cos| > 0.999 partner (nan otherwise), from two more solves on
    the same mesh object and the same solver (its analysis and context are reused)."""
    out = []
    x = _vals(modes).transpose(1, 0, 2).reshape(len(modes), -1)
    x = x / np.linalg.norm(x, axis=1)[:, None]
    g0, k00 = solver.geometry, solver.k0
    try:
        for s in (1 + delta, 1 - delta):
            g = copy.copy(geometry)
            g.k0, g.wavelength = geometry.k0 * s, geometry.wavelength / s
            solver.geometry, solver.k0 = g, g.k0
            other = solve(mesh)
            y = _vals(other).transpose(1, 0, 2).reshape(len(other), -1)
            c = np.abs(x @ (y / np.linalg.norm(y, axis=1)[:, None]).T)
            b = np.array([other[int(np.argmax(r))]["beta"] for r in c])
            b[(c > 0.999).sum(1) != 1] = np.nan
            out.append(b)
    finally:
        solver.geometry, solver.k0 = g0, k00
    return out, 2 * delta * geometry.k0


def test_group_index_against_finite_differences_of_gpu_solves(c1, c1_geometry):
    mesh = c1["mesh"]
    cases = (("vectorial", c1["vsol"], lambda m: c1["vsol"].solve_vectorial_modes(m, 20), c1["vec"], 1.0),
             ("scalar", c1["ssol"], lambda m: c1["ssol"].solve(m, 10), c1["scal"], -1.0))
    for kind, solver, solve, modes, sgn in cases:
        res = mode_dispersion(modes, c1["mf"], c1_geometry)
        (bp, bm), h = _fd(solver, solve, mesh, c1_geometry, modes)
        mu = sgn * np.array([m["beta"] for m in modes]) ** 2
        mup, mum = sgn * bp ** 2, sgn * bm ** 2
        errs = []
        for i in range(len(modes)):
            j = int(np.argsort(np.abs(mu - mu[i]))[1])
            moved = max(abs((mup[i] - mup[j]) - (mu[i] - mu[j])), abs((mum[i] - mum[j]) - (mu[i] - mu[j])))
            if not np.isfinite(moved) or abs(mu[i] - mu[j]) < 100 * moved:
                continue
            errs.append(abs(res["n_g"][i] - (bp[i] - bm[i]) / h))
        print(f"{kind}: {len(errs)} of {len(modes)} modes compared, worst |n_g(HF) - n_g(FD)| = {max(errs):.2e}")
        assert len(errs) >= 3
        assert max(errs) <= 1e-6
