"""The error-indicator kernel (k_mode_indicators, plfem_mode_indicators) against its NumPy restatement
(tests/indicator_emulation.py) on the jittered square of tests/core_ties.py (128 elements, boundary edges on every side)
and on C1 at level 0 (11 313 elements): both pencils, k = 1, 33 and 70 seeded random modes, step-index tables with no,
one and seven cores, the tie discs, a disc that owns no point, and profiles with a ring and a graded layer.  The bits
of a mode's indicators must not depend on the run, on what the work buffer held, or on the modes it is computed with."""
import ctypes

import numpy as np
import pytest

from core_ties import Ties, jittered_square_mesh
from indicator_emulation import IndicatorEmulation, eps_of
from pl_fem_vectoriel_amd import IndexProfile, ModeFields, ProfiledGeometry, _native, generate_mesh

pytestmark = pytest.mark.gpu
K0 = 2 * np.pi / 1.55
ALPHA = 0.75                        # not the solver's 1: the penalty must arrive in the kernel
KMAX = 70
KS = (1, 33, 70)
KINDS = ("vectorial", "scalar")
TOL = 1e-12                         # of the largest output, the bar of the Gram tests


def material_args(geometry):
    """(cores, (eps_core, eps_clad, eps_bg), layer table) as ModeFields._indicators_staged takes them."""
    prof = getattr(geometry, "index_profile", None)
    if prof is not None:
        return np.zeros((0, 3)), (1.0, 1.0, prof.eps_background), prof.table()
    cores = np.column_stack([np.asarray(geometry.positions, dtype=np.float64).reshape(-1, 2),
                             np.asarray(geometry.core_radii, dtype=np.float64).reshape(-1)])
    return cores, (geometry.n_core ** 2, geometry.n_clad ** 2, 1.0), np.zeros((0, 8))


class Section:
    """A mesh with its locator, its emulation and, per kind, KMAX seeded random modes and eigenvalues."""

    def __init__(self, mesh, materials, device, seed):
        self.mesh, self.materials = mesh, materials
        self.fields = ModeFields(mesh, device=device)
        self.fields._ensure_locator()
        self.emu = IndicatorEmulation(mesh.p, mesh.t)
        rng = np.random.default_rng(seed)
        self.vals = {"vectorial": rng.standard_normal((2, KMAX, self.fields.nsolve)),
                     "scalar": rng.standard_normal((1, KMAX, self.fields.N))}
        self.lam = {"vectorial": (K0 * rng.uniform(1.2, 1.5, KMAX)) ** 2, "scalar": -(K0 * rng.uniform(1.2, 1.5, KMAX)) ** 2}
        self._ref = {}

    def run(self, kind, material, sel=slice(None), work=None):
        vals = np.ascontiguousarray(self.vals[kind][:, sel])
        staged, _src = self.fields._stage(vals)
        return self.fields._indicators_staged(kind, staged, self.lam[kind][sel], K0, ALPHA,
                                              *material_args(self.materials[material]), work=work)

    def ref(self, kind, material):
        """The emulation for all KMAX modes, computed once per (kind, material) and never written to."""
        key = (kind, material)
        if key not in self._ref:
            r = self.emu.eta2(self.vals[kind], kind == "vectorial", self.lam[kind], K0, ALPHA, eps_of(self.materials[material]))
            r.setflags(write=False)
            self._ref[key] = r
        return self._ref[key]


def bare(ties, positions, radii, n_core=1.535, n_clad=1.2):
    g = ties.geometry(n_core, n_clad)
    g.positions = g.core_positions = np.asarray(positions, dtype=np.float64).reshape(-1, 2)
    g.core_radii = np.asarray(radii, dtype=np.float64).reshape(-1)
    g.n_cores = len(g.core_radii)
    return g


@pytest.fixture(scope="module")
def square(gpu_device, built_library):
    mesh = jittered_square_mesh(8)
    assert mesh.t.shape[1] == 128
    ties = Ties(mesh)
    prof = IndexProfile(1.2).ring((0.5, 0.5), 0.22, 0.37, 1.40).graded((0.31, 0.62), 0.21, 1.535, 1.45, 2.0)
    for i, ((cx, cy), r) in enumerate(zip(ties.positions, ties.radii)):
        prof.disc((cx, cy), r, 1.535 if i % 2 == 0 else 1.50)
    base = ties.geometry(1.535, 1.2)
    mats = {"none": bare(ties, np.zeros((0, 2)), np.zeros(0)), "one": bare(ties, [[0.4, 0.55]], [0.23]),
            "ties": base, "empty_disc": bare(ties, [[0.503, 0.4991]], [1e-7]),
            "profile": ProfiledGeometry(base, prof, n_core=1.535, n_clad=1.2)}
    S = Section(mesh, mats, gpu_device, seed=21)
    # the disc of "empty_disc" owns no quadrature or edge point
    qx, qy = S.emu.basis.qx
    ex, ey = S.emu.edge_points()
    eps = eps_of(mats["empty_disc"])
    assert np.all(eps(qx, qy) == 1.2 ** 2) and np.all(eps(ex, ey) == 1.2 ** 2)
    yield S
    S.fields.close()


@pytest.fixture(scope="module")
def c1(gpu_device, built_library, c1_geometry):
    mesh = generate_mesh(c1_geometry, 1.0, 0)
    assert mesh.t.shape[1] == 11313
    prof = IndexProfile(1.0).disc((0.0, 0.0), 7.0, 1.45).ring((0.0, 0.0), 2.0, 3.1, 1.40).graded((0.0, 0.0), 1.5, 1.535, 1.46, 2.0)
    for (cx, cy), r in zip(np.atleast_2d(c1_geometry.positions)[1:], np.asarray(c1_geometry.core_radii).reshape(-1)[1:]):
        prof.disc((cx, cy), r, 1.53)
    S = Section(mesh, {"seven": c1_geometry, "profile": ProfiledGeometry(c1_geometry, prof)}, gpu_device, seed=22)
    yield S
    S.fields.close()


def check(S, kind, material, k):
    got = S.run(kind, material, slice(0, k))
    want = S.ref(kind, material)[:k]
    assert got.shape == want.shape == (k, S.mesh.t.shape[1])
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{kind} {material} k = {k}: error {err:.1e} of the largest output {np.abs(want).max():.2e}; "
          f"largest error relative to its own entry {np.max(np.abs(got - want) / want):.1e}")
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    assert err <= TOL
    return got


@pytest.mark.parametrize("material", ["none", "one", "ties", "empty_disc", "profile"])
@pytest.mark.parametrize("kind", KINDS)
def test_square_matches_emulation(square, kind, material):
    for k in KS:
        check(square, kind, material, k)


@pytest.mark.parametrize("material", ["seven", "profile"])
@pytest.mark.parametrize("kind", KINDS)
def test_c1_matches_emulation(c1, kind, material):
    for k in KS:
        check(c1, kind, material, k)


def test_materials_differ(square, c1):
    """The tables are told apart: the cases above do not all check one material map."""
    for S, names in ((square, ["none", "one", "ties", "profile"]), (c1, ["seven", "profile"])):
        refs = [S.ref("scalar", nm) for nm in names]
        for i in range(len(refs)):
            for j in range(i):
                assert np.max(np.abs(refs[i] - refs[j]) / refs[i]) > 1e-6          # (entry by entry: slivers dominate a maximum)
    assert np.array_equal(square.ref("scalar", "none"), square.ref("scalar", "empty_disc"))


@pytest.mark.parametrize("kind", KINDS)
def test_bits_do_not_depend_on_run_work_buffer_or_company(square, c1, kind):
    import torch
    for S, material in ((square, "profile"), (square, "ties"), (c1, "seven")):
        full = S.run(kind, material)
        assert np.array_equal(S.run(kind, material), full)
        need = ctypes.c_int64(0)
        assert S.fields._lib.plfem_indicator_work_bytes(S.fields._loc, 2 if kind == "vectorial" else 1, KMAX,
                                                        ctypes.byref(need)) == _native.PLFEM_OK
        work = torch.full(((int(need.value) + 256 + 7) // 8,), float("nan"), dtype=torch.float64, device=S.fields.tdev)
        torch.cuda.synchronize()
        assert np.array_equal(S.run(kind, material, work=work.view(torch.uint8)), full)
        for m in (0, 17, 69):
            assert np.array_equal(S.run(kind, material, slice(m, m + 1))[0], full[m])
        assert np.array_equal(S.run(kind, material, slice(0, 33)), full[:33])
        sel = np.array([69, 3, 40])
        assert np.array_equal(S.run(kind, material, sel), full[sel])


def test_vectorial_boundary_edges_contribute_nothing(square):
    """Full-length vectorial rows with values on the boundary DOFs: the flux through a boundary edge is far from 0, and
    no trace of it is in the result."""
    S = square
    rng = np.random.default_rng(5)
    vals = rng.standard_normal((2, 3, S.fields.N))
    lam = (K0 * np.array([1.3, 1.4, 1.45])) ** 2
    geometry = S.materials["one"]
    staged, _src = S.fields._stage(vals)
    # (the kind only chooses the row map of the staged record: "scalar" = rows are all N DOFs; ncomp is the record's 2)
    got = S.fields._indicators_staged("scalar", staged, lam, K0, ALPHA, *material_args(geometry))
    res, jmp = S.emu.eta2_parts(vals, False, lam, K0, ALPHA, eps_of(geometry))
    want = res + jmp
    assert np.abs(got - want).max() <= TOL * want.max()
    # what a weight of 1 on the boundary edges would have added
    P = S.emu.pieces(vals, False, lam, K0, ALPHA, eps_of(geometry))
    bnd = S.emu.nbr < 0
    extra = 0.5 * np.einsum("le,ckleg->ke", bnd * 1.0, P["flux"][0] ** 2)
    on_boundary = bnd.any(axis=0)
    # 32 boundary edges on 30 elements: the two corner elements cut off by a diagonal have two each
    assert bnd.sum() == 32 and on_boundary.sum() == 30
    assert np.all(extra[:, on_boundary] > 1e-3 * want[:, on_boundary])
    assert np.all(extra[:, ~on_boundary] == 0)


def test_records_through_the_public_surface(square):
    from pl_fem_vectoriel_amd import mode_error_indicators
    S = square
    g = S.materials["profile"]
    beta = np.sqrt(S.lam["vectorial"][:4])
    modes = [{"Ex_dofs": S.vals["vectorial"][0, m], "Ey_dofs": S.vals["vectorial"][1, m], "beta": float(beta[m])} for m in range(4)]
    res = S.fields.indicators(modes, g, alpha_p=ALPHA)
    k0 = float(g.k0)
    want = S.emu.eta2(S.vals["vectorial"][:, :4], True, beta ** 2, k0, ALPHA, eps_of(g))
    assert np.abs(res["eta2"] - want).max() <= TOL * want.max()
    assert np.array_equal(res["total"], res["eta2"].sum(axis=1))
    eta2, total = mode_error_indicators(modes, S.mesh, g, alpha_p=ALPHA)
    assert np.array_equal(eta2, res["eta2"]) and np.array_equal(total, res["total"])
    smodes = [{"field_vector": S.vals["scalar"][0, m], "beta": float(np.sqrt(-S.lam["scalar"][m]))} for m in range(3)]
    res = S.fields.indicators(smodes, S.materials["ties"])
    lam = -np.array([m["beta"] for m in smodes]) ** 2
    want = S.emu.eta2(S.vals["scalar"][:, :3], False, lam, k0, 1.0, eps_of(S.materials["ties"]))
    assert np.abs(res["eta2"] - want).max() <= TOL * want.max()
    assert S.fields.indicators([], g)["eta2"].shape == (0, 128)
    with pytest.raises(ValueError):
        S.fields.indicators([{"field_vector": S.vals["scalar"][0, 0]}], g)          # no beta: no eigenvalue


def test_argument_errors_at_the_c_abi(square):
    import torch
    S = square
    f, lib = S.fields, S.fields._lib
    k = 3
    staged, _src = f._stage(np.ascontiguousarray(S.vals["vectorial"][:, :k]))
    lam = np.ascontiguousarray(S.lam["vectorial"][:k])
    cores = np.array([[0.4, 0.55, 0.23]])
    table = S.materials["profile"].index_profile.table()
    need = ctypes.c_int64(0)
    assert lib.plfem_indicator_work_bytes(f._loc, 2, k, ctypes.byref(need)) == _native.PLFEM_OK
    assert need.value >= 8 * k * 128 + 12 * 128 + 8 * k
    for bad in ((None, 2, k), (f._loc, 0, k), (f._loc, 3, k), (f._loc, 2, 0)):
        assert lib.plfem_indicator_work_bytes(bad[0], bad[1], bad[2], ctypes.byref(need)) == _native.PLFEM_EINVAL
    assert lib.plfem_indicator_work_bytes(f._loc, 2, k, None) == _native.PLFEM_EINVAL
    work = torch.full(((int(need.value) + 256) // 8 + 1,), float("nan"), dtype=torch.float64, device=f.tdev)
    aligned = (work.data_ptr() + 255) & ~255
    out = np.full((k, 128), -1.0)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = dict(loc=f._loc, ncomp=2, k=k, modes=ctypes.c_void_p(staged.data_ptr()), indexed=1, lam=ptr(lam), k0=K0, alpha=1.0,
                cores=ptr(cores), ncore=1, ec=2.3, el=1.4, layers=None, nlayer=0, bg=1.0, work=ctypes.c_void_p(aligned),
                wb=ctypes.c_int64(need.value), out=ptr(out))

    def call(**kw):
        a = dict(good, **kw)
        return lib.plfem_mode_indicators(a["loc"], a["ncomp"], a["k"], a["modes"], a["indexed"], a["lam"], a["k0"], a["alpha"],
                                         a["cores"], a["ncore"], a["ec"], a["el"], a["layers"], a["nlayer"], a["bg"],
                                         a["work"], a["wb"], a["out"])

    nan_lam = lam.copy()
    nan_lam[1] = np.nan
    bad_table = table.copy()
    bad_table[0, 3] = bad_table[0, 2]                            # r_out = r_in
    assert call(loc=None) == _native.PLFEM_EINVAL
    for kw in (dict(ncomp=0), dict(ncomp=3), dict(k=0), dict(modes=None), dict(lam=None), dict(work=None), dict(out=None),
               dict(lam=ptr(nan_lam)), dict(k0=float("inf")), dict(alpha=float("nan")), dict(ncore=-1), dict(ncore=65),
               dict(cores=None), dict(ec=0.0), dict(el=float("nan")), dict(layers=None, nlayer=2), dict(nlayer=65, layers=ptr(table)),
               dict(layers=ptr(bad_table), nlayer=bad_table.shape[0]), dict(layers=ptr(table), nlayer=table.shape[0], bg=-1.0),
               dict(wb=ctypes.c_int64(need.value - 1)), dict(work=ctypes.c_void_p(aligned + 8))):
        assert call(**kw) == _native.PLFEM_EINVAL, kw
        assert lib.plfem_locator_last_error(f._loc).decode().startswith("plfem_mode_indicators: "), kw
    assert np.all(out == -1.0)                                   # nothing was written
    torch.cuda.synchronize()
    assert bool(torch.isnan(work).all())                         # ... and nothing launched
    assert call() == _native.PLFEM_OK and np.all(out > 0)        # the locator is still usable
    assert call(layers=ptr(table), nlayer=table.shape[0], bg=1.44, cores=None, ncore=-5, ec=0.0) == _native.PLFEM_OK
