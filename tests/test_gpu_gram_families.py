"""The seven same-mesh Gram calls on one small shape (k_mode_grams, k_core_grams, k_profile_grams, k_flux_grams,
k_velocity_grams, k_moment_grams, k_weighted_grams; the two compactions; k_overlap_reduce): six of the kernels share one
frame (GramFrame: the chunk-pair indices, the feature pass, the loads of a lane's block and the partial-slot formula) and
k_mode_grams writes the same out, and this file pins that frame where it can go wrong at the least cost: the 50-element unit square (300 quadrature points: 18 full
tiles of 16 and one of 12, fewer tiles than slices), 33 modes (two chunks per side, the second with one mode), a core and
a velocity with empty lists, five tangents (two column groups).  Every call against its NumPy emulation at the bound of
its own test file (1e-12 of the largest reference entry), for vectorial and scalar records (the flux call takes
vectorial records only), under core discs, a layer profile and a sampled map where the call takes them; and three
checks of bits: a mode's entries do not depend on the chunk count, the cores sum to the core region, and no call reads
a work buffer it has not written."""
from types import SimpleNamespace

import numpy as np
import pytest

from core_gram_emulation import CoreGramEmulation
from gram_emulation import GramEmulation
from moment_gram_emulation import MomentGramEmulation
from power_emulation import PowerEmulation
from profile_gram_emulation import ProfileGramEmulation
from tangent_gram_emulation import TangentGramEmulation, random_tangent
from velocity_gram_emulation import VelocityGramEmulation
from pl_fem_vectoriel_amd import IndexProfile, ModeFields, ProfiledGeometry
from pl_fem_vectoriel_amd.mesh import unit_square_mesh
from test_gpu_cores import discs, records, vals
from test_gpu_field_instances import _scratch_filled
from test_gpu_power import GRAM_TOL
from test_gpu_profile_tangent import whole_profile_tangent

pytestmark = pytest.mark.gpu

KINDS = ("vectorial", "scalar")
K, K_SHORT = 33, 20
TOL = 1e-12             # of the largest reference entry: the bound of every family's own test file
ORIGIN = (0.3, -0.2)
assert GRAM_TOL == TOL


def materials():
    """Core discs (the third holds no quadrature point of the unit square), a layer profile, and the profile over a map."""
    g = discs([(0.3, 0.3), (0.7, 0.6), (5.0, 5.0)], [0.2, 0.15, 0.1])
    layers = lambda p: p.disc((0.3, 0.3), 0.2, 1.50).ring((0.65, 0.6), 0.1, 0.22, 1.40).graded((0.7, 0.25), 0.15, 1.535, 1.45, 2)
    x, y = np.linspace(-0.05, 1.1, 7), np.linspace(0.1, 0.95, 5)       # the map covers a part of the square
    n = 1.25 + 0.2 * np.random.default_rng(11).uniform(size=(5, 7))
    return {"discs": g,
            "profile": ProfiledGeometry(g, layers(IndexProfile(1.2)), n_core=1.535, n_clad=1.2),
            "map": ProfiledGeometry(g, layers(IndexProfile(1.2).sampled(x, y, n)), n_core=1.535, n_clad=1.2)}


def velocities(mesh):
    """A random field on every vertex, and a translation: G = 0 on every element, an empty list."""
    nv = mesh.p.shape[1]
    return np.ascontiguousarray(np.stack([np.random.default_rng(12).standard_normal((nv, 2)), np.tile((0.3, -1.1), (nv, 1))]))


def tangents(prof):
    """Five: two column groups of k_weighted_grams, the second with one tangent and the two moment columns."""
    return [random_tangent(prof, seed=13), random_tangent(prof, seed=14, with_map=False), whole_profile_tangent(prof)] + prof.unit_tangents()[:2]


CALLS = ("grams", "core_grams", "moment_grams", "profile_grams", "flux_grams", "velocity_grams", "tangent_grams")


def families(kind):
    """(call, material) of every family for a record kind."""
    out = [("grams", "discs"), ("core_grams", "discs"), ("moment_grams", "discs"), ("profile_grams", "profile"),
           ("profile_grams", "map"), ("velocity_grams", "discs"), ("velocity_grams", "profile"), ("velocity_grams", "map"),
           ("tangent_grams", "profile"), ("tangent_grams", "map")]
    if kind == "vectorial":
        out += [("flux_grams", "discs"), ("flux_grams", "profile"), ("flux_grams", "map")]
    return out


def device_call(S, call, mat, modes):
    """The family's call of ModeFields: a dict of arrays."""
    mf, geo = S.mf, S.materials[mat]
    if call == "grams":
        return mf.grams(modes, geo)
    if call == "core_grams":
        return mf.core_grams(modes, geo)
    if call == "moment_grams":
        return mf.moment_grams(modes, geo, origin=ORIGIN)
    if call == "profile_grams":
        return mf.profile_grams(modes, geo)
    if call == "flux_grams":
        return mf.flux_grams(modes, geo)
    if call == "velocity_grams":
        return mf.velocity_grams(modes, geo, S.velocities)
    return mf.profile_tangent_grams(modes, geo, S.tangents[mat], moments=True, origin=ORIGIN)


def emulated(S, call, mat, kind):
    """The same from the family's emulation, for all K modes."""
    geo, v, indexed = S.materials[mat], vals(S.modes[kind]), kind == "vectorial"
    p, t = S.mesh.p, S.mesh.t
    if call == "grams":
        return GramEmulation(p, t).grams(v, indexed, geo)
    if call == "core_grams":
        return CoreGramEmulation(p, t).core_grams(v, indexed, geo)
    if call == "moment_grams":
        return MomentGramEmulation(p, t).moment_grams(v, indexed, geo, ORIGIN)
    if call == "profile_grams":
        return ProfileGramEmulation(p, t).profile_grams(v, indexed, geo.index_profile)
    if call == "flux_grams":
        return PowerEmulation(p, t).flux_grams(v, True, geo)
    if call == "velocity_grams":
        em = VelocityGramEmulation(p, t)
        out, count = em.velocity_grams(v, indexed, geo, S.velocities)
        return dict(em.named(out), count=count)
    em = TangentGramEmulation(p, t)
    tans = S.tangents[mat]
    return em.named(em.tangent_grams(v, indexed, geo.index_profile, tans, True, ORIGIN), len(tans), True)


def setup(mesh, mf):
    mats = materials()
    rng = np.random.default_rng(10)
    S = SimpleNamespace(mesh=mesh, mf=mf, materials=mats, velocities=velocities(mesh),
                        tangents={m: tangents(mats[m].index_profile) for m in ("profile", "map")},
                        modes={"vectorial": records(rng, "vectorial", mf.nsolve, K), "scalar": records(rng, "scalar", mf.N, K)})
    return S


@pytest.fixture(scope="module")
def shape(gpu_device, built_library):
    mesh = unit_square_mesh(5)
    mf = ModeFields(mesh, device=gpu_device)
    S = setup(mesh, mf)
    assert mf.ne == 50 and (6 * mf.ne) // 16 == 18 and (6 * mf.ne) % 16 == 12 and 32 < K < 64
    assert all(len(t) == 5 for t in S.tangents.values())
    # what every test below compares with: each family's 33-mode call, made once
    S.full = {kind: {fam: device_call(S, *fam, S.modes[kind]) for fam in families(kind)} for kind in KINDS}
    yield S
    mf.close()


def _integer(nm):
    return nm in ("points", "count")


@pytest.mark.parametrize("kind", KINDS)
def test_every_family_matches_its_emulation(shape, kind):
    S = shape
    for fam in families(kind):
        got, ref = S.full[kind][fam], emulated(S, *fam, kind)
        assert set(got) == set(ref), fam
        for nm in ref:
            if _integer(nm):
                assert np.array_equal(got[nm], ref[nm]), (fam, nm, got[nm], ref[nm])
                continue
            assert got[nm].shape == ref[nm].shape, (fam, nm)
            # per core, per velocity and per column where the output has them: a small one hides behind no large one
            pairs = list(zip(got[nm], ref[nm])) if ref[nm].ndim == 3 else [(got[nm], ref[nm])]
            if fam[0] == "core_grams":                                   # as tests/test_gpu_cores.py: of the sum over the cores
                scale = np.abs(ref[nm].sum(0)).max()
                assert np.abs(got[nm] - ref[nm]).max() <= TOL * scale, (fam, nm)
                assert (got[nm][ref["points"] == 0] == 0).all(), (fam, nm)
                continue
            for i, (a, b) in enumerate(pairs):
                scale = np.abs(b).max()
                if scale == 0:                                           # the translation: exact zeros
                    assert fam[0] == "velocity_grams" and i == 1 and (a == 0).all(), (fam, nm, i)
                    continue
                err = np.abs(a - b).max() / scale
                print(f"{kind} {fam[0]} {fam[1]} {nm}[{i}]: {err:.2e}")
                assert err <= TOL, (fam, nm, i, err)
        if fam[0] == "core_grams":
            assert ref["points"][2] == 0 and (ref["points"][:2] > 0).all() and (ref["points"][:2] % 16 != 0).all()
        if fam[0] == "velocity_grams":
            assert list(ref["count"]) == [S.mf.ne, 0]


@pytest.mark.parametrize("kind", KINDS)
def test_the_first_modes_have_the_same_bits_in_a_one_chunk_call(shape, kind):
    """Two chunks per side against one: the chunk-pair indices and the slots of the frame, for every family."""
    S = shape
    for fam in families(kind):
        short = device_call(S, *fam, S.modes[kind][:K_SHORT])
        for nm, full in S.full[kind][fam].items():
            want = full if _integer(nm) else full[..., :K_SHORT, :K_SHORT]
            assert np.array_equal(short[nm], want), (fam, nm)


@pytest.mark.parametrize("kind", KINDS)
def test_cores_sum_to_the_core_region_of_mode_grams(shape, kind):
    """The listed walk of k_core_grams against the region branch of k_mode_grams, to the bound of tests/test_gpu_cores.py."""
    G, C = shape.full[kind][("grams", "discs")], shape.full[kind][("core_grams", "discs")]
    M = C["Mx"] + C["My"] if kind == "vectorial" else C["M"]
    assert np.abs(G["M_core"]).max() > 0
    assert np.abs(M.sum(0) - G["M_core"]).max() <= 1e-12 * np.abs(G["M_core"]).max()
    if kind == "vectorial":
        assert np.abs(C["K"].sum(0) - G["K_core"]).max() <= 1e-12 * np.abs(G["K_core"]).max()


@pytest.mark.parametrize("kind", KINDS)
def test_a_filled_work_buffer_changes_no_bit(shape, kind, monkeypatch):
    """Every partial slot that k_overlap_reduce reads is written by the call, and so is every list entry that is read."""
    S = shape
    for fam in families(kind):
        seen = []
        with _scratch_filled(monkeypatch, 0xFF, seen):
            again = device_call(S, *fam, S.modes[kind])
        assert seen, fam
        for nm, full in S.full[kind][fam].items():
            assert np.array_equal(again[nm], full), (fam, nm)
