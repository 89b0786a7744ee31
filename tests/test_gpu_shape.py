"""Velocity Grams and shape sensitivities on the GPU (k_velocity_flag, k_velocity_count, k_velocity_fill, k_velocity_grams,
k_velocity_symmetrise): the kernels against their NumPy emulation on discs, layers, maps and closed-rim ties; identities
with the existing Gram kernels; the bit contract; the argument checks of the C ABI on a live locator; d n_eff / d (x_c,
y_c, r_c) against central differences of GPU re-solves on the moved mesh; and the scaling identity with the group
index."""
import ctypes

import numpy as np
import pytest

import test_gpu_profile_tangent as tpt
from pl_fem_vectoriel_amd import (ModeFields, PhotonicLanternGeometry, TriMesh, _native, core_velocities, mode_dispersion,
                                  shape_response)
from map_cases import m3l
from profile_cases import POS, RAD, p5, three_core, tie_square
from velocity_gram_emulation import NAMES, VelocityGramEmulation

pytestmark = pytest.mark.gpu
KINDS = ("vectorial", "scalar")
GRADIENT_FORMS = ("dK_w", "dD", "dS")
_random_records, _vals = tpt._random_records, tpt._vals


# ---- what the tests share --------------------------------------------------------------------------------------------
def one_vertex(mesh, at):
    """An interior vertex near ``at`` and the elements round it."""
    v = int(np.argmin((mesh.p[0] - at[0]) ** 2 + (mesh.p[1] - at[1]) ** 2))
    return v, int((mesh.t == v).any(0).sum())


def velocity_batch(mesh, geometry=None, at=(2.6, 2.1)):
    """(V, names, ring): the core fields of ``geometry`` (15 on the three-core mesh), two random full-support fields, a field
    that is non-zero at one interior vertex, the zero field, a translation of everything, and V = x."""
    rng = np.random.default_rng(77)
    nv = mesh.p.shape[1]
    V, names = [], []
    if geometry is not None:
        cv, labels = core_velocities(mesh, geometry)
        V += list(cv)
        names += labels
    V += [rng.standard_normal((nv, 2)), rng.standard_normal((nv, 2))]
    v, ring = one_vertex(mesh, at)
    bump = np.zeros((nv, 2))
    bump[v] = (0.7, -0.4)
    V += [bump, np.zeros((nv, 2)), np.tile((0.3, -1.1), (nv, 1)), mesh.p.T.copy()]
    names += ["random0", "random1", "bump", "zero", "translation", "scaling"]
    return np.ascontiguousarray(np.stack(V)), names, ring


@pytest.fixture(scope="module")
def sections(gpu_device, built_library):
    g, mesh = three_core()
    _, gt, pgt, mesht = tie_square()
    batch = velocity_batch(mesh, g)
    assert batch[0].shape[0] == 21
    return {"three": (g, mesh, batch), "p5": (p5(g), mesh, batch), "m3l": (m3l(g), mesh, batch),
            "square": (pgt, mesht, velocity_batch(mesht, None, at=(0.52, 0.47)))}


@pytest.fixture(scope="module")
def fields(sections, gpu_device):
    three = (ModeFields(sections["three"][1], device=gpu_device), VelocityGramEmulation(sections["three"][1].p, sections["three"][1].t))
    square = (ModeFields(sections["square"][1], device=gpu_device), VelocityGramEmulation(sections["square"][1].p, sections["square"][1].t))
    out = {"three": three, "p5": three, "m3l": three, "square": square}
    yield out
    three[0].close()
    square[0].close()
    import torch
    torch.cuda.empty_cache()


def base_grams(mf, modes, geo):
    """The forms themselves under the names of profile_grams, for discs too."""
    if hasattr(geo, "index_profile"):
        return mf.profile_grams(modes, geo)
    G = mf.grams(modes, geo)
    ec, el = geo.n_core ** 2, geo.n_clad ** 2
    if "S" in G:
        return {"M": G["M_core"] + G["M_clad"], "M_w": ec * G["M_core"] + el * G["M_clad"], "S": G["S"]}
    return {"M": G["M_core"] + G["M_clad"], "M_w": G["M_core"] / ec + G["M_clad"] / el, "K_w": G["K_core"] / ec + G["K_clad"] / el,
            "D": G["D"]}


# ---- the kernels against the emulation -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 33, 70])
@pytest.mark.parametrize("name", ["three", "p5", "m3l", "square"])
def test_velocity_gram_kernels_match_emulation(sections, fields, name, k):
    """Per velocity and per output 1e-12 of max |reference|.  One exception, by the nature of the reference: under V = x
    the gradient forms cancel to rounding noise in the emulation as in the kernel (gt = 0 in exact arithmetic), so
    there both are held to 1e-12 of the form itself, the bound the scaling identity sets."""
    geo, mesh, (V, names, ring) = sections[name]
    mf, em = fields[name]
    for kind in KINDS:
        modes = _random_records(kind, mf, k, seed=300 + k)
        G = mf.velocity_grams(modes, geo, V)
        out, count = em.velocity_grams(_vals(modes), kind == "vectorial", geo, V)
        ref = em.named(out)
        forms = base_grams(mf, modes, geo)
        assert set(G) == set(ref) | {"count"} and G["count"].dtype == np.int64
        assert np.array_equal(G["count"], count), (G["count"], count)
        assert G["count"][names.index("bump")] == ring and G["count"][names.index("scaling")] == mesh.t.shape[1]
        for z in ("zero", "translation"):
            i = names.index(z)
            assert G["count"][i] == 0 and not any(G[nm][i].any() for nm in ref), z
        worst = 0.0
        for nm in ref:
            assert G[nm].shape == (len(names), k, k)
            for i, label in enumerate(names):
                if label in ("zero", "translation"):
                    continue
                if label == "scaling" and nm in GRADIENT_FORMS:
                    scale = np.abs(forms[nm[1:]]).max()
                    assert np.abs(G[nm][i]).max() <= 1e-12 * scale and np.abs(ref[nm][i]).max() <= 1e-12 * scale, nm
                    continue
                err = np.abs(G[nm][i] - ref[nm][i]).max() / np.abs(ref[nm][i]).max()
                worst = max(worst, err)
                assert err <= 1e-12, (nm, label, err)
        print(f"{name} {kind} k = {k}: worst column {worst:.2e} of its max |reference|")


# ---- identities with the existing kernels ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three", "p5", "m3l"])
def test_scaling_rotation_and_linearity_identities(sections, fields, name):
    geo, mesh, (V, names, _) = sections[name]
    mf, _ = fields[name]
    x = mesh.p.T.copy()
    rot = np.stack([-mesh.p[1], mesh.p[0]], axis=1)
    v1, v2 = V[names.index("random0")], V[names.index("random1")]
    a, b = 0.75, -1.5
    for kind in KINDS:
        modes = _random_records(kind, mf, 33, seed=9)
        F = base_grams(mf, modes, geo)
        G = mf.velocity_grams(modes, geo, np.stack([x, rot, v1, v2, a * v1 + b * v2]))
        close = lambda p, q, scale: np.abs(p - q).max() <= 1e-12 * np.abs(scale).max()
        assert close(G["dM"][0], 2.0 * F["M"], F["M"]) and close(G["dM_w"][0], 2.0 * F["M_w"], F["M_w"])
        for nm in GRADIENT_FORMS:
            if nm in G:
                assert np.abs(G[nm][0]).max() <= 1e-12 * np.abs(F[nm[1:]]).max(), nm
        if kind == "scalar":                                             # a rotation moves neither S nor M
            assert np.abs(G["dS"][1]).max() <= 1e-12 * np.abs(F["S"]).max()
            assert np.abs(G["dM"][1]).max() <= 1e-12 * np.abs(F["M"]).max()
        for nm in NAMES[2 if kind == "vectorial" else 1]:
            comb = a * G[nm][2] + b * G[nm][3]
            assert close(G[nm][4], comb, comb), nm


# ---- bits ------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(a[nm], b[nm]) for nm in a)


def test_repeats_batches_permutations_subsets_and_work_contents_give_the_same_symmetric_bits(sections, fields):
    import torch
    geo, mesh, (V, names, _) = sections["p5"]
    mf, _ = fields["p5"]
    k = 33
    for kind in KINDS:
        modes = _random_records(kind, mf, k, seed=7)
        G = mf.velocity_grams(modes, geo, V)
        assert _same(G, mf.velocity_grams(modes, geo, V))
        for nm in G:
            if nm != "count":
                assert np.array_equal(G[nm], G[nm].transpose(0, 2, 1)), nm
        # a velocity alone, and in a batch of another order (another group, another place in it)
        for i in (0, 7, 16, 20):
            alone = mf.velocity_grams(modes, geo, V[i])
            assert all(np.array_equal(alone[nm][0], G[nm][i]) for nm in alone), i
        back = mf.velocity_grams(modes, geo, V[::-1][:18])
        assert all(np.array_equal(back[nm], G[nm][::-1][:18]) for nm in back)
        perm = np.random.default_rng(k).permutation(k)
        P = mf.velocity_grams([modes[i] for i in perm], geo, V)
        assert _same(P, {nm: (v if nm == "count" else v[:, perm[:, None], perm[None, :]]) for nm, v in G.items()})
        S = mf.velocity_grams(modes[:20], geo, V)                        # one chunk instead of two
        assert _same(S, {nm: (v if nm == "count" else v[:, :20, :20]) for nm, v in G.items()})
        # a work buffer full of NaN and one full of zeros: everything that is read is written first
        _, vals, _ = mf._check_records(modes)
        staged, _src = mf._stage(vals)
        need = ctypes.c_int64(0)
        assert mf._lib.plfem_velocity_gram_work_bytes(mf._loc, vals.shape[0], k, len(names), ctypes.byref(need)) == _native.PLFEM_OK
        mat = mf._material(geo)
        for fill in (float("nan"), 0.0):
            work = torch.full(((need.value + 256 + 7) // 8,), fill, dtype=torch.float64, device=mf.tdev).view(torch.uint8)
            assert _same(G, mf._velocity_grams_staged(kind, staged, mat, V, work=work))


# ---- the C ABI on a live locator -------------------------------------------------------------------------------------
def test_velocity_argument_errors_on_a_live_locator(sections, fields):
    geo, mesh, (V, names, _) = sections["m3l"]
    mf, em = fields["m3l"]
    lib = _native.load_library()
    prof = geo.index_profile
    mf._ensure_locator()
    mf._set_index_map(prof.index_map)
    modes = _random_records("vectorial", mf, 3, seed=1)
    _, vals, _ = mf._check_records(modes)
    staged, _src = mf._stage(vals)
    table = prof.table()
    cores = np.ascontiguousarray(np.column_stack([POS, RAD]))
    vel = np.ascontiguousarray(V[[2, 15, 19]])
    nv, ne = mesh.p.shape[1], mesh.t.shape[1]
    need = ctypes.c_int64(0)
    size = lambda ncomp, k, nvel, out=need: lib.plfem_velocity_gram_work_bytes(mf._loc, ncomp, k, nvel,
                                                                               None if out is None else ctypes.byref(out))
    # the documented layout and its bound
    a = lambda b: (b + 255) // 256 * 256
    for ncomp, nout in ((1, 3), (2, 4)):
        for k, nvel in ((1, 1), (22, 35), (33, 16), (70, 256)):
            assert size(ncomp, k, nvel) == _native.PLFEM_OK
            nc = (k + 31) // 32
            g = max(1, min(16, nvel, (256 << 20) // (8 * nout * nc * nc * 128 * 1024)))
            assert g == min(nvel, 16 if k <= 64 else {1: 9, 2: 7}[ncomp])
            want = (a(8 * nvel * nout * k * k) + a(8 * g * nout * nc * nc * 128 * 1024) + a(16 * g * nv) + 2 * a(4 * g * ne) + a(128))
            assert need.value == want
    assert size(2, 70, 256) == _native.PLFEM_OK and need.value <= 512 << 20
    keep = ctypes.c_int64(-7)
    for bad in ((0, 3, 3), (3, 3, 3), (2, 0, 3), (2, 3, 0), (2, 3, 257)):
        assert size(*bad, out=keep) == _native.PLFEM_EINVAL and keep.value == -7, bad
    assert size(2, 3, 3, out=None) == _native.PLFEM_EINVAL
    assert lib.plfem_velocity_gram_work_bytes(None, 2, 3, 3, ctypes.byref(keep)) == _native.PLFEM_EINVAL and keep.value == -7
    assert size(2, 3, 3) == _native.PLFEM_OK
    work = _native.device_scratch(need.value + 512, mf.tdev)
    wp = (work.data_ptr() + 255) & ~255
    out = np.zeros((3, 4, 3, 3))
    count = np.full(3, -5, dtype=np.int64)
    ptr = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)

    def call(ncomp=2, k=3, modes_ptr=staged.data_ptr(), c=cores, ncore=3, ec=2.3, el=1.0, t=table, nlayer=2, bg=1.0, prof_=1, v=vel,
             nvel=3, w=wp, wb=None, res=out, cnt=count):
        return lib.plfem_velocity_grams(mf._loc, ncomp, k, ctypes.c_void_p(modes_ptr), 1, ptr(c), ncore, ec, el, ptr(t), nlayer, bg,
                                        prof_, ptr(v), nvel, ctypes.c_void_p(w), ctypes.c_int64(need.value if wb is None else wb),
                                        ptr(res), ptr(cnt))

    def with_entry(x, idx, val):
        y = x.copy()
        y[idx] = val
        return y

    # in the documented order: each call has one error of its class and one of the class checked next, and reports the first
    classes = [("ncomp must be", [dict(ncomp=0), dict(ncomp=3), dict(k=0)]),
               ("nvel must be", [dict(nvel=0), dict(nvel=257)]),
               ("ncore must be", [dict(ncore=65), dict(ncore=-1)]),
               ("null array", [dict(modes_ptr=0), dict(v=None), dict(w=0), dict(res=None), dict(cnt=None), dict(c=None)]),
               ("velocity entry must be finite", [dict(v=with_entry(vel, (1, 5, 0), np.nan)), dict(v=with_entry(vel, (2, nv - 1, 1), np.inf))]),
               (None, [dict(t=with_entry(table, (0, 3), -1.0)), dict(nlayer=65), dict(bg=0.0), dict(prof_=0, ec=np.nan),
                       dict(prof_=0, el=0.0), dict(prof_=0)]),
               ("smaller than plfem_velocity_gram_work_bytes", [dict(wb=need.value - 1)]),
               ("256-byte aligned", [dict(w=wp + 8)])]
    for i, (what, cases) in enumerate(classes):
        nxt = classes[i + 1] if i + 1 < len(classes) else (None, [{}])
        for kw in cases:
            assert call(**{**nxt[1][0], **kw}) == _native.PLFEM_EINVAL, kw
            msg = lib.plfem_locator_last_error(mf._loc)
            assert msg.startswith(b"plfem_velocity_grams: "), (kw, msg)
            assert (what.encode() in msg) if what else (nxt[0].encode() not in msg), (kw, msg)
    assert call(prof_=0, ec=np.nan) == _native.PLFEM_EINVAL and b"eps_core and eps_clad" in lib.plfem_locator_last_error(mf._loc)
    assert call(prof_=0) == _native.PLFEM_EINVAL and b"sampled index map" in lib.plfem_locator_last_error(mf._loc)
    assert lib.plfem_velocity_grams(None, 2, 3, ctypes.c_void_p(staged.data_ptr()), 1, ptr(cores), 3, 2.3, 1.0, ptr(table), 2, 1.0, 1,
                                    ptr(vel), 3, ctypes.c_void_p(wp), need, ptr(out), ptr(count)) == _native.PLFEM_EINVAL
    assert not out.any() and np.all(count == -5)
    assert call() == _native.PLFEM_OK and out.any()
    ref, cnt = em.velocity_grams(vals, True, geo, vel)
    assert np.array_equal(count, cnt)
    assert all(np.abs(out[v, o] - ref[v, o]).max() <= 1e-12 * np.abs(ref[v, o]).max() for v in range(3) for o in range(4))
    # the discs as material need the map cleared
    mf._set_index_map(None)
    assert call(prof_=0) == _native.PLFEM_OK


# ---- physics: central differences of GPU re-solves on the moved mesh -------------------------------------------------
T_STEP = 2.5e-4
MOTIONS = [(c, kd) for c in range(3) for kd in ("dx", "dy", "dr")]


def moved(core, kind, s):
    pos, rad = POS.copy(), RAD.copy()
    if kind == "dr":
        rad[core] += s
    else:
        pos[core, "xy".index(kind[1])] += s
    return PhotonicLanternGeometry(3, "triangular_3", pos, rad, 1.535, 1.0, wavelength=1.55)


@pytest.fixture(scope="module")
def solves(sections, gpu_device):
    """Both solvers on three_core() and on the eighteen moved meshes with the displaced / resized geometry."""
    g, mesh, (V, names, _) = sections["three"]
    out = {kind: {} for kind in KINDS}
    for key in [None] + MOTIONS:
        for s in ((0.0,) if key is None else (T_STEP, -T_STEP)):
            geo = g if key is None else moved(*key, s)
            m = mesh if key is None else TriMesh(mesh.p + s * V[names.index(key)].T, mesh.t)
            S = tpt.Solvers(geo, m, gpu_device)
            for kind in KINDS:
                out[kind].setdefault(key, []).append(S.solve(kind, geo))
            S.close()
    return out


def group_differences(kind, modes, label, values, resolves):
    """``[(group, mean of values, central difference of the mean mu)]`` over the groups of ``label`` (clusters and
    singletons), matched as tpt.group_means matches them: to a group of the same size of each re-solve -- the re-solve's
    own clusters under the same tolerance -- on whose span every member projects with norm above 0.999; the group that
    the end of a mode list may have cut is left out.  (group_means also drops a group whose gap to its neighbour moves by
    1 % in a re-solve: a radius step moves every mode of its core by that much, so that filter is not applied here.)"""
    X, mu = tpt._unit_rows(modes), tpt._mu(kind, modes)
    out = []
    for G in tpt._groups(label):
        if len(modes) - 1 in G:
            continue
        means = []
        for other in resolves:
            Y, muo = tpt._unit_rows(other), tpt._mu(kind, other)
            for H in tpt._groups(tpt._clusters(muo, 1e-6 * float(np.abs(muo).max()))):
                if len(H) == len(G) and len(other) - 1 not in H:
                    Q, _ = np.linalg.qr(Y[H].T)
                    if np.all(np.linalg.norm(X[G] @ Q, axis=1) > 0.999):
                        means.append(float(muo[H].mean()))
                        break
        if len(means) == 2:
            out.append((G, float(np.mean(values[G])), (means[0] - means[1]) / (2 * T_STEP)))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_core_position_and_radius_sensitivities_against_central_differences_of_gpu_solves(sections, fields, solves, kind):
    """Measured on an MI355X: see DESIGN.md section 31."""
    g, mesh, (V, names, _) = sections["three"]
    mf, _ = fields["three"]
    modes = solves[kind][None][0]
    res = shape_response(modes, mf, g, cluster_rtol=1e-6)
    assert res["labels"] == names[:15] and res["rayleigh_defect"].max() <= 1e-10
    assert res["dneff_dx"].shape == res["dneff_dr"].shape == res["dneff_de2s"].shape == (len(modes), 3)
    beta = np.array([m["beta"] for m in modes])
    to_mu = (1.0 if kind == "vectorial" else -1.0) * 2.0 * beta * g.k0
    tol = 1e-4 if kind == "vectorial" else 1e-5
    report = []
    for core, kd in MOTIONS:
        col = res["dneff_d" + kd[1]][:, core]
        assert np.array_equal(col, res["dneff_dp"][:, names.index((core, kd))])
        rows = group_differences(kind, modes, res["cluster"], col * to_mu, solves[kind][(core, kd)])
        big = max(abs(f) for _, _, f in rows)
        worst = max(abs(v - f) for _, v, f in rows) / big
        report.append((core, kd, len(rows), worst, big))
        print(f"{kind} core {core} {kd}: {len(rows)} groups, worst |HF - FD| = {worst:.2e} of max |d mu| = {big:.3g}")
    for core, kd, n, worst, big in report:
        assert n >= 3 and worst <= tol, (core, kd, worst)


@pytest.mark.parametrize("kind", KINDS)
def test_scaling_the_section_gives_the_group_index(sections, fields, solves, kind):
    g, mesh, _ = sections["three"]
    mf, _ = fields["three"]
    modes = solves[kind][None][0]
    disp = mode_dispersion(modes, mf, g, dn_dlambda=(0.0, 0.0))
    res = shape_response(modes, mf, g, velocities=mesh.p.T)
    assert res["labels"] == [0] and res["count"].tolist() == [mesh.t.shape[1]] and np.array_equal(res["cluster"], disp["cluster"])
    n_eff = np.array([m["beta"] for m in modes]) / g.k0
    err = np.abs(res["dneff_dp"][:, 0] - (disp["n_g"] - n_eff)).max()
    print(f"{kind}: |d n_eff / d scale - (n_g - n_eff)| max {err:.1e} (n_g - n_eff up to {np.abs(disp['n_g'] - n_eff).max():.3f})")
    assert err <= 1e-9
