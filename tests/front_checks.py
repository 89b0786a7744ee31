"""The rules by which a GPU factorisation / solve is held against the NumPy emulation of the same front tree
(front_emulation.py) and against SuperLU, shared by test_gpu_operator_forms.py and test_gpu_pivot_replacement.py (and by
the host tests that let a deliberately wrong emulation play the device)."""
import numpy as np

FACTOR_TOL = 1e-8       # per front, relative to the largest entry of the block (test_fronts_match_numpy_emulation)
# ... or this many times the double-precision emulation's own error, where that is larger: on the ill-conditioned fronts
# of the sliver mesh (c1_h10) the GPU's factor, built from explicit inverses of the pivot blocks, is 10-12 times further
# from the extended-precision reference than the sequential elimination (the solve's backward error: 9.3 times)
FACTOR_RATIO = 30.0
BERR_FLOOR = 1e-14
FWD_TOL = 1e-9


def backward_error(K, x, b):
    """Componentwise backward error max|K x - b| / max(|K| |x| + |b|)."""
    return float(np.abs(K @ x - b).max() / (abs(K) @ np.abs(x) + np.abs(b)).max())


def front_errors(got, dbl, xp):
    """(error of got, error of dbl) against xp, both relative to the largest entry of xp."""
    xp = xp.astype(np.float64)
    scale = max(np.abs(xp).max(), 1e-300)
    return np.abs(got - xp).max() / scale, np.abs(dbl - xp).max() / scale


def front_check(got, dbl, xp, what):
    """A block of the GPU's factor against the extended-precision emulation: within FACTOR_TOL of the block's largest
    entry, or within FACTOR_RATIO times the error of the double-precision emulation (ill-conditioned fronts).  Returns
    (error, the emulation's error)."""
    if not got.size:
        return 0.0, 0.0
    err, ref = front_errors(got, dbl, xp)
    assert err <= max(FACTOR_TOL, FACTOR_RATIO * ref), (what, err, ref)
    return err, ref


def owned_dofs(T, f, N):
    """Global DOFs owned by front f (component-major vectors of length dpn N)."""
    nodes = T.nodes(f)[:int(T.fs[f])]
    nodes = nodes[nodes >= 0]
    return np.concatenate([c * N + nodes for c in range(T.dpn)])


def shallowest_owner(T, N):
    """The shallowest front that owns DOFs: lowest level, then lowest index (heap order is level order).  The root,
    unless the first cut of the dissection runs through a gap of the mesh and owns nothing."""
    return next(f for f in range(T.nf) if owned_dofs(T, f, N).size)


def right_hand_sides(T, idx, N):
    """The four right-hand sides of a case (full length dpn N, zero outside the unknowns idx): two random ones, one
    supported on the owned DOFs of one leaf, one ("root") on the topmost separator that owns DOFs."""
    n2 = T.dpn * N
    rng = np.random.default_rng(7)
    out = {}
    for name in ("random", "random2"):
        b = np.zeros(n2)
        b[idx] = rng.standard_normal(len(idx))
        out[name] = b
    # supported on the owned DOFs of one leaf (the one with the most) only: travels up through every level
    leaves = range(T.leaf0, T.nf)
    leaf = max(leaves, key=lambda f: int(T.fs[f]))
    b = np.zeros(n2)
    d = owned_dofs(T, leaf, N)
    b[d] = rng.standard_normal(len(d))
    out["leaf"] = b
    # supported on the topmost separator only (the root of every tree whose root owns DOFs): travels down through every
    # level below it
    b = np.zeros(n2)
    d = owned_dofs(T, shallowest_owner(T, N), N)
    b[d] = rng.standard_normal(len(d))
    out["root"] = b
    assert all(np.count_nonzero(v) for v in out.values())
    return out


def check_tree_invariants(sym):
    """The front tree of an analysis is a valid elimination structure: every unknown node is owned by exactly one front
    (a Dirichlet node by none), the boundary nodes of a front are owned by proper ancestors, the root has no boundary,
    front sizes are multiples of 8, and every element sits in one leaf with all its unknown nodes in that front.  Every
    front, boundary node and element is checked.  Returns the FrontTree."""
    import front_emulation as fe
    T = fe.FrontTree(sym)
    owner = sym.array("owner")
    bmask = sym.array("bmask").astype(bool)
    assert (owner[bmask] == -1).all() and (owner[~bmask] >= 0).all()
    seen = np.zeros(sym.N, dtype=int)
    for f in range(T.nf):
        fn = T.nodes(f)
        own = fn[:T.fs[f]]
        own = own[own >= 0]
        assert (owner[own] == f).all()
        seen[own] += 1
        bnd = fn[T.fs[f]:]
        bnd = bnd[bnd >= 0]
        for v in bnd:
            a = owner[v]
            g = f
            while g > a:
                g = (g - 1) // 2
            assert g == a and a != f, (f, v, a)
        assert T.fs[f] % 8 == 0 and T.fb[f] % 8 == 0
    assert (seen[~bmask] == 1).all() and (seen[bmask] == 0).all()
    assert T.fb[0] == 0                                            # the root has no boundary
    epos = T.epos
    edof = sym.array("edof").reshape(6, -1)
    leaf = sym.array("leaf_of_elem")
    count = np.zeros(sym.ne, dtype=int)
    np.add.at(count, T.lel, 1)
    assert (count == 1).all()                                      # every element in exactly one leaf's list
    for e in range(sym.ne):
        fn = T.nodes(T.leaf0 + leaf[e])
        for a in range(6):
            if bmask[edof[a, e]]:
                assert epos[a, e] == -1
            else:
                assert fn[epos[a, e]] == edof[a, e]
    return T
