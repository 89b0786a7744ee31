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


def right_hand_sides(T, idx, N):
    """The four right-hand sides of a case (full length dpn N, zero outside the unknowns idx): two random ones, one
    supported on the owned DOFs of one leaf, one on the root separator."""
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
    # supported on the root separator only: travels down through every level
    b = np.zeros(n2)
    d = owned_dofs(T, 0, N)
    b[d] = rng.standard_normal(len(d))
    out["root"] = b
    assert all(np.count_nonzero(v) for v in out.values())
    return out
