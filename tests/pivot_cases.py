"""The cases of the static-pivot replacement tests: element matrices written so that chosen node pairs of chosen fronts
arrive at their elimination step with exactly the 2 x 2 block E = [[a, b], [b, c]] the case wants (kernels_front.hip,
pair_step / ldl_pivot_block; restated in front_emulation.ldl_partial).  Shared by the host tests
(test_pivot_replacement_host.py) and the GPU tests (test_gpu_pivot_replacement.py).

Construction.  The device assembles the leaf fronts from the element matrices it holds (k_leaf_assemble reads d_elem),
and the emulation takes the same K_e: the base is the oracle's physical K_e = A_e - sigma B_e of the tree's pencil at
its usual shift, symmetrised and rounded to float64, written into the AXX / AXY / AYX / AYY slots (AXX alone for the
scalar pencil) with zeros in MINV and factored at sigma = 0 -- `v - 0 * 0`, so the numbers reach the front as written.
  * A DECOUPLED plant zeroes the rows and columns of the pair's DOFs in every K_e that holds them and writes E into one
    element.  Whatever was eliminated before the pair, its Schur update of the pair is 0 * x: the pair meets its step
    with E itself, the largest entry of its own rows is max|E|, and its D^-1 has a closed form.
  * A COUPLED plant keeps the couplings of the pair to its neighbours (see coupled_fire / coupled_sliver below).
A pair is the two DOFs (Hx, Hy) of one node (vectorial pencil) or two neighbouring nodes of the front (scalar pencil;
E's off-diagonal entry needs an element that holds both, which the positions below were chosen for -- printed first)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

import front_emulation as fe
import operator_cases as oc

DELTA_TOL = 1e-15       # D^-1 of a decoupled plant against its closed form: rep rounded once, fast_rcp's ~1 ulp, one product
#                         -- at most four roundings, 4.4e-16


@dataclass(frozen=True)
class Tree:
    name: str
    mesh: tuple
    leaf: int
    dpn: int
    positions: tuple        # (label, front, k): the pair of local DOFs k, k + 1 of that front
    pad_pair: tuple         # (front, k) of a (true DOF, padding DOF) pair (scalar pencil, odd number of owned nodes) or ()
    fire: tuple             # (front, k): first pair of a leaf front whose rows couple to later nodes of its block
    sliver: tuple           # ((front, k) of the healthy small pair, (front, k) of the huge one): the same pivot block
    reaches: str

    @property
    def case(self):
        return oc.Case(self.name, self.mesh, self.leaf, self.dpn, True, self.reaches)


# Block step j of a front is the pivot block of local DOFs 32 j .. 32 j + 31.  Step 0 of a level is factorised by
# k_ldl_first_panel straight from the front; step j + 1 by ldl_column_block inside k_ldl_update<j & 1> of step j, from
# the LDS tile it has just updated.
TREES = (
    Tree("sq6_one_vec", ("square", 6), 10 ** 6, 2,
         (("first", 0, 0), ("middle of block 0", 0, 14), ("last of block 0", 0, 30), ("block 1", 0, 32),
          ("block 2", 0, 80), ("last owned node, block 7", 0, 240)), (), (0, 0), ((0, 14), (0, 30)),
         "one front, s2 = 256: first panel, then seven steps of k_ldl_update, both parities"),
    Tree("sq6_one_sca", ("square", 6), 10 ** 6, 1,
         (("first", 0, 0), ("middle of block 0", 0, 14), ("last of block 0", 0, 30), ("block 1", 0, 32),
          ("block 2", 0, 78), ("partial block 5", 0, 160)), (0, 168), (0, 0), ((0, 14), (0, 30)),
         "one front, s2 = 176: five full blocks and a partial one of 16; (true DOF, padding) pair"),
    Tree("sq10_l16_vec", ("square", 10), 16, 2,
         (("first of a leaf", 15, 0), ("last owned of a leaf", 18, 26), ("level 2, block 0", 3, 10),
          ("level 2, partial block 1", 3, 32), ("level 1", 1, 4), ("root, block 0", 0, 0),
          ("root, partial block 1", 0, 36)), (), (15, 0), ((3, 10), (3, 4)),
         "31 fronts on 5 levels: gathered fronts, a second (partial) block step above the leaves"),
    Tree("sq16_l32_sca", ("square", 16), 32, 1,
         (("first of a leaf", 15, 0), ("leaf, block 1", 20, 40), ("level 3", 7, 2), ("level 1", 1, 2),
          ("root, block 0", 0, 6)), (0, 32), (15, 0), ((20, 40), (20, 46)),
         "scalar, 31 fronts on 5 levels: leaves of two full blocks, root with a partial block and a padding pair"),
)

KINDS = ("a", "d2", "det")


def block_of(kind, sign):
    """E = [[a, b], [b, c]] of a decoupled plant, the site it must fire at (None: a control) and the sign of the replaced
    value.  Magnitudes: the replaced value lies between 30 ulp of max|E| and a tenth of the threshold 1e-13 max|E|, so
    rounding moves neither the branch nor the sign."""
    if kind == "a":             # first scalar pivot: b = 0 -> scalar order, |a| = 1e-14 < thr = 1e-13
        return (sign * 1e-14, 0.0, 1.0), "a", sign
    if kind == "d2":            # a = 2, g = 1.5, d2 = c - 4.5 = +-4.5 2^-46 = +-6.4e-14 exactly; thr = 4.5e-13
        return (2.0, 3.0, 4.5 * (1.0 + sign * 2.0 ** -46)), "d2", sign
    if kind == "det":           # a = 0 -> the 2 x 2 form; det = -b^2 = -1e-18 against thr s = 1e-13.  A determinant that
        #                         reaches the 2 x 2 form is negative (b^2 |det| > a^2 s^2 rules out a c > b^2): the sign
        #                         of the case is that of b and c
        return (0.0, sign * 1e-9, sign * 1.0), "det", -1
    if kind == "ctl_2x2":       # healthy 2 x 2 pivot with a = 0
        return (0.0, 1.0, 1.0), None, 0
    if kind == "ctl_diag":      # small against the rest of the front, healthy against its own rows
        return (1e-4, 0.0, 1e-4), None, 0
    raise ValueError(kind)


@dataclass(frozen=True)
class Plant:
    front: int
    k: int
    kind: str
    sign: int = 1
    pad: bool = False       # the pair's second DOF is a padding DOF (unit diagonal): only E[0, 0] is written


@dataclass(frozen=True)
class Case:
    name: str
    plants: tuple = ()
    coupled: str = ""       # "", "fire" or "sliver"
    solves: bool = False    # run the solve checks on this case


def cases_of(tree):
    pos = tree.positions
    out = [Case("unplanted", solves=True)]
    for kind in KINDS:
        for sign in (1, -1):
            pl = [Plant(f, k, kind, sign) for _, f, k in pos]
            if tree.pad_pair and kind == "a":
                pl.append(Plant(*tree.pad_pair, "a", sign, pad=True))
            out.append(Case(f"{kind}{'+' if sign > 0 else '-'}", tuple(pl)))
    for name, first, solves in (("controls", 0, True), ("controls_swapped", 1, False)):       # every position gets both controls
        out.append(Case(name, tuple(Plant(f, k, ("ctl_2x2", "ctl_diag")[(i + first) & 1]) for i, (_, f, k) in enumerate(pos)),
                        solves=solves))
    out.append(Case("coupled_fire", coupled="fire", solves=True))
    out.append(Case("coupled_sliver", coupled="sliver", solves=True))
    # every site and sign at once, in several fronts and levels, for the count
    combos = [(kind, sign) for kind in KINDS for sign in (1, -1)]
    pl = [Plant(f, k, *combos[(i + 1) % 6]) for i, (_, f, k) in enumerate(pos)]
    if tree.pad_pair:
        pl.append(Plant(*tree.pad_pair, "a", -1, pad=True))
    out.append(Case("all_at_once", tuple(pl), solves=True))
    return tuple(out)


CASE_IDS = [f"{t.name}:{c.name}" for t in TREES for c in cases_of(t)]


def find(case_id):
    tname, cname = case_id.split(":")
    tree = next(t for t in TREES if t.name == tname)
    return tree, next(c for c in cases_of(tree) if c.name == cname)


class TreeData:
    """Mesh, analysis, front tree, base element matrices and unknowns of a tree (host only)."""

    def __init__(self, tree, geometry):
        from oracle import hfield, scalar
        from oracle.p2 import MeshTriLite, P2Basis
        from pl_fem_vectoriel_amd.solver_fem import shift_estimate
        self.tree, self.g = tree, geometry
        self.mesh = oc.mesh_of(tree.case, geometry)
        self.sym = oc.symbolic_of(tree.case, self.mesh)
        self.T = fe.FrontTree(self.sym)
        self.N, self.dpn = self.sym.N, tree.dpn
        self.edof = self.sym.array("edof").reshape(6, -1)
        basis = P2Basis(MeshTriLite(self.mesh.p, self.mesh.t))
        if self.dpn == 2:
            self.sigma = shift_estimate(geometry)
            Ke = fe.element_K(hfield.element_matrices(geometry, basis), geometry.k0 ** 2, self.sigma)
            interior = self.sym.array("interior")
            self.idx = np.concatenate([interior, interior + self.N])
        else:
            self.sigma = scalar.shift(geometry)
            Ke = fe.element_K_scalar(scalar.element_matrices(geometry, basis), geometry.k0 ** 2, self.sigma)
            self.idx = np.arange(self.N)
        self.Ke0 = np.ascontiguousarray(0.5 * (Ke + np.transpose(Ke, (0, 2, 1))), dtype=np.float64)

    # -- where a pair lives ---------------------------------------------------------------------------------------
    def pair_nodes(self, f, k):
        """Global nodes of local DOFs k, k + 1 of front f (the same node twice for the vectorial pencil; -1: padding)."""
        fn = self.T.nodes(f)
        return int(fn[k // self.dpn]), int(fn[(k + 1) // self.dpn])

    def slots(self, node):
        """(element, local node) of every element that holds the node."""
        a, e = np.nonzero(self.edof == node)
        order = np.argsort(e, kind="stable")
        return [(int(e[i]), int(a[i])) for i in order]

    def pair_slots(self, f, k):
        """(element, local DOFs of k, local DOFs of k + 1) for one element that holds the whole pair, or None."""
        n1, n2 = self.pair_nodes(f, k)
        if self.dpn == 2:
            e, a = self.slots(n1)[0]
            return e, 2 * a, 2 * a + 1
        s1, s2 = dict(self.slots(n1)), dict(self.slots(n2))
        both = sorted(set(s1) & set(s2))
        return (both[0], s1[both[0]], s2[both[0]]) if both else None

    def decouple(self, Ke, node):
        d = np.arange(self.dpn)
        for e, a in self.slots(node):
            Ke[e][self.dpn * a + d, :] = 0.0
            Ke[e][:, self.dpn * a + d] = 0.0

    # -- the element matrices of a case ---------------------------------------------------------------------------
    def elements(self, case):
        """(K_e of the case, expected replacements [(front, pair, site, sign of the replaced value, rmax or None)])."""
        Ke = self.Ke0.copy()
        expect = []
        for p in case.plants:
            (a, b, c), site, sgn = block_of(p.kind, p.sign)
            n1, n2 = self.pair_nodes(p.front, p.k)
            assert n1 >= 0 and (p.pad or n2 >= 0) and (not p.pad or n2 < 0), (p, n1, n2)
            self.decouple(Ke, n1)
            if p.pad:
                e, l1 = self.slots(n1)[0]
                Ke[e][l1, l1] = a
                c = 1.0
            else:
                self.decouple(Ke, n2)
                e, l1, l2 = self.pair_slots(p.front, p.k)
                Ke[e][l1, l1], Ke[e][l2, l2] = a, c
                Ke[e][l1, l2] = Ke[e][l2, l1] = b
            if site:
                expect.append((p.front, p.k // 2, site, sgn, max(abs(a), abs(b), abs(c))))
        if case.coupled == "fire":
            expect.append(self._coupled_fire(Ke))
        elif case.coupled == "sliver":
            self._coupled_sliver(Ke)
        return Ke, sorted(expect)

    def _zero_entry(self, Ke, n1, n2):
        """K[n1's first DOF, n2's last DOF] and its mirror image to zero in every element (n1 = n2, dpn 2: the node's Hx-Hy
        coupling; dpn 1: the coupling of two nodes; n2 None: the diagonal entry of n1's first DOF)."""
        dp = self.dpn
        for e, a1 in self.slots(n1):
            if n2 is None:
                Ke[e][dp * a1, dp * a1] = 0.0
                continue
            for e2, a2 in self.slots(n2):
                if e2 == e:
                    Ke[e][dp * a1, dp * a2 + dp - 1] = Ke[e][dp * a2 + dp - 1, dp * a1] = 0.0

    def _coupled_fire(self, Ke):
        """(i) The first pair of a leaf front (nothing is eliminated before it: E is the assembled K_pp) with b = 0, its
        couplings to every other node kept, and a pivot of 1e-14 of the largest coupling its rows have inside the pivot
        block: vanishing against its OWN rows, it must be replaced -- by 1e-8 of that coupling, multipliers of 1e8, the
        situation one refinement pass is there for."""
        f, k = self.tree.fire
        assert f >= self.T.leaf0 and k == 0
        n1, n2 = self.pair_nodes(f, k)
        self._zero_entry(Ke, n1, None)
        self._zero_entry(Ke, n1, n2)
        Fm = fe.assemble_front(self.T, f, Ke, None)
        nbk = min(fe.NB, self.T.s2(f))
        rmax = float(np.abs(Fm[k:k + 2, :nbk]).max())
        rows = float(np.abs(Fm[k, 2:nbk]).max())
        assert rows > 0.05 * rmax, (rows, rmax)         # row k itself couples to a later node of the block at that order
        a = 1e-14 * rmax
        e, l1 = self.slots(n1)[0]
        Ke[e][self.dpn * l1, self.dpn * l1] = a
        return (f, 0, "a", 1, rmax)

    def _coupled_sliver(self, Ke):
        """(ii) The sliver situation: a healthy pair whose own rows are of order 1e-4 (3e-5) with entries of 2e9 elsewhere in
        the same pivot block.  Judged against the whole block (thr 2e-4) it would be replaced; against its own rows it
        is not."""
        (f1, k1), (f2, k2) = self.tree.sliver
        assert f1 == f2 and k1 // fe.NB == k2 // fe.NB
        for (f, k), v in (((f1, k1), 3e-5), ((f2, k2), 2e9)):
            n1, n2 = self.pair_nodes(f, k)
            self.decouple(Ke, n1)
            self.decouple(Ke, n2)
            e, l1, l2 = self.pair_slots(f, k)
            Ke[e][l1, l1] = Ke[e][l2, l2] = v

    def device_elements(self, Ke):
        """K_e in the layout of the device's element store, [ne][8][6][6]: A slots filled, MINV (and the rest) zero."""
        el = np.zeros((self.sym.ne, 8, 6, 6))
        if self.dpn == 2:
            el[:, 0], el[:, 1], el[:, 2], el[:, 3] = Ke[:, 0::2, 0::2], Ke[:, 0::2, 1::2], Ke[:, 1::2, 0::2], Ke[:, 1::2, 1::2]
        else:
            el[:, 0] = Ke
        return el

    def matrix(self, Ke):
        """The assembled K of the unknowns (CSR) from the element matrices."""
        dp, N = self.dpn, self.N
        gd = (np.arange(dp)[None, :, None] * N + self.edof.T[:, None, :]).transpose(0, 2, 1).reshape(-1, 6 * dp)   # [ne][6 dp]: node-major, component inside
        rows = np.broadcast_to(gd[:, :, None], Ke.shape).ravel()
        cols = np.broadcast_to(gd[:, None, :], Ke.shape).ravel()
        K = sp.coo_matrix((Ke.ravel(), (rows, cols)), shape=(dp * N, dp * N)).tocsr()
        return K[self.idx][:, self.idx].tocsr()


class Reference:
    """A case emulated in float64 and in extended precision: factors, D^-1, pivot kinds, replacement logs."""

    def __init__(self, data, case, mistake=None):
        self.data, self.case = data, case
        self.Ke, self.expect = data.elements(case)
        T = data.T
        self.logs, self.logx, self.kinds = {}, {}, {}
        self.Fs, self.Ds = fe.factor(T, self.Ke, None, self.logs, mistake)
        if mistake is None:
            self.Fx, self.Dx = fe.factor(T, self.Ke.astype(np.longdouble), self.kinds, self.logx)

    @staticmethod
    def flat(logs):
        """[(front, pair, site, sign, rmax)] of a factorisation's logs, sorted."""
        return sorted((f, q, site, -1 if v < 0 else 1, float(rm)) for f, lg in logs.items() for q, site, v, rm in lg)

    @property
    def count(self):
        return sum(len(v) for v in self.logs.values())

    def plant_rows(self):
        """(plant, front, k, D^-1 rows k, k + 1 of the extended-precision emulation) of every decoupled plant."""
        return [(p, p.front, p.k, self.Dx[p.front][p.k:p.k + 2]) for p in self.case.plants]


def delta_error(got, ref):
    """Largest relative error of the 2 x 2 entries of D^-1 rows `got` against the extended-precision `ref`; an entry that
    is zero in ref (the off-diagonal entry of scalar pivots, a / det with a = 0) must be exactly zero: inf otherwise."""
    worst = 0.0
    for g, r in zip(np.asarray(got, dtype=np.longdouble).ravel(), np.asarray(ref).ravel()):
        if r == 0:
            worst = max(worst, 0.0 if g == 0 else np.inf)
        else:
            worst = max(worst, float(abs(g - r) / abs(r)))
    return worst


def closed_form(kind, sign, pad=False):
    """D^-1 rows (diagonal, off-diagonal) of a decoupled plant in extended precision, from the rule itself."""
    x = np.longdouble
    (a, b, c), site, sgn = block_of(kind, sign)
    a, b, c = x(a), x(b), x(1.0 if pad else c)
    rmax = max(abs(a), abs(b), abs(c))
    rep = x(1e-8) * rmax
    if site == "a":
        return np.array([[1 / (sgn * rep), 0], [1 / c, 0]], dtype=x)
    if site == "d2":
        return np.array([[1 / a, 0], [1 / (sgn * rep), 0]], dtype=x)
    if site == "det":
        dt = sgn * rep * rmax
    else:
        dt = a * c - b * b
        if b == 0:
            return np.array([[1 / a, 0], [1 / c, 0]], dtype=x)
    return np.array([[c / dt, -b / dt], [a / dt, -b / dt]], dtype=x)


_trees, _refs = {}, {}


def tree_data(name, geometry):
    """(cached: the geometry is the suite's one C1 geometry)"""
    if name not in _trees:
        _trees[name] = TreeData(next(t for t in TREES if t.name == name), geometry)
    return _trees[name]


def reference(case_id, geometry):
    if case_id not in _refs:
        tree, case = find(case_id)
        _refs[case_id] = Reference(tree_data(tree.name, geometry), case)
    return _refs[case_id]


# ---- what the GPU tests assert about the count and the decoupled plants, as functions of "what the device returned": the
# host tests hand them a deliberately wrong emulation in the device's place ---------------------------------------------
def device_findings(ref, count, delta_of):
    """Failures of a device result against the reference of a case: [(what, margin)], margin = how many times its
    tolerance an error is (inf for a wrong count, a wrong pivot kind or a nonzero where an exact zero belongs).
    count: the device's pivot_perturbations; delta_of(front): its D^-1 of that front, [s2][2]."""
    out = []
    if count != ref.count:
        out.append((("count", count, ref.count), np.inf))
    for p, f, k, rows in ref.plant_rows():
        got = np.asarray(delta_of(f))[k:k + 2]
        if bool(got[0, 1] != 0.0) != ref.kinds[f][k // 2][0]:
            out.append((("kind", p), np.inf))
        err = delta_error(got, rows)
        if err > DELTA_TOL:
            out.append((("delta", p, err), err / DELTA_TOL))
    return out
