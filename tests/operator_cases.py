"""The case matrix of the shift-invert operator tests: meshes / leaf sizes / pencils chosen so that, between them, every
kernel form the launch plan can pick (plan.h: forward row forms, tile form, mixed launch; backward row forms, leaf tile
form) runs at a leaf and at an inner level, for the vectorial (2 unknowns per node) and the scalar (1) pencil; and meshes
with a hole, a gap, a pinch, teeth or graded sizes (topology_cases.py), whose trees have an empty root, fronts without
boundary and a root of one real node.  Shared
by the host test of the coverage (test_operator_cases_host.py) and the GPU tests (test_gpu_operator_forms.py)."""
from __future__ import annotations

from dataclasses import dataclass

import front_emulation as fe


@dataclass(frozen=True)
class Case:
    name: str
    mesh: tuple            # ("c1", refinement, levels) of generate_mesh on the C1 geometry, ("square", n), or ("topo", name)
                           # of topology_cases.py
    leaf: int              # leaf_elems of the analysis (0: the default)
    dpn: int               # unknowns per node: 2 vectorial, 1 scalar
    factor: bool           # compare every front of the factorisation with the emulation
    reaches: str           # what the case is in the matrix for

    @property
    def id(self):
        return self.name


CASES = (
    Case("c1_h05_l24_vec", ("c1", 0.5, 0), 24, 2, True, "baseline; s2 = 0 fronts; tile forms"),
    Case("c1_h05_l24_sca", ("c1", 0.5, 0), 24, 1, True, "scalar baseline; s2 = 0 fronts"),
    Case("c1_h10_vec", ("c1", 1.0, 0), 0, 2, True, "inner-level mixed launch; slivers"),
    Case("c1_h10_sca", ("c1", 1.0, 0), 0, 1, True, "scalar, default leaf size"),
    Case("c1_h10_l150_vec", ("c1", 1.0, 0), 150, 2, False, "leaf-level mixed launch"),
    Case("c1_h10_l300_sca", ("c1", 1.0, 0), 300, 1, False, "scalar leaf-level mixed launch"),
    Case("c1_h20_l150_sca", ("c1", 2.0, 0), 150, 1, False, "scalar inner-level mixed launch"),
    Case("c1_h05_l400_vec", ("c1", 0.5, 0), 400, 2, False, "leaf-level k_fwd_rows<P,2,4> (16 leaves)"),
    Case("c1_h05_l400_sca", ("c1", 0.5, 0), 400, 1, False, "scalar leaf-level k_fwd_rows<P,2,4>"),
    Case("c1_h05_l8_vec", ("c1", 0.5, 0), 8, 2, True, "levels of >= 1024 fronts (panel cap 1); 116 s2 = 0 fronts"),
    Case("c1_h05_l8_sca", ("c1", 0.5, 0), 8, 1, True, "scalar, levels of >= 1024 fronts"),
    Case("sq12_one_vec", ("square", 12), 10 ** 6, 2, True, "one front: leaf = root"),
    Case("sq12_one_sca", ("square", 12), 10 ** 6, 1, True, "scalar, one front"),
    Case("sq20_l100_vec", ("square", 20), 100, 2, False, "8 leaves: leaf-level k_fwd_rows<P,1,4> within the P = 4 budget"),
) + tuple(
    # meshes with holes, gaps and pinches (topology_cases.py; the facts in topology_cases.EXPECT): a few hundred nodes each
    Case(f"{name}_l{leaf}_{'vec' if dpn == 2 else 'sca'}", ("topo", name), leaf, dpn, True, reaches)
    for name, leaf, dpns, reaches in (
        ("islands", 24, (2, 1), "empty root (m = 0), level 0 with max_s2 = 0, two fronts without boundary"),
        ("islands", 4, (2, 1), "the same in a tree of seven levels"),
        ("bowtie", 24, (2, 1), "vectorial: empty root through a pinch; scalar: a root that owns one real node"),
        ("comb", 4, (2, 1), "20 inner fronts without owned DOFs (republished boundaries); empty leaves"),
        ("annulus", 4, (2,), "a separator cut by the hole; 3 empty inner fronts, 6 empty leaves"),
        ("strip1", 4, (2,), "every vertex Dirichlet: all unknowns on edge midpoints"),
        ("graded", 24, (2,), "element areas spread by marked bisection"),
        ("tiny2", 0, (2, 1), "vectorial: two unknowns in a front padded to 16"))
    for dpn in dpns)
TOPOLOGY_CASES = tuple(c for c in CASES if c.mesh[0] == "topo")
# the north-star size (N = 90 639), solve checks against splu only
FULL_SIZE = Case("c1_full_vec", ("c1", 1.0, 1), 0, 2, False, "full size")


def mesh_of(case, geometry):
    from pl_fem_vectoriel_amd.mesh import generate_mesh, unit_square_mesh
    if case.mesh[0] == "c1":
        return generate_mesh(geometry, case.mesh[1], case.mesh[2])
    if case.mesh[0] == "topo":
        import topology_cases
        return topology_cases.trimesh(case.mesh[1])
    return unit_square_mesh(case.mesh[1])


def symbolic_of(case, mesh):
    from pl_fem_vectoriel_amd import _native
    return _native.Symbolic(mesh.p, mesh.t, leaf_elems=case.leaf, dofs_per_node=case.dpn, dirichlet=case.dpn == 2)


def host_pencil(sym, mesh, geometry, dpn, element_matrices=True):
    """The oracle's pencil of a mesh, as the GPU tests and the host tests of the emulation use it: (K = A - sigma B on the
    unknowns, idx = the unknowns in full-length component-major vectors, sigma, A, B, element matrices of K for
    front_emulation.factor)."""
    import numpy as np
    from oracle import hfield, scalar
    from oracle.p2 import MeshTriLite, P2Basis
    from pl_fem_vectoriel_amd.solver_fem import shift_estimate
    g, N = geometry, sym.N
    om = MeshTriLite(mesh.p, mesh.t)
    if dpn == 2:
        sigma = shift_estimate(g)
        A, B, _, _, _, _, _ = hfield.assemble_hfield_system_fused(g, om, eliminate_zeros=False)
        basis = P2Basis(om)
        A, B, interior = hfield.restrict_interior(A, B, basis)
        idx = np.concatenate([interior, interior + N])
        Ke = fe.element_K(hfield.element_matrices(g, basis), g.k0 ** 2, sigma) if element_matrices else None
    else:
        sigma = scalar.shift(g)
        K, M, Me, basis = scalar.assemble(g, om, eliminate_zeros=False)
        A, B = (K - g.k0 ** 2 * Me).tocsr(), M.tocsr()
        idx = np.arange(N)
        Ke = fe.element_K_scalar(scalar.element_matrices(g, basis), g.k0 ** 2, sigma) if element_matrices else None
    return (A - sigma * B).tocsr(), idx, sigma, A.tocsr(), B.tocsr(), Ke


def forms_reached(forms, dpn):
    """(direction, kernel, "leaf" | "inner", dpn) of every launch of a tree with these level_forms records."""
    out = set()
    for r in forms:
        where = "leaf" if r["leaf"] else "inner"
        out.add(("fwd", r["fwd"], where, dpn))
        out.add(("bwd", r["bwd"], where, dpn))
    return out


def forms_possible():
    """Every (direction, kernel, level kind, dpn) the rules of plan.h can produce: levels of 2^l fronts, leaf or not, with
    or without a front of more than MIX_BIG_S2 owned DOFs."""
    out = set()
    for lev in range(16):
        count = 1 << lev
        for leaf in (False, True):
            for big in (False, True):
                fr, br = fe.fwd_block_rows(count), fe.bwd_block_rows(count, leaf)
                fwd = {8: "k_fwd_rows<P,1,4>", 16: "k_fwd_rows<P,2,4>"}.get(fr, "k_fwd_mix" if big else "k_fwd")
                bwd = {8: "k_bwd_rows<P,1,4>", 16: "k_bwd_rows<P,2,4>"}.get(br, "k_bwd")
                where = "leaf" if leaf else "inner"
                for dpn in (1, 2):
                    out.add(("fwd", fwd, where, dpn))
                    out.add(("bwd", bwd, where, dpn))
    return out
