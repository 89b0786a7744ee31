"""NumPy emulation of the posed overlap (k_field_overlap_posed) for the tests, built on ``fields_emulation.Emulation``:
mesh B's quadrature points are taken into mesh A's frame with the kernel's arithmetic (every product rounded on its
own, an IEEE division), sampled there by brute-force location, turned by the rotation for two-component values, and
contracted with B's own values times the weights.  Also the helpers the tests share: the two small meshes, a mesh and a
record set moved by a pose on the host, quadratic records and their closed-form posed overlap."""
from __future__ import annotations

import numpy as np

from fields_emulation import Emulation

IDENTITY = (0.0, 0.0, 1.0, 0.0, 1.0)
COVERING = (0.1, -0.2, float(np.cos(0.3)), float(np.sin(0.3)), 1.2)      # the posed A covers B
HALF_OUT = (2.0, 0.1, float(np.cos(0.2)), float(np.sin(0.2)), 1.0)       # about half of B's points fall outside A
EXP = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2))                     # monomials 1, x, y, x^2, xy, y^2


def to_a_frame(pts, pose):
    """B's points (2, n) in A's frame: R^T (x - t) / m, operation by operation as the kernel."""
    tx, ty, c, s, m = (np.float64(v) for v in pose)
    dx, dy = pts[0] - tx, pts[1] - ty
    return np.vstack([(c * dx + s * dy) / m, (c * dy - s * dx) / m])


def rotate(vals, pose):
    """Two-component values (2, ...) turned by the pose's rotation; one-component values as they are."""
    if vals.shape[0] == 1:
        return vals
    c, s = np.float64(pose[2]), np.float64(pose[3])
    return np.stack([c * vals[0] - s * vals[1], s * vals[0] + c * vals[1]])


def posed_overlap(em_a: Emulation, vals_a, em_b: Emulation, vals_b, indexed, pose, weight=None):
    """(O (ka, kb), element of A per quadrature point of B) under one pose."""
    qx, w = em_b.quadrature(weight)
    ua, elem = em_a.sample(vals_a, to_a_frame(qx, pose), indexed)
    ua = rotate(ua, pose)
    ub = em_b.own_values(vals_b, indexed)
    return sum(ua[c] @ (ub[c] * w[None]).T for c in range(vals_a.shape[0])), elem


def small_meshes():
    """Mesh A: unit_square_mesh(5) mapped to [-2, 2]^2; mesh B: unit_square_mesh(4) mapped to [-0.5, 0.5]^2; interior
    vertices moved by up to 0.03 (seeded).  300 and 192 quadrature points."""
    from pl_fem_vectoriel_amd.mesh import TriMesh, unit_square_mesh
    out = []
    for n, half, seed in ((5, 2.0, 11), (4, 0.5, 12)):
        sq = unit_square_mesh(n)
        inner = (sq.p[0] > 0) & (sq.p[0] < 1) & (sq.p[1] > 0) & (sq.p[1] < 1)
        p = (2.0 * sq.p - 1.0) * half
        p[:, inner] += np.random.default_rng(seed).uniform(-0.03, 0.03, (2, int(inner.sum())))
        out.append(TriMesh(p, sq.t.copy()))
    return out


def moved_mesh(mesh, pose):
    """The mesh with every vertex at t + m R p: the posed mesh A in B's frame."""
    from pl_fem_vectoriel_amd.mesh import TriMesh
    tx, ty, c, s, m = pose
    p = np.vstack([tx + m * (c * mesh.p[0] - s * mesh.p[1]), ty + m * (s * mesh.p[0] + c * mesh.p[1])])
    return TriMesh(p, mesh.t.copy())


def records(rng, kind, nrows, k):
    if kind == "vectorial":
        return [{"Ex_dofs": rng.standard_normal(nrows), "Ey_dofs": rng.standard_normal(nrows)} for _ in range(k)]
    return [{"field_vector": rng.standard_normal(nrows)} for _ in range(k)]


def vals(modes):
    if "Ex_dofs" in modes[0]:
        return np.stack([np.array([m["Ex_dofs"] for m in modes]), np.array([m["Ey_dofs"] for m in modes])])
    return np.array([m["field_vector"] for m in modes])[None]


def moved_records(modes, pose):
    """The records as they stand on the moved mesh: the DOF values of a vectorial record turned by the rotation."""
    if "Ex_dofs" not in modes[0]:
        return modes
    c, s = pose[2], pose[3]
    return [{"Ex_dofs": c * m["Ex_dofs"] - s * m["Ey_dofs"], "Ey_dofs": s * m["Ex_dofs"] + c * m["Ey_dofs"]} for m in modes]


def monomials(x, y):
    return np.array([x ** a * y ** b for a, b in EXP])


def quadratic_records(em: Emulation, C):
    """Scalar records interpolating the quadratics sum_e C[i, e] monomial_e at the mesh's DOF locations."""
    dl = em.basis.doflocs
    return [{"field_vector": f} for f in C @ monomials(dl[0], dl[1])]


def closed_form(Ca, Cb, pose, box=(-0.5, 0.5, -0.5, 0.5)):
    """integral over the box of f_a(R^T (x - t) / m) f_b(x): a 6 x 6 Gauss-Legendre rule, exact for the degree-4
    integrand."""
    g, w = np.polynomial.legendre.leggauss(6)
    x = 0.5 * (box[0] + box[1]) + 0.5 * (box[1] - box[0]) * g
    y = 0.5 * (box[2] + box[3]) + 0.5 * (box[3] - box[2]) * g
    X, Y = (v.ravel() for v in np.meshgrid(x, y))
    W = np.outer(w, w).ravel() * 0.25 * (box[1] - box[0]) * (box[3] - box[2])
    xa = to_a_frame(np.vstack([X, Y]), pose)
    return (Ca @ monomials(xa[0], xa[1])) @ ((Cb @ monomials(X, Y)) * W[None]).T
