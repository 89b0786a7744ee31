"""NumPy emulation of the tangent Gram call (plfem_profile_tangent_grams: k_profile_point_weights + k_weighted_grams +
k_overlap_reduce) for the tests.

Built on ``ProfileGramEmulation``: the same features at the six-point rule and the same material weight ``w`` (1 / eps for
vectorial records, eps for scalar ones, ``IndexProfile.epsilon`` at ``P2Basis.qx``).  A column's point weight is what the
pre-pass writes: ``-(d eps w) w`` or ``d eps`` with ``d eps = ProfileTangent.epsilon`` at the same points, and ``w X``,
``w Y`` for the two moment columns.  As the kernel does, the unweighted M- and K-form products of a point are formed once
and scaled by the column's weight.
"""
from __future__ import annotations

import copy

import numpy as np

from profile_gram_emulation import ProfileGramEmulation

NAMES = {2: ("M", "K"), 1: ("M",)}


class TangentGramEmulation(ProfileGramEmulation):
    def column_weights(self, profile, tangents, ncomp, moments=False, origin=(0.0, 0.0)):
        """(ncol, ne, 6): the point weights of every column, tangents first, then ``w X``, ``w Y``."""
        qx, qy = self.basis.qx
        w = self.profile_weight(profile, ncomp)
        cols = []
        for t in tangents:
            d = t.epsilon(qx, qy)
            cols.append(-(d * w) * w if ncomp == 2 else d)
        if moments:
            cols += [w * (qx - origin[0]), w * (qy - origin[1])]
        return np.stack(cols) if cols else np.zeros((0,) + qx.shape)

    def tangent_grams(self, vals, indexed, profile, tangents, moments=False, origin=(0.0, 0.0)):
        """(ncol, nout, k, k): out_host of plfem_profile_tangent_grams."""
        ncomp, k = vals.shape[0], vals.shape[1]
        C = self.column_weights(profile, tangents, ncomp, moments, origin) * self.basis.dx[None]
        C = C.reshape(C.shape[0], -1)

        def g(X, Y):
            """(ncol, k, k): sum over the points of c X_m Y_n."""
            X, Y = X.reshape(k, -1), Y.reshape(k, -1)
            return np.einsum("cq,mq,nq->cmn", C, X, Y, optimize=True)

        F = self.features(vals, indexed)
        if ncomp == 1:
            (u, _, _), = F
            return g(u, u)[:, None]
        (hx, hxx, hxy), (hy, hyx, hyy) = F                             # hxy = d hx / dy, hyx = d hy / dx
        return np.stack([g(hx, hx) + g(hy, hy), g(hxy, hxy) + g(hyx, hyx) - g(hxx, hyy) - g(hyy, hxx)], axis=1)

    def named(self, out, ntan, moments):
        """``out`` under the names of ModeFields.profile_tangent_grams."""
        names = NAMES[out.shape[1]]
        res = {nm + "_d": out[:ntan, i] for i, nm in enumerate(names)}
        if moments:
            for i, nm in enumerate(names):
                res[nm + "_wX"], res[nm + "_wY"] = out[ntan, i], out[ntan + 1, i]
        return res


def moved_profile(profile, tangent=None, s=1.0, eps_of=None):
    """A copy of ``profile`` -- same layers, same grid -- with other VALUES: ``eps + s d_eps`` of ``tangent``, entered as the
    index ``n' = sqrt(eps + s d_eps)`` that a user would give (so each value is ``n' * n'``), or ``eps_of(eps, d_eps)`` taken
    as it is when ``eps_of`` is given."""
    q = copy.deepcopy(profile)

    def new(eps, d):
        eps, d = np.asarray(eps, dtype=np.float64), np.asarray(d, dtype=np.float64)
        if eps_of is not None:
            return eps_of(eps, d)
        n = np.sqrt(eps + s * d)
        return n * n

    q.eps_background = float(new(profile.eps_background, tangent.d_eps_background))
    q.n_background = float(np.sqrt(q.eps_background))
    q._layers = [(cx, cy, r_in, r_out, float(new(ea, da)), float(new(eb, db)), g, z)
                 for (cx, cy, r_in, r_out, ea, eb, g, z), (da, db) in zip(profile._layers, tangent.d_layers)]
    q._indices = [q.n_background] + [float(np.sqrt(v)) for row in q._layers for v in row[4:6]]
    if profile.index_map is not None:
        E, *grid = profile.index_map
        E2 = np.ascontiguousarray(new(E, tangent.d_map if tangent.d_map is not None else tangent.d_eps_background))
        q._map = (E2, *grid)
    return q


def random_tangent(profile, seed, scale=0.1, with_map=True):
    """A tangent of ``profile`` with random values of size ``scale``: distinct per layer, centre != edge on a graded one,
    and a random map when the profile has one."""
    rng = np.random.default_rng(seed)
    t = profile.table()
    d = scale * rng.uniform(0.3, 1.0, (len(profile), 2)) * rng.choice([-1.0, 1.0], (len(profile), 1))
    d[t[:, 6] == 0, 1] = d[t[:, 6] == 0, 0]
    d_map = None
    if with_map and profile.index_map is not None:
        d_map = scale * rng.uniform(-1.0, 1.0, profile.index_map[0].shape)
    return profile.tangent_eps(scale * rng.uniform(0.3, 1.0), d, d_map)
