// The P2 element on the device: the quadrature rule, the basis, the element map and the core test that every kernel
// integrating or evaluating on the mesh shares (k_element_matrices, k_count_core_qp, k_core_mask, k_sample_fields,
// k_field_overlap, k_mode_grams, k_profile_grams, k_mode_quartic, k_mode_project, k_mode_project_sampled, k_core_owner,
// k_mode_indicators, k_flux_grams, k_sample_efields, k_flux_overlap_posed, k_profile_point_weights, k_weighted_grams, k_map_point_keys,
// k_point_densities).  One definition, so that a quadrature point lands in the same region, and det J rounds
// the same way, in the assembly and in every kernel that must reproduce it.
#pragma once
#include <hip/hip_runtime.h>

#include "plan.h"   // MAX_CORES, LAYER_DOUBLES

namespace plfem {

namespace {

// 6-point degree-4 rule on the reference triangle (weights sum to 1/2) — scikit-fem's default
// intorder = 2*maxdeg = 4 for ElementTriP2.
__constant__ double c_qx[6] = {0.445948490915965, 0.10810301816807, 0.445948490915965,
                               0.091576213509771, 0.816847572980458, 0.091576213509771};
__constant__ double c_qy[6] = {0.445948490915965, 0.445948490915965, 0.10810301816807,
                               0.091576213509771, 0.091576213509771, 0.816847572980458};
__constant__ double c_qw[6] = {0.1116907948390055, 0.1116907948390055, 0.1116907948390055,
                               0.054975871827661, 0.054975871827661, 0.054975871827661};

// 16-point degree-8 rule on the reference triangle (Dunavant 1985; positive interior weights summing to 1/2), the digits
// polished to 20 places on the rule's moment equations: the products of four P2 fields of k_mode_quartic.  The centroid,
// three 3-point orbits (a, a), then the 6-point orbit of (0.00839..., 0.26311...).  The Python copy is
// pl_fem_vectoriel_amd/nonlinear.py (QUAD16_X / QUAD16_W).
__constant__ double c_q16x[16] = {
    0.33333333333333333333, 0.45929258829272315603, 0.45929258829272315603, 0.081414823414553687942,
    0.17056930775176020662, 0.17056930775176020662, 0.65886138449647958676, 0.050547228317030975458,
    0.050547228317030975458, 0.89890554336593804908, 0.0083947774099576053372, 0.0083947774099576053372,
    0.26311282963463811342, 0.26311282963463811342, 0.72849239295540428124, 0.72849239295540428124};
__constant__ double c_q16y[16] = {
    0.33333333333333333333, 0.45929258829272315603, 0.081414823414553687942, 0.45929258829272315603,
    0.17056930775176020662, 0.65886138449647958676, 0.17056930775176020662, 0.050547228317030975458,
    0.89890554336593804908, 0.050547228317030975458, 0.26311282963463811342, 0.72849239295540428124,
    0.0083947774099576053372, 0.72849239295540428124, 0.0083947774099576053372, 0.26311282963463811342};
__constant__ double c_q16w[16] = {
    0.072157803838893584126, 0.047545817133642312397, 0.047545817133642312397, 0.047545817133642312397,
    0.051608685267359125141, 0.051608685267359125141, 0.051608685267359125141, 0.016229248811599040155,
    0.016229248811599040155, 0.016229248811599040155, 0.013615157087217497132, 0.013615157087217497132,
    0.013615157087217497132, 0.013615157087217497132, 0.013615157087217497132, 0.013615157087217497132};

// IEEE product kept out of fused multiply-adds: hipcc's default -ffp-contract=fast ignores the contract pragma.  det J
// of a sliver element cancels to ~1e-8 of its terms, so its two products must round individually (as the reference's
// NumPy arithmetic does; a fused multiply-add changes 1e9-sized element entries at the 1e-8 relative level), and the
// locator's barycentric numerators must round as the host's do, so that a point on a vertex gets coordinates of exactly
// 0 / 1 and the emulation in tests/ reproduces every containment decision.
__device__ __forceinline__ double mul_rn(double a, double b) {
  double r;
  asm volatile("v_mul_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// P2 basis function i at (x, y) of the reference triangle: vertices 0-2, then the midpoints of edges 01, 12, 20
__device__ __forceinline__ double p2_phi(int i, double x, double y) {
  switch (i) {
    case 0: return 1 - 3 * x - 3 * y + 2 * x * x + 4 * x * y + 2 * y * y;
    case 1: return 2 * x * x - x;
    case 2: return 2 * y * y - y;
    case 3: return 4 * x - 4 * x * x - 4 * x * y;
    case 4: return 4 * x * y;
    default: return 4 * y - 4 * x * y - 4 * y * y;
  }
}

__device__ __forceinline__ void p2_phi(double x, double y, double phi[6]) {
#pragma unroll
  for (int i = 0; i < 6; ++i) phi[i] = p2_phi(i, x, y);
}

// physical gradients of the six basis functions at (xi, eta): J^-T grad_hat, inv = J^-1 row-major
__device__ __forceinline__ void p2_grad(const double inv[4], double xi, double eta, double gx[6], double gy[6]) {
  const double dxh[6] = {-3 + 4 * xi + 4 * eta, 4 * xi - 1, 0.0, 4 - 8 * xi - 4 * eta, 4 * eta, -4 * eta};
  const double dyh[6] = {-3 + 4 * xi + 4 * eta, 0.0, 4 * eta - 1, -4 * xi, 4 * xi, 4 - 4 * xi - 8 * eta};
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    gx[i] = inv[0] * dxh[i] + inv[2] * dyh[i];
    gy[i] = inv[1] * dxh[i] + inv[3] * dyh[i];
  }
}

// physical second derivatives of the P2 field with nodal values u: constant over the element.  The reference Hessians of
// the six basis functions are (4, 4, 0, -8, 0, 0) for xi xi, (4, 0, 4, 0, 0, -8) for eta eta and (4, 0, 0, -4, 4, -4) for
// xi eta; with d/dx = inv[0] d_xi + inv[2] d_eta and d/dy = inv[1] d_xi + inv[3] d_eta (p2_grad) they transform as below
__device__ __forceinline__ void p2_hess(const double inv[4], const double u[6], double& uxx, double& uxy, double& uyy) {
  const double h00 = 4.0 * (u[0] + u[1]) - 8.0 * u[3];
  const double h11 = 4.0 * (u[0] + u[2]) - 8.0 * u[5];
  const double h01 = 4.0 * (u[0] - u[3] + u[4] - u[5]);
  uxx = inv[0] * inv[0] * h00 + 2.0 * (inv[0] * inv[2]) * h01 + inv[2] * inv[2] * h11;
  uxy = inv[0] * inv[1] * h00 + (inv[0] * inv[3] + inv[2] * inv[1]) * h01 + inv[2] * inv[3] * h11;
  uyy = inv[1] * inv[1] * h00 + 2.0 * (inv[1] * inv[3]) * h01 + inv[3] * inv[3] * h11;
}

// physical second derivatives of the six basis functions themselves (constant over the element): the J^-1 products of
// p2_hess applied to the reference Hessians listed there, for the kernels that contract them with many DOF vectors
// (k_flux_grams, k_sample_efields, k_flux_overlap_posed)
__device__ __forceinline__ void p2_basis_hess(const double inv[4], double hxx[6], double hxy[6], double hyy[6]) {
  const double h00[6] = {4.0, 4.0, 0.0, -8.0, 0.0, 0.0};
  const double h11[6] = {4.0, 0.0, 4.0, 0.0, 0.0, -8.0};
  const double h01[6] = {4.0, 0.0, 0.0, -4.0, 4.0, -4.0};
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    hxx[i] = inv[0] * inv[0] * h00[i] + 2.0 * (inv[0] * inv[2]) * h01[i] + inv[2] * inv[2] * h11[i];
    hxy[i] = inv[0] * inv[1] * h00[i] + (inv[0] * inv[3] + inv[2] * inv[1]) * h01[i] + inv[2] * inv[3] * h11[i];
    hyy[i] = inv[1] * inv[1] * h00[i] + 2.0 * (inv[1] * inv[3]) * h01[i] + inv[3] * inv[3] * h11[i];
  }
}

// Affine map of element e: vertices = rows 0-2 of vrow ([3+][ne], sorted), coordinates x[v], y[v].  The type of ne is
// that of the row offsets (size_t or int).  det J is a call of its own: its opaque products are not dropped where unused.
struct P2Map {
  double x0, y0, j00, j01, j10, j11;   // J = [p1 - p0, p2 - p0]

  template <typename Int>
  __device__ __forceinline__ P2Map(const int32_t* vrow, Int ne, const double* x, const double* y, int e) {
    const int v0 = vrow[e], v1 = vrow[ne + e], v2 = vrow[2 * ne + e];
    x0 = x[v0];
    y0 = y[v0];
    j00 = x[v1] - x0;
    j10 = y[v1] - y0;
    j01 = x[v2] - x0;
    j11 = y[v2] - y0;
  }
  __device__ __forceinline__ double det() const { return mul_rn(j00, j11) - mul_rn(j01, j10); }
  // J^-1 = 1/det [[j11, -j01], [-j10, j00]]
  __device__ __forceinline__ void inverse(double det, double inv[4]) const {
    const double idet = 1.0 / det;
    inv[0] = j11 * idet; inv[1] = -j01 * idet; inv[2] = -j10 * idet; inv[3] = j00 * idet;
  }
  // the quadrature point in the reference's order, p0 + (J[r, 0] xi + J[r, 1] eta), every operation rounded on its own
  // (oracle P2Basis.qx): a point within an ulp of a core circle must land where the reference puts it
  __device__ __forceinline__ void point(double xi, double eta, double& X, double& Y) const {
    X = x0 + (mul_rn(j00, xi) + mul_rn(j01, eta));
    Y = y0 + (mul_rn(j10, xi) + mul_rn(j11, eta));
  }
};

// the core test: union of closed discs, cores[3 c .. 3 c + 2] = (x, y, r).  The reference's
// (x - cx)**2 + (y - cy)**2 <= r**2 (MCFGeometry.epsilon) with each square rounded on its own: a fused multiply-add
// would decide a point on the circle differently ("Core-boundary ties")
__device__ __forceinline__ bool in_any_core(double X, double Y, const double* cores, int ncore) {
  bool in = false;
  for (int c = 0; c < ncore; ++c) {
    const double dx = X - cores[3 * c], dy = Y - cores[3 * c + 1], r = cores[3 * c + 2];
    in |= (mul_rn(dx, dx) + mul_rn(dy, dy) <= mul_rn(r, r));
  }
  return in;
}

// which core: the highest index c whose closed disc holds the point, or -1 (the reference's epsilon writes the cores in
// order, so a later disc overwrites an earlier one).  The comparison is that of in_any_core, operation for operation:
// core_owner(...) >= 0 exactly where in_any_core(...), ties included
__device__ __forceinline__ int core_owner(double X, double Y, const double* cores, int ncore) {
  int owner = -1;
  for (int c = 0; c < ncore; ++c) {
    const double dx = X - cores[3 * c], dy = Y - cores[3 * c + 1], r = cores[3 * c + 2];
    if (mul_rn(dx, dx) + mul_rn(dy, dy) <= mul_rn(r, r)) owner = c;
  }
  return owner;
}

// Permittivity of an index profile at a point: eps_bg overwritten by every layer that holds the point, in table order
// (a later layer wins, as a later disc does above).  Layer l = layers[8 l .. 8 l + 7] = (cx, cy, r_in, r_out, eps_a,
// eps_b, g, 0): the point is in the layer when r_in^2 <= d2 <= r_out^2, the squared distance and the squares formed as
// in in_any_core, so a layer with r_in = 0 is that closed disc, ties included.  g = 0: the value is eps_a; g > 0: the
// alpha-profile eps_a + (eps_b - eps_a) t^g, t = (sqrt(d2) - r_in) / (r_out - r_in) clamped to [0, 1], the product
// rounded on its own (IndexProfile.epsilon of profile.py is this, operation for operation).  The table is read at
// indices every lane shares: uniform loads.
__device__ __forceinline__ double profile_eps(double X, double Y, const double* __restrict__ layers, int nlayer, double eps_bg) {
  double eps = eps_bg;
  for (int l = 0; l < nlayer; ++l) {
    const double* p = layers + LAYER_DOUBLES * l;
    const double dx = X - p[0], dy = Y - p[1], r_in = p[2], r_out = p[3];
    const double d2 = mul_rn(dx, dx) + mul_rn(dy, dy);
    if (mul_rn(r_in, r_in) <= d2 && d2 <= mul_rn(r_out, r_out)) {
      const double eps_a = p[4], g = p[6];
      if (g > 0.0) {
        const double t = fmin(fmax((sqrt(d2) - r_in) / (r_out - r_in), 0.0), 1.0);
        eps = eps_a + mul_rn(p[5] - eps_a, pow(t, g));
      } else {
        eps = eps_a;
      }
    }
  }
  return eps;
}

// A uniform node grid x_i = x0 + i dx, y_j = y0 + j dy of nx x ny samples (k_mode_project_sampled: fields; the map of an
// index profile below: permittivities).  inv_dx = fl(1 / dx) is formed once on the host.
struct SampledGrid {
  double x0, y0, inv_dx, inv_dy;
  int nx, ny;
};

// Cell (i0, j0) and weights (a, b) of the bilinear interpolant at (X, Y); false outside the closed extent (and for a NaN).
// tx = (X - x0) (1 / dx), the difference and the product each rounded on their own.
__device__ __forceinline__ bool sampled_cell(const SampledGrid& G, double X, double Y, int& i0, int& j0, double& a, double& b) {
  const double tx = mul_rn(X - G.x0, G.inv_dx), ty = mul_rn(Y - G.y0, G.inv_dy);
  if (!(tx >= 0.0 && tx <= (double)(G.nx - 1) && ty >= 0.0 && ty <= (double)(G.ny - 1))) return false;
  i0 = min((int)floor(tx), G.nx - 2);
  j0 = min((int)floor(ty), G.ny - 2);
  a = tx - (double)i0;
  b = ty - (double)j0;
  return true;
}

// The sampled map of an index profile (plfem_set_index_map, plfem_locator_set_index_map) as a kernel takes it: one
// pointer to the handle's map buffer (IndexMap of device.h), which holds the grid in its first MAP_HEADER doubles and
// behind it the permittivities E[j][i], row-major, nx ny <= 2^24 of them.  The grid is read where a point needs it
// (uniform loads), not carried in twelve scalar registers through a kernel that has none to spare.
struct EpsMap {
  const double* buf;
  __device__ __forceinline__ const SampledGrid& grid() const { return *reinterpret_cast<const SampledGrid*>(buf); }
  __device__ __forceinline__ const double* eps() const { return buf + MAP_HEADER; }
};
static_assert(sizeof(SampledGrid) <= MAP_HEADER * sizeof(double), "the grid fits the map buffer's header");

// The profile over a map: inside the closed extent of the grid the background is the bilinear interpolant of E -- the
// cell of sampled_cell, the interpolation order of k_mode_project_sampled (along x in both rows, then along y), every
// product through mul_rn so that no fused multiply-add decides a value -- and eps_bg outside it; the layers are painted
// over that as above (IndexProfile.epsilon of profile.py, operation for operation).  The four corners are ordinary
// vector loads at i0 <= nx - 2, j0 <= ny - 2: inside the map for every point, NaN included (outside: nothing is read).
__device__ __forceinline__ double profile_eps(double X, double Y, const double* __restrict__ layers, int nlayer, double eps_bg,
                                              const EpsMap& map) {
  int i0, j0;
  double a, b;
  const SampledGrid G = map.grid();
  if (sampled_cell(G, X, Y, i0, j0, a, b)) {
    const double* p = map.eps() + ((int64_t)j0 * G.nx + i0);
    const double e00 = p[0], e01 = p[1], e10 = p[G.nx], e11 = p[G.nx + 1];
    const double a1 = 1.0 - a, b1 = 1.0 - b;
    const double lo = mul_rn(a1, e00) + mul_rn(a, e01), hi = mul_rn(a1, e10) + mul_rn(a, e11);
    eps_bg = mul_rn(lo, b1) + mul_rn(hi, b);
  }
  return profile_eps(X, Y, layers, nlayer, eps_bg);
}

// Where a point lies in the layer table, in one walk (k_profile_point_weights): the topmost layer that holds it -- the
// membership test of profile_eps, operation for operation -- or -1, and tg = t^g of that layer when it is graded (0
// otherwise), t as profile_eps forms it.  profile_eps evaluates every graded layer it meets; the last one it meets is this
// one, so layer_value(eps_a, eps_b, tg) of the returned layer has the bits of profile_eps.
__device__ __forceinline__ int profile_top_layer(double X, double Y, const double* __restrict__ layers, int nlayer, double& tg) {
  int top = -1;
  double d2_top = 0.0;
  for (int l = 0; l < nlayer; ++l) {
    const double* p = layers + LAYER_DOUBLES * l;
    const double dx = X - p[0], dy = Y - p[1], r_in = p[2], r_out = p[3];
    const double d2 = mul_rn(dx, dx) + mul_rn(dy, dy);
    if (mul_rn(r_in, r_in) <= d2 && d2 <= mul_rn(r_out, r_out)) {
      top = l;
      d2_top = d2;
    }
  }
  tg = 0.0;
  if (top >= 0) {
    const double* p = layers + LAYER_DOUBLES * top;
    const double r_in = p[2], r_out = p[3], g = p[6];
    if (g > 0.0) tg = pow(fmin(fmax((sqrt(d2_top) - r_in) / (r_out - r_in), 0.0), 1.0), g);
  }
  return top;
}

// value of a layer at a point with tg = t^g: v_a for a constant layer (g = 0), v_a + (v_b - v_a) t^g for a graded one,
// the product rounded on its own -- for the permittivities of the table this is profile_eps, for a tangent's (d_a, d_b)
// the first-order change of it
__device__ __forceinline__ double layer_value(double v_a, double v_b, double g, double tg) {
  return g > 0.0 ? v_a + mul_rn(v_b - v_a, tg) : v_a;
}

// the bilinear interpolant of a map E[ny][nx] in the cell (i0, j0) with the weights (a, b) of sampled_cell: the order and
// the roundings of profile_eps over a map
__device__ __forceinline__ double map_bilinear(const double* __restrict__ E, int nx, int i0, int j0, double a, double b) {
  const double* p = E + ((int64_t)j0 * nx + i0);
  const double e00 = p[0], e01 = p[1], e10 = p[nx], e11 = p[nx + 1];
  const double a1 = 1.0 - a, b1 = 1.0 - b;
  const double lo = mul_rn(a1, e00) + mul_rn(a, e01), hi = mul_rn(a1, e10) + mul_rn(a, e11);
  return mul_rn(lo, b1) + mul_rn(hi, b);
}

}  // namespace
}  // namespace plfem
