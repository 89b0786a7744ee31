// gfx950 kernels and C-ABI of the mode-field calls (include/plfem.h, "Mode fields at arbitrary points"): the point
// locator bound to a device, P2 evaluation of many modes at many points (k_sample_fields) and the overlap integral of
// two mode sets living on two meshes (k_field_overlap + k_overlap_reduce), alone or under a table of poses of one mesh
// relative to the other (k_field_overlap_posed + k_overlap_reduce), and the same-mesh Grams of a mode set under
// the assembly's element forms, split by material region (k_mode_grams + k_overlap_reduce), and the quartic overlap of
// products of four modes on a 16-point degree-8 rule (k_mode_quartic + k_quartic_reduce), and the projection of a mode
// set on a family of analytic fields that separate in x and y -- plane waves and Gaussian beams -- on the same rule
// (k_mode_project + k_project_reduce) and on a batch of sampled complex fields, images on a pixel grid interpolated
// bilinearly (k_mode_project_sampled + k_project_sampled_reduce), and the Grams of a mode set restricted to each core disc (k_core_owner,
// k_core_count + k_core_fill, k_core_grams + k_overlap_reduce), and the region Grams weighted by the coordinates of the
// quadrature point (k_moment_grams + k_overlap_reduce), and the Grams under the permittivity of an index profile
// (k_profile_grams + k_overlap_reduce), and the per-element a-posteriori error indicators of a mode set: element residual
// plus flux jumps across the edges (k_mode_indicators), and the electric field and axial Poynting flux of vectorial modes
// at points (k_sample_efields) with the Grams their cross powers are built from (k_flux_grams + k_overlap_reduce), and the
// E x H cross flux of two vectorial mode sets on two meshes under a table of poses (k_flux_overlap_posed + k_overlap_reduce),
// and the first-order change of the Grams when the mesh moves with a vertex velocity field and carries its material along
// (k_velocity_flag, k_velocity_count + k_velocity_fill, k_velocity_grams + k_overlap_reduce + k_velocity_symmetrise),
// and the derivative of the profile Grams' diagonal in every pixel of a sampled map (k_map_point_keys, the sort of
// sort_pairs.h, k_map_cell_ranges, k_point_densities, k_map_gather).
//
// Replaces, on the user's side, scikit-fem's Basis.probes / Basis.interpolate on the reference's P2 basis
// (reference solver_fem.py:126): the reference itself turns no mode vector back into a field, so the Grams, the
// quartic overlap and the projection have no counterpart there.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>

#include "device.h"
#include "p2_element.h"
#include "sort_pairs.h"

struct plfem_locator {
  const plfem::Symbolic* S = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  int nv = 0, ne = 0, N = 0, nsolve = 0;
  double x0 = 0, y0 = 0, inv_hx = 0, inv_hy = 0;
  int nx = 0, ny = 0;
  int32_t *d_cell_ptr = nullptr, *d_cell_elems = nullptr, *d_edof = nullptr, *d_int_index = nullptr;
  double* d_pxy = nullptr;                     // [2][nv] vertex coordinates
  double* d_layers = nullptr;                  // [64][8] layer table of the profile of the call in flight (plfem_profile_grams)
  plfem::IndexMap map;                         // the sampled map under the layers (plfem_locator_set_index_map)
};

namespace plfem {
namespace {

struct LocArgs {
  double x0, y0, inv_hx, inv_hy;
  int nx, ny, nv, ne;
  const int32_t* cell_ptr;
  const int32_t* cell_elems;
  const double* pxy;
  const int32_t* edof;      // [6][ne]; rows 0-2 = the sorted vertices
  const int32_t* map;       // DOF -> row of the staged modes (int_index) or nullptr = identity
};

struct CoreTable {
  double c[MAX_CORES * 3];
};

// The material of the electric-field kernels (k_sample_efields, k_flux_grams), one of three instances: PROFILE false: eps_core
// in the closed discs of `cores` and eps_clad outside; PROFILE true: the index profile (layers, nlayer, eps_bg), plain or
// over a sampled map (Map... = one EpsMap).  The discs are also the region split of k_flux_grams, whatever the instance.
struct Material {
  CoreTable cores;
  int ncore;
  double eps_core, eps_clad;
  const double* layers;
  int nlayer;
  double eps_bg;
};

// permittivity at a point, by the helpers the assembly uses; in_core: in_any_core of the point (read by the disc instance only)
template <bool PROFILE, typename... Map>
__device__ __forceinline__ double material_eps(const Material& mat, double X, double Y, bool in_core, Map... map) {
  if constexpr (PROFILE) return profile_eps(X, Y, mat.layers, mat.nlayer, mat.eps_bg, map...);
  else return in_core ? mat.eps_core : mat.eps_clad;
}

EpsMap eps_map(const IndexMap& m) { return {m.d}; }

LocArgs loc_args(const plfem_locator* L, bool indexed) {
  return {L->x0, L->y0, L->inv_hx, L->inv_hy, L->nx, L->ny, L->nv, L->ne, L->d_cell_ptr, L->d_cell_elems, L->d_pxy,
          L->d_edof, indexed ? L->d_int_index : nullptr};
}

// cell index: the formula of locator.cpp (cell_of), so a point inside an element's bounding box lands in a listed cell
__device__ __forceinline__ int dev_cell(double v, double v0, double inv_h, int n) {
  const double f = floor((v - v0) * inv_h);
  if (!(f >= 0.0)) return 0;
  return f >= (double)(n - 1) ? n - 1 : (int)f;
}

// Smallest element id among the point's cell candidates that contain it (the lists are ascending, so that is the first
// hit), with the reference coordinates (xi, eta) and the inverse Jacobian.  Containment: every barycentric coordinate
// >= -(PLFEM_LOC_TOL + its rounding bound s), s = PLFEM_LOC_EPS4 (|j11| (|x| + |x0|) + |j01| (|y| + |y0|)) / |det J| for xi
// (the same form for eta, s_xi + s_eta for 1 - xi - eta): what the rounding of the point's and the vertex's own
// coordinates can move the coordinate by.  On a sliver (det J ~ 1e-8 of its edge products) that exceeds 1e-10.  A
// coordinate within its bound of 0 is set to 0 exactly: the point is then evaluated ON that edge, through the
// well-conditioned coordinate along it, instead of through the sliver's ill-conditioned width.
__device__ int dev_locate(const LocArgs& L, double x, double y, double& xi, double& eta, double inv[4]) {
  const int ix = dev_cell(x, L.x0, L.inv_hx, L.nx), iy = dev_cell(y, L.y0, L.inv_hy, L.ny);
  const int cell = iy * L.nx + ix;
  const int q1 = L.cell_ptr[cell + 1];
  const double* px = L.pxy;
  const double* py = L.pxy + L.nv;
  for (int q = L.cell_ptr[cell]; q < q1; ++q) {
    const int e = L.cell_elems[q];
    const P2Map M(L.edof, L.ne, px, py, e);
    const double ax = M.x0, ay = M.y0, j00 = M.j00, j10 = M.j10, j01 = M.j01, j11 = M.j11;
    const double det = M.det();
    const double dx = x - ax, dy = y - ay;
    double a = (mul_rn(j11, dx) - mul_rn(j01, dy)) / det, b = (mul_rn(j00, dy) - mul_rn(j10, dx)) / det;
    const double mx = fabs(x) + fabs(ax), my = fabs(y) + fabs(ay);
    const double sa = PLFEM_LOC_EPS4 * (mul_rn(fabs(j11), mx) + mul_rn(fabs(j01), my)) / fabs(det);
    const double sb = PLFEM_LOC_EPS4 * (mul_rn(fabs(j00), my) + mul_rn(fabs(j10), mx)) / fabs(det);
    const double c = 1.0 - a - b;
    if (a >= -(PLFEM_LOC_TOL + sa) && b >= -(PLFEM_LOC_TOL + sb) && c >= -(PLFEM_LOC_TOL + sa + sb)) {   // (NaN: never)
      const bool za = fabs(a) <= sa, zb = fabs(b) <= sb;
      if (za) a = 0.0;
      if (zb) b = 0.0;
      if (fabs(c) <= sa + sb) {               // on the edge opposite vertex 0: a + b = 1
        if (zb) a = 1.0;
        else if (za) b = 1.0;
        else if (sa >= sb) a = 1.0 - b;
        else b = 1.0 - a;
      }
      xi = a;
      eta = b;
      M.inverse(det, inv);
      return e;
    }
  }
  return -1;
}

// staged row of DOF d of element e, -1 = contributes nothing (boundary DOF of an interior-indexed record)
__device__ __forceinline__ int dev_row(const LocArgs& L, int e, int a) {
  const int d = L.edof[a * L.ne + e];
  return L.map ? L.map[d] : d;
}

// offsets of the six DOFs of element e into one component of the staged modes ([nrows][k]), -1 = contributes nothing
__device__ __forceinline__ void dev_row_offsets(const LocArgs& L, int e, int k, int64_t row[6]) {
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const int r = dev_row(L, e, a);
    row[a] = r < 0 ? -1 : (int64_t)r * k;
  }
}

// One lane per point.  Modes staged DOF-major ([comp][nrows][k]): the six gathers of a point are six contiguous runs of k
// doubles, read one mode per iteration; the output is [comp][k][npts], so a wave's stores of one mode are coalesced.
__global__ __launch_bounds__(256) void k_sample_fields(LocArgs L, int ncomp, int k, int64_t nrows, const double* __restrict__ V,
                                                       const double* __restrict__ beta, int npts, const double* __restrict__ pts,
                                                       double* __restrict__ out, int32_t* __restrict__ elem) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npts) return;
  double xi = 0, eta = 0, inv[4] = {0, 0, 0, 0};
  const int e = dev_locate(L, pts[p], pts[(int64_t)npts + p], xi, eta, inv);
  elem[p] = e;
  const int64_t plane = (int64_t)k * npts;
  const int nout = ncomp + (ncomp == 2 && beta != nullptr);
  if (e < 0) {
    for (int c = 0; c < nout; ++c)
      for (int m = 0; m < k; ++m) out[c * plane + (int64_t)m * npts + p] = 0.0;
    return;
  }
  double phi[6], gx[6], gy[6];
  p2_phi(xi, eta, phi);
  p2_grad(inv, xi, eta, gx, gy);
  int64_t row[6];
  dev_row_offsets(L, e, k, row);
  const double* V1 = V + nrows * k;
  for (int m = 0; m < k; ++m) {
    double u0 = 0.0, u1 = 0.0, dv = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      if (row[a] < 0) continue;
      const double v0 = V[row[a] + m];
      u0 += phi[a] * v0;
      if (ncomp == 2) {
        const double v1 = V1[row[a] + m];
        u1 += phi[a] * v1;
        dv += gx[a] * v0 + gy[a] * v1;
      }
    }
    out[(int64_t)m * npts + p] = u0;
    if (ncomp == 2) {
      out[plane + (int64_t)m * npts + p] = u1;
      if (beta) out[2 * plane + (int64_t)m * npts + p] = -dv / beta[m];
    }
  }
}

// Electric field and axial Poynting flux of vectorial modes at points (plfem_sample_efields).  One lane per point, located
// as in k_sample_fields (dev_locate: the same scan and tie rule).  Fields vary as exp(j (w t - beta z)), H = (hx, hy,
// j hz_im); from curl H = j w eps0 eps E with e = E / Z0 and w = 1 / eps at the point itself,
//   gx = -(hx,xx + hy,xy),  gy = -(hx,xy + hy,yy)     (constant over the element)
//   Ex = w (beta hy + gy / beta) / k0,  Ey = -w (beta hx + gx / beta) / k0,  Ez_im = -w (dx hy - dy hx) / k0,
//   Sz = (Ex hy - Ey hx) / 2,
// evaluated per mode in this order.  Output [4][k][npts] = Ex, Ey, Ez_im, Sz, a wave's stores of one mode coalesced;
// eps_out[npts] (optional) the permittivity used.  A point in no element: element -1, every output and eps 0.
template <bool PROFILE, typename... Map>
__global__ __launch_bounds__(256) void k_sample_efields(LocArgs L, int k, int64_t nrows, const double* __restrict__ V,
                                                        const double* __restrict__ beta, double k0, Material mat, int npts,
                                                        const double* __restrict__ pts, double* __restrict__ out,
                                                        double* __restrict__ eps_out, int32_t* __restrict__ elem, Map... map) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npts) return;
  const double X = pts[p], Y = pts[(int64_t)npts + p];
  double xi = 0, eta = 0, inv[4] = {0, 0, 0, 0};
  const int e = dev_locate(L, X, Y, xi, eta, inv);
  elem[p] = e;
  const int64_t plane = (int64_t)k * npts;
  if (e < 0) {
    for (int c = 0; c < 4; ++c)
      for (int m = 0; m < k; ++m) out[c * plane + (int64_t)m * npts + p] = 0.0;
    if (eps_out) eps_out[p] = 0.0;
    return;
  }
  const double eps = material_eps<PROFILE>(mat, X, Y, PROFILE ? false : in_any_core(X, Y, mat.cores.c, mat.ncore), map...);
  if (eps_out) eps_out[p] = eps;
  const double w = 1.0 / eps;
  double phi[6], gx[6], gy[6], hxx[6], hxy[6], hyy[6];
  p2_phi(xi, eta, phi);
  p2_grad(inv, xi, eta, gx, gy);
  p2_basis_hess(inv, hxx, hxy, hyy);
  int64_t row[6];
  dev_row_offsets(L, e, k, row);
  const double* V1 = V + nrows * k;
  for (int m = 0; m < k; ++m) {
    double hx = 0.0, hy = 0.0, dxhy = 0.0, dyhx = 0.0, sx = 0.0, sy = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      if (row[a] < 0) continue;
      const double vx = V[row[a] + m], vy = V1[row[a] + m];
      hx += phi[a] * vx;
      hy += phi[a] * vy;
      dxhy += gx[a] * vy;
      dyhx += gy[a] * vx;
      sx += hxx[a] * vx + hxy[a] * vy;
      sy += hxy[a] * vx + hyy[a] * vy;
    }
    const double b = beta[m];
    const double ex = w * (b * hy - sy / b) / k0;       // gy = -sy
    const double ey = -w * (b * hx - sx / b) / k0;      // gx = -sx
    out[(int64_t)m * npts + p] = ex;
    out[plane + (int64_t)m * npts + p] = ey;
    out[2 * plane + (int64_t)m * npts + p] = -w * (dxhy - dyhx) / k0;
    out[3 * plane + (int64_t)m * npts + p] = (ex * hy - ey * hx) / 2;
  }
}

// [c][m][r] -> [c][r][m], 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void k_stage_modes(int k, int nrows, const double* __restrict__ src, double* __restrict__ dst) {
  __shared__ double tile[32][33];
  const int c = blockIdx.z;
  const int r0 = blockIdx.x * 32, m0 = blockIdx.y * 32;
  const double* s = src + (int64_t)c * k * nrows;
  double* d = dst + (int64_t)c * k * nrows;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  for (int j = ty; j < 32; j += 8) {
    const int m = m0 + j, r = r0 + tx;
    if (m < k && r < nrows) tile[j][tx] = s[(int64_t)m * nrows + r];
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int r = r0 + j, m = m0 + tx;
    if (m < k && r < nrows) d[(int64_t)r * k + m] = tile[tx][j];
  }
}

// Overlap: one workgroup walks tiles of OT quadrature points of mesh B (element-major, six points per element) for one
// (32-mode chunk of A, 32-mode chunk of B) pair.  Per tile: OT lanes locate their point in mesh A and stage the basis
// values and rows; all lanes evaluate ua[c][t][i] and w ub[c][t][j] into LDS; every lane then accumulates a 2 x 2 block
// of the 32 x 32 chunk product over the tile.  The workgroup's partial goes to its own slot: no atomics.
constexpr int OT = 64;          // quadrature points per tile
constexpr int OC = 32;          // modes per chunk
constexpr int OVL_BLOCKS = 1024;

__global__ __launch_bounds__(256) void k_field_overlap(LocArgs A, LocArgs B, int ncomp, int ka, int64_t nrows_a,
                                                       const double* __restrict__ Va, int kb, int64_t nrows_b,
                                                       const double* __restrict__ Vb, CoreTable cores, int ncore,
                                                       double inv_eps_core, double inv_eps_clad, int nchunk_b,
                                                       double* __restrict__ partial) {
  __shared__ double s_phi[6][OT];
  __shared__ int s_ra[6][OT], s_rb[6][OT];
  __shared__ double s_w[OT];
  __shared__ int s_q[OT];
  __shared__ double s_ua[2][OT][OC];
  __shared__ double s_ub[2][OT][OC];
  const int tid = threadIdx.x;
  const int ca = blockIdx.y / nchunk_b, cb = blockIdx.y % nchunk_b;
  const int ia0 = ca * OC, jb0 = cb * OC;
  const int64_t nq = (int64_t)6 * B.ne;
  const int64_t ntiles = (nq + OT - 1) / OT;
  const int ti = tid >> 4, tj = tid & 15;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  const double* pbx = B.pxy;
  const double* pby = B.pxy + B.nv;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (tid < OT) {
      const int64_t g = tile * OT + tid;
      double w = 0.0;
      int q = 0;
      for (int a = 0; a < 6; ++a) { s_ra[a][tid] = -1; s_rb[a][tid] = -1; s_phi[a][tid] = 0.0; }
      if (g < nq) {
        const int e = (int)(g / 6);
        q = (int)(g % 6);
        const P2Map M(B.edof, B.ne, pbx, pby, e);
        double X, Y;
        M.point(c_qx[q], c_qy[q], X, Y);
        w = fabs(M.det()) * c_qw[q];
        if (ncore >= 0) w *= in_any_core(X, Y, cores.c, ncore) ? inv_eps_core : inv_eps_clad;
        double axi, aeta, inv[4];
        const int ea = dev_locate(A, X, Y, axi, aeta, inv);
        if (ea >= 0) {
          double phi[6];
          p2_phi(axi, aeta, phi);
          for (int a = 0; a < 6; ++a) {
            s_phi[a][tid] = phi[a];
            s_ra[a][tid] = dev_row(A, ea, a);
            s_rb[a][tid] = dev_row(B, e, a);
          }
        } else {
          w = 0.0;
        }
      }
      s_w[tid] = w;
      s_q[tid] = q;
    }
    __syncthreads();
    // ua[c][t][i] and w ub[c][t][j]: consecutive lanes read consecutive modes of one staged row
    for (int idx = tid; idx < 2 * OT * OC; idx += 256) {
      const int i = idx % OC, t = (idx / OC) % OT, c = idx / (OC * OT);
      double ua = 0.0, ub = 0.0;
      if (c < ncomp) {
        const double* va = Va + c * nrows_a * ka;
        const double* vb = Vb + c * nrows_b * kb;
        const int q = s_q[t];
        const double w = s_w[t];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          const int ra = s_ra[a][t], rb = s_rb[a][t];
          if (ia0 + i < ka && ra >= 0) ua += s_phi[a][t] * va[(int64_t)ra * ka + ia0 + i];
          if (jb0 + i < kb && rb >= 0) {
            const double ph = p2_phi(a, c_qx[q], c_qy[q]);   // B's basis at its own quadrature point q
            ub += ph * vb[(int64_t)rb * kb + jb0 + i];
          }
        }
        ub *= w;
      }
      s_ua[c][t][i] = ua;
      s_ub[c][t][i] = ub;
    }
    __syncthreads();
    for (int c = 0; c < ncomp; ++c) {
      for (int t = 0; t < OT; ++t) {
        const double2 a = *reinterpret_cast<const double2*>(&s_ua[c][t][2 * ti]);
        const double2 b = *reinterpret_cast<const double2*>(&s_ub[c][t][2 * tj]);
        acc[0][0] += a.x * b.x; acc[0][1] += a.x * b.y;
        acc[1][0] += a.y * b.x; acc[1][1] += a.y * b.y;
      }
    }
    __syncthreads();
  }
  double* out = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (OC * OC);
  for (int r = 0; r < 2; ++r)
    for (int s = 0; s < 2; ++s) out[(2 * ti + r) * OC + 2 * tj + s] = acc[r][s];
}

// Posed overlap (plfem_field_overlap_posed): the contract of k_field_overlap with a pose between B's quadrature point
// and its location in A.  A pose row is (tx, ty, c, s, m): a point xi of mesh A appears in B's frame at x = t + m R xi,
// R = [[c, -s], [s, c]], so B's point (X, Y) is looked up in A at R^T (x - t) / m -- every product rounded on its own,
// the division IEEE, which gives (X, Y) back bit for bit under the identity pose -- and A's value there is turned by R
// when the record is vectorial.  The core test and B's own values stay in B's frame.  Grid = (slice of B's tiles, chunk
// pair, pose of the batch); tiles blockIdx.x, blockIdx.x + gridDim.x, ... as in k_field_overlap, and gridDim.x follows
// B's element count alone, so the sum order of an entry depends on neither the other poses nor the mode counts.
// Partials [pose][chunk pair][slice][OC * OC], every slot written: what k_overlap_reduce sums with blockIdx.y = pose.
constexpr int POSE_SLICES = 128;    // most slices (partial blocks) per pose and chunk pair
constexpr int POSE_DOUBLES = 5;

__global__ __launch_bounds__(256) void k_field_overlap_posed(LocArgs A, LocArgs B, int ncomp, int ka, int64_t nrows_a,
                                                             const double* __restrict__ Va, int kb, int64_t nrows_b,
                                                             const double* __restrict__ Vb, CoreTable cores, int ncore,
                                                             double inv_eps_core, double inv_eps_clad, int nchunk_b,
                                                             const double* __restrict__ poses, double* __restrict__ partial) {
  __shared__ double s_phi[6][OT];
  __shared__ int s_ra[6][OT], s_rb[6][OT];
  __shared__ double s_w[OT];
  __shared__ int s_q[OT];
  __shared__ double s_ua[2][OT][OC];
  __shared__ double s_ub[2][OT][OC];
  const int tid = threadIdx.x;
  const int ca = blockIdx.y / nchunk_b, cb = blockIdx.y % nchunk_b;
  const int ia0 = ca * OC, jb0 = cb * OC;
  const double* pose = poses + (int64_t)blockIdx.z * POSE_DOUBLES;     // the same for every lane
  const double tx = pose[0], ty = pose[1], pc = pose[2], ps = pose[3], pm = pose[4];
  const int64_t nq = (int64_t)6 * B.ne;
  const int64_t ntiles = (nq + OT - 1) / OT;
  const int ti = tid >> 4, tj = tid & 15;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  const double* pbx = B.pxy;
  const double* pby = B.pxy + B.nv;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (tid < OT) {
      const int64_t g = tile * OT + tid;
      double w = 0.0;
      int q = 0;
      for (int a = 0; a < 6; ++a) { s_ra[a][tid] = -1; s_rb[a][tid] = -1; s_phi[a][tid] = 0.0; }
      if (g < nq) {
        const int e = (int)(g / 6);
        q = (int)(g % 6);
        const P2Map M(B.edof, B.ne, pbx, pby, e);
        double X, Y;
        M.point(c_qx[q], c_qy[q], X, Y);
        w = fabs(M.det()) * c_qw[q];
        if (ncore >= 0) w *= in_any_core(X, Y, cores.c, ncore) ? inv_eps_core : inv_eps_clad;
        const double dx = X - tx, dy = Y - ty;
        const double xa = (mul_rn(pc, dx) + mul_rn(ps, dy)) / pm;
        const double ya = (mul_rn(pc, dy) - mul_rn(ps, dx)) / pm;
        double axi, aeta, inv[4];
        const int ea = dev_locate(A, xa, ya, axi, aeta, inv);
        if (ea >= 0) {
          double phi[6];
          p2_phi(axi, aeta, phi);
          for (int a = 0; a < 6; ++a) {
            s_phi[a][tid] = phi[a];
            s_ra[a][tid] = dev_row(A, ea, a);
            s_rb[a][tid] = dev_row(B, e, a);
          }
        } else {
          w = 0.0;
        }
      }
      s_w[tid] = w;
      s_q[tid] = q;
    }
    __syncthreads();
    // ua'[c][t][i] and w ub[c][t][j]: a lane holds both components of its (point, mode), so that it can turn A's value
    for (int idx = tid; idx < OT * OC; idx += 256) {
      const int i = idx % OC, t = idx / OC;
      const int q = s_q[t];
      const double w = s_w[t];
      double ua[2] = {0.0, 0.0}, ub[2] = {0.0, 0.0};
      for (int c = 0; c < ncomp; ++c) {
        const double* va = Va + c * nrows_a * ka;
        const double* vb = Vb + c * nrows_b * kb;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          const int ra = s_ra[a][t], rb = s_rb[a][t];
          if (ia0 + i < ka && ra >= 0) ua[c] += s_phi[a][t] * va[(int64_t)ra * ka + ia0 + i];
          if (jb0 + i < kb && rb >= 0) {
            const double ph = p2_phi(a, c_qx[q], c_qy[q]);   // B's basis at its own quadrature point q
            ub[c] += ph * vb[(int64_t)rb * kb + jb0 + i];
          }
        }
        ub[c] *= w;
      }
      if (ncomp == 2) {
        const double ux = ua[0], uy = ua[1];
        ua[0] = mul_rn(pc, ux) - mul_rn(ps, uy);
        ua[1] = mul_rn(ps, ux) + mul_rn(pc, uy);
      }
      s_ua[0][t][i] = ua[0]; s_ua[1][t][i] = ua[1];
      s_ub[0][t][i] = ub[0]; s_ub[1][t][i] = ub[1];
    }
    __syncthreads();
    for (int c = 0; c < ncomp; ++c) {
      for (int t = 0; t < OT; ++t) {
        const double2 a = *reinterpret_cast<const double2*>(&s_ua[c][t][2 * ti]);
        const double2 b = *reinterpret_cast<const double2*>(&s_ub[c][t][2 * tj]);
        acc[0][0] += a.x * b.x; acc[0][1] += a.x * b.y;
        acc[1][0] += a.y * b.x; acc[1][1] += a.y * b.y;
      }
    }
    __syncthreads();
  }
  double* out = partial + (((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (OC * OC);
  for (int r = 0; r < 2; ++r)
    for (int s = 0; s < 2; ++s) out[(2 * ti + r) * OC + 2 * tj + s] = acc[r][s];
}

// Second stage: O[i][j] = sum over the workgroups' partials in workgroup order (the k_axpy_first pattern: fixed order,
// the same bits on every run).  blockIdx.y = output matrix: partials [gridDim.y][gridDim.x][nblk][OC * OC], O [gridDim.y][ka][kb]
// (k_field_overlap: one matrix; k_mode_grams: five or three).  blockIdx.z = slice of the OC x OC entries (each entry is still
// summed by one lane, in workgroup order).
__global__ __launch_bounds__(256) void k_overlap_reduce(int ka, int kb, int nblk, int nchunk_b, const double* __restrict__ partial,
                                                        double* __restrict__ O) {
  const int ca = blockIdx.x / nchunk_b, cb = blockIdx.x % nchunk_b;
  const double* pp = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * nblk * (OC * OC);
  O += (int64_t)blockIdx.y * ka * kb;
  for (int v = blockIdx.z * 256 + threadIdx.x; v < OC * OC; v += 256 * gridDim.z) {
    const int i = ca * OC + v / OC, j = cb * OC + v % OC;
    if (i >= ka || j >= kb) continue;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += pp[(int64_t)b * (OC * OC) + v];
    O[(int64_t)i * kb + j] = s;
  }
}

// Same-mesh Grams of k modes under the element forms of the assembly, split by material region (plfem_mode_grams).  One
// workgroup walks tiles of GT quadrature points of the mesh's own six-point rule (element-major) for one (32-mode chunk,
// 32-mode chunk) pair.  Per tile: GT lanes form det J, J^-1, the quadrature point and its core test (p2_element.h, as the
// assembly does), and stage the physical basis gradients, the weight and the rows; all lanes then evaluate the
// features of every (point, mode) -- ncomp = 2: hx, hy, dx hx, dy hx, dx hy, dy hy; ncomp = 1: u, dx u, dy u -- plain
// for the row chunk, times |det J| w_q for the column chunk; every lane accumulates a 2 x 2 block of each output over the
// tile.  The region of a point is the same for all lanes, so its branch costs no divergence and the region split costs
// no extra products.  Outputs (ncomp = 2): M_core, M_clad, K_core, K_clad, D; (ncomp = 1): M_core, M_clad, S.
constexpr int GT = 16;          // quadrature points per tile
constexpr int GRAM_BLOCKS = 768;

// What k_mode_grams and k_core_grams share.  gram_stage_point: lane `lane` of a tile stages quadrature point g (element
// g / 6, point g % 6 of the six-point rule) -- det J, J^-1, the physical basis gradients, the weight |det J| w_q, the
// staged rows -- or, when not `live`, a point that contributes nothing (rows -1, weight 0).  at_point(X, Y) is called for
// a live point with the physical point as the assembly forms it; an at_point(X, Y, inv) also gets the point's J^-1.
template <typename AtPoint>
__device__ __forceinline__ void gram_stage_point(const LocArgs& L, int64_t g, bool live, int lane, double (&s_gx)[6][GT],
                                                 double (&s_gy)[6][GT], int (&s_r)[6][GT], double (&s_w)[GT], int (&s_q)[GT],
                                                 AtPoint&& at_point) {
  double w = 0.0;
  int q = 0;
  for (int a = 0; a < 6; ++a) { s_r[a][lane] = -1; s_gx[a][lane] = 0.0; s_gy[a][lane] = 0.0; }
  if (live) {
    const int e = (int)(g / 6);
    q = (int)(g % 6);
    const P2Map M(L.edof, L.ne, L.pxy, L.pxy + L.nv, e);
    const double xi = c_qx[q], eta = c_qy[q];
    double det = M.det(), inv[4], X, Y, gx[6], gy[6];
    M.inverse(det, inv);
    M.point(xi, eta, X, Y);
    if constexpr (std::is_invocable_v<AtPoint, double, double, const double(&)[4]>) at_point(X, Y, inv);
    else at_point(X, Y);
    w = fabs(det) * c_qw[q];
    p2_grad(inv, xi, eta, gx, gy);
    for (int a = 0; a < 6; ++a) {
      s_gx[a][lane] = gx[a];
      s_gy[a][lane] = gy[a];
      s_r[a][lane] = dev_row(L, e, a);
    }
  }
  s_w[lane] = w;
  s_q[lane] = q;
}

// gram_features: all 256 lanes evaluate the features of every (staged point, mode of the row chunk i0 / of the column
// chunk j0) into s_f -- plain for the row chunk, times the point's weight for the column chunk.  Consecutive lanes read
// consecutive modes of one staged row.
template <int NCOMP>
__device__ __forceinline__ void gram_features(int tid, int k, int64_t nrows, const double* __restrict__ V, int i0, int j0,
                                              const double (&s_gx)[6][GT], const double (&s_gy)[6][GT], const int (&s_r)[6][GT],
                                              const double (&s_w)[GT], const int (&s_q)[GT],
                                              double (&s_f)[2][3 * NCOMP][GT][OC]) {
  constexpr int NF = 3 * NCOMP;
  for (int idx = tid; idx < 2 * GT * OC; idx += 256) {
    const int i = idx % OC, t = (idx / OC) % GT, side = idx / (OC * GT);
    const int m = (side ? j0 : i0) + i;
    double f[NF];
#pragma unroll
    for (int c = 0; c < NF; ++c) f[c] = 0.0;
    if (m < k) {
      double phi[6];
      p2_phi(c_qx[s_q[t]], c_qy[s_q[t]], phi);
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const int r = s_r[a][t];
        if (r < 0) continue;
        const double gx = s_gx[a][t], gy = s_gy[a][t];
#pragma unroll
        for (int c = 0; c < NCOMP; ++c) {
          const double v = V[(int64_t)c * nrows * k + (int64_t)r * k + m];
          f[c] += phi[a] * v;
          f[NCOMP + 2 * c] += gx * v;
          f[NCOMP + 2 * c + 1] += gy * v;
        }
      }
      if (side) {
        const double w = s_w[t];
#pragma unroll
        for (int c = 0; c < NF; ++c) f[c] *= w;
      }
    }
#pragma unroll
    for (int c = 0; c < NF; ++c) s_f[side][c][t][i] = f[c];
  }
}

// acc[o] += s x a[p] (x) b[q], s = +-1, on a lane's 2 x 2 block.  Explicit fused multiply-adds: left to contraction, a
// product that both region branches of k_mode_grams share is hoisted above the branch, and the compiler then fuses it
// into some of the four accumulators of the 2 x 2 block and not others, so that an entry's rounding would depend on its
// place in the block
#define GRAM_ACC(o, p, q, s)                                                                        \
      acc[o][0][0] = fma((s) * a[p].x, b[q].x, acc[o][0][0]); acc[o][0][1] = fma((s) * a[p].x, b[q].y, acc[o][0][1]); \
      acc[o][1][0] = fma((s) * a[p].y, b[q].x, acc[o][1][0]); acc[o][1][1] = fma((s) * a[p].y, b[q].y, acc[o][1][1]);

// acc[o] += wgt x p on a lane's 2 x 2 block, p the block's unweighted products (gram_m_block, gram_k_block) and wgt the
// same for every lane: the accumulate of k_moment_grams and k_weighted_grams.
#define GRAM_WACC(o, wgt, p)                                                                        \
      acc[o][0][0] = fma(wgt, p[0][0], acc[o][0][0]); acc[o][0][1] = fma(wgt, p[0][1], acc[o][0][1]); \
      acc[o][1][0] = fma(wgt, p[1][0], acc[o][1][0]); acc[o][1][1] = fma(wgt, p[1][1], acc[o][1][1]);

// p = a[0] (x) b[0] (+ a[1] (x) b[1] when NCOMP = 2) on a lane's block: u u', or hx hx' + hy hy'.  One multiply, then one
// fused multiply-add, in this order for the four entries.
template <int NCOMP, int NF>
__device__ __forceinline__ void gram_m_block(const double2 (&a)[NF], const double2 (&b)[NF], double (&p)[2][2]) {
  p[0][0] = a[0].x * b[0].x; p[0][1] = a[0].x * b[0].y; p[1][0] = a[0].y * b[0].x; p[1][1] = a[0].y * b[0].y;
  if constexpr (NCOMP == 2) {
    p[0][0] = fma(a[1].x, b[1].x, p[0][0]); p[0][1] = fma(a[1].x, b[1].y, p[0][1]);
    p[1][0] = fma(a[1].y, b[1].x, p[1][0]); p[1][1] = fma(a[1].y, b[1].y, p[1][1]);
  }
}

// p = the form of K_r on a lane's block: dy hx dy hx' + dx hy dx hy' - dx hx dy hy' - dy hy dx hx' (features 2 dx hx,
// 3 dy hx, 4 dx hy, 5 dy hy).  One multiply, then three fused multiply-adds, in this order for the four entries.
#define GRAM_K_ENTRY(r_, s_, ar, bs)                                                                \
  p[r_][s_] = a[3].ar * b[3].bs; p[r_][s_] = fma(a[4].ar, b[4].bs, p[r_][s_]);                       \
  p[r_][s_] = fma(-a[2].ar, b[5].bs, p[r_][s_]); p[r_][s_] = fma(-a[5].ar, b[2].bs, p[r_][s_]);
__device__ __forceinline__ void gram_k_block(const double2 (&a)[6], const double2 (&b)[6], double (&p)[2][2]) {
  GRAM_K_ENTRY(0, 0, x, x) GRAM_K_ENTRY(0, 1, x, y) GRAM_K_ENTRY(1, 0, y, x) GRAM_K_ENTRY(1, 1, y, y)
}
#undef GRAM_K_ENTRY

// The LDS of a tile: what gram_stage_point stages and gram_features fills.  A kernel's own per-point values (region,
// material weight, coordinates, velocity gradient) stay in arrays of its own.  alignas(16): the loads of the t loop are
// double2; a struct of doubles is 8-aligned, and then each becomes a pair of 64-bit LDS reads (a fifth slower, measured).
template <int NCOMP>
struct alignas(16) GramTile {
  double f[2][3 * NCOMP][GT][OC];             // [0]: row chunk, plain; [1]: column chunk, times the weight
  double gx[6][GT], gy[6][GT];
  int r[6][GT];
  double w[GT];                               // |det J| w_q
  int q[GT];
};

template <int NCOMP, typename AtPoint>
__device__ __forceinline__ void gram_stage_point(const LocArgs& L, int64_t g, bool live, int lane, GramTile<NCOMP>& S,
                                                 AtPoint&& at_point) {
  gram_stage_point(L, g, live, lane, S.gx, S.gy, S.r, S.w, S.q, at_point);
}

// What the same-mesh Gram kernels after k_mode_grams share besides the tile, as a local object of the kernel: the lane's
// place in the workgroup's (row chunk, column chunk) pair = blockIdx.y, its zeroed 2 x 2 block of each of NOUT outputs,
// the feature pass, the loads of the t loop and the store of the partials.  The tile walk, the staging and every
// accumulate stay in the kernel, on `acc` through a local reference: the accumulators must never be seen through a
// pointer that a branch could index (they would go to scratch).  k_mode_grams itself stays written out: its scalar
// instance measured 0.4 % slower on the frame.
template <int NCOMP, int NOUT>
struct GramFrame {
  static constexpr int NF = 3 * NCOMP;        // features per (point, mode)
  const int tid, i0, j0, ti, tj;
  double acc[NOUT][2][2];

  __device__ __forceinline__ explicit GramFrame(int nchunk)
      : tid(threadIdx.x), i0((int)(blockIdx.y / nchunk) * OC), j0((int)(blockIdx.y % nchunk) * OC), ti(tid >> 4), tj(tid & 15) {
#pragma unroll
    for (int o = 0; o < NOUT; ++o) acc[o][0][0] = acc[o][0][1] = acc[o][1][0] = acc[o][1][1] = 0.0;
  }

  // gram_features between its two barriers: after the staging lanes, before the t loop.  settle = false leaves the
  // second barrier to a caller that first rewrites features in place, every lane those it wrote itself.
  __device__ __forceinline__ void features(GramTile<NCOMP>& S, int k, int64_t nrows, const double* __restrict__ V,
                                           bool settle = true) const {
    __syncthreads();
    gram_features<NCOMP>(tid, k, nrows, V, i0, j0, S.gx, S.gy, S.r, S.w, S.q, S.f);
    if (settle) __syncthreads();
  }

  // features C0 .. C1 - 1 of point t: the lane's two row modes and two column modes
  template <int C0 = 0, int C1 = NF>
  __device__ __forceinline__ void load(const GramTile<NCOMP>& S, int t, double2 (&a)[NF], double2 (&b)[NF]) const {
#pragma unroll
    for (int c = C0; c < C1; ++c) {
      a[c] = *reinterpret_cast<const double2*>(&S.f[0][c][t][2 * ti]);
      b[c] = *reinterpret_cast<const double2*>(&S.f[1][c][t][2 * tj]);
    }
  }

  // The partial slots: [output][chunk pair][slice = blockIdx.x][OC * OC], output o of the kernel at first_out + place(o)
  // of the launch's list, every slot written.  This is one half of a contract: k_overlap_reduce sums the slices of
  // (output, chunk pair) in slice order, and gram_layout, CoreGramLayout, VelocityGramLayout and TangentGramLayout size
  // the buffer and count the outputs (first_out = core x NOUT, velocity x NOUT for the listed calls).
  template <typename Place>
  __device__ __forceinline__ void store(double* __restrict__ partial, int64_t first_out, Place place) const {
    const int64_t npair = (int64_t)gridDim.y;
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
      double* out = partial + (((first_out + place(o)) * npair + blockIdx.y) * gridDim.x + blockIdx.x) * (OC * OC);
      for (int r = 0; r < 2; ++r)
        for (int s = 0; s < 2; ++s) out[(2 * ti + r) * OC + 2 * tj + s] = acc[o][r][s];
    }
  }
  __device__ __forceinline__ void store(double* __restrict__ partial, int64_t first_out) const {
    store(partial, first_out, [](int o) { return o; });
  }
};

template <int NCOMP>
__global__ __launch_bounds__(256) void k_mode_grams(LocArgs L, int k, int64_t nrows, const double* __restrict__ V,
                                                    CoreTable cores, int ncore, int nchunk, double* __restrict__ partial) {
  constexpr int NF = 3 * NCOMP;               // features per (point, mode)
  constexpr int NOUT = NCOMP == 2 ? 5 : 3;
  __shared__ double s_f[2][NF][GT][OC];       // [0]: row chunk, plain; [1]: column chunk, times the weight
  __shared__ double s_gx[6][GT], s_gy[6][GT];
  __shared__ int s_r[6][GT];
  __shared__ double s_w[GT];
  __shared__ int s_q[GT], s_core[GT];
  const int tid = threadIdx.x;
  const int ci = blockIdx.y / nchunk, cj = blockIdx.y % nchunk;
  const int i0 = ci * OC, j0 = cj * OC;
  const int64_t nq = (int64_t)6 * L.ne;
  const int64_t ntiles = (nq + GT - 1) / GT;
  const int ti = tid >> 4, tj = tid & 15;
  double acc[NOUT][2][2];
#pragma unroll
  for (int o = 0; o < NOUT; ++o) acc[o][0][0] = acc[o][0][1] = acc[o][1][0] = acc[o][1][1] = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (tid < GT) {
      const int64_t g = tile * GT + tid;
      int core = 0;
      gram_stage_point(L, g, g < nq, tid, s_gx, s_gy, s_r, s_w, s_q,
                       [&](double X, double Y) { core = in_any_core(X, Y, cores.c, ncore) ? 1 : 0; });
      s_core[tid] = core;
    }
    __syncthreads();
    gram_features<NCOMP>(tid, k, nrows, V, i0, j0, s_gx, s_gy, s_r, s_w, s_q, s_f);
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < GT; ++t) {
      double2 a[NF], b[NF];
#pragma unroll
      for (int c = 0; c < NF; ++c) {
        a[c] = *reinterpret_cast<const double2*>(&s_f[0][c][t][2 * ti]);
        b[c] = *reinterpret_cast<const double2*>(&s_f[1][c][t][2 * tj]);
      }
      const int r = s_core[t] ? 0 : 1;          // the same for every lane
      if (NCOMP == 2) {
        // M_r: hx hx + hy hy;  K_r: dy hx dy hx + dx hy dx hy - dx hx dy hy - dy hy dx hx;
        // D: dx hx dx hx + dy hy dy hy + dy hx dx hy + dx hy dy hx  (features 0 hx, 1 hy, 2 dx hx, 3 dy hx, 4 dx hy, 5 dy hy)
        if (r == 0) {
          GRAM_ACC(0, 0, 0, 1.0) GRAM_ACC(0, 1, 1, 1.0)
          GRAM_ACC(2, 3, 3, 1.0) GRAM_ACC(2, 4, 4, 1.0) GRAM_ACC(2, 2, 5, -1.0) GRAM_ACC(2, 5, 2, -1.0)
        } else {
          GRAM_ACC(1, 0, 0, 1.0) GRAM_ACC(1, 1, 1, 1.0)
          GRAM_ACC(3, 3, 3, 1.0) GRAM_ACC(3, 4, 4, 1.0) GRAM_ACC(3, 2, 5, -1.0) GRAM_ACC(3, 5, 2, -1.0)
        }
        GRAM_ACC(NOUT - 1, 2, 2, 1.0) GRAM_ACC(NOUT - 1, 5, 5, 1.0) GRAM_ACC(NOUT - 1, 3, 4, 1.0) GRAM_ACC(NOUT - 1, 4, 3, 1.0)
      } else {
        // M_r: u u;  S: dx u dx u + dy u dy u  (features 0 u, 1 dx u, 2 dy u)
        if (r == 0) { GRAM_ACC(0, 0, 0, 1.0) } else { GRAM_ACC(1, 0, 0, 1.0) }
        GRAM_ACC(NOUT - 1, 1, 1, 1.0) GRAM_ACC(NOUT - 1, NF - 1, NF - 1, 1.0)
      }
    }
    __syncthreads();
  }
  const int64_t npair = (int64_t)gridDim.y;
#pragma unroll
  for (int o = 0; o < NOUT; ++o) {
    double* out = partial + (((int64_t)o * npair + blockIdx.y) * gridDim.x + blockIdx.x) * (OC * OC);
    for (int r = 0; r < 2; ++r)
      for (int s = 0; s < 2; ++s) out[(2 * ti + r) * OC + 2 * tj + s] = acc[o][r][s];
  }
}

// Per-core Grams (plfem_core_grams): the Grams of the modes restricted to each core disc, in three passes.
//
// Pass 1, k_core_owner: one lane per quadrature point of the six-point rule, element-major; the point formed as the
// assembly forms it; owner[g] = core_owner (p2_element.h): the highest-index closed disc holding it, or -1.
__global__ __launch_bounds__(256) void k_core_owner(LocArgs L, CoreTable cores, int ncore, int32_t* __restrict__ owner) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (int64_t)6 * L.ne) return;
  const int e = (int)(g / 6), q = (int)(g % 6);
  const P2Map M(L.edof, L.ne, L.pxy, L.pxy + L.nv, e);
  double X, Y;
  M.point(c_qx[q], c_qy[q], X, Y);
  owner[g] = core_owner(X, Y, cores.c, ncore);
}

// Pass 2, compaction: per core the ascending list of the points it owns.  One workgroup per core walks the owner array
// in order, first to count (k_core_count), then, with the exclusive offsets summed from the counts, to fill
// (k_core_fill).  A point's place is its rank among the core's points -- ballot and popcount inside a wave, the four
// wave totals in wave order, a running base across the 256-point steps -- so the lists do not depend on scheduling and
// no atomic is involved.  meta = counts [MAX_CORES], then offsets [MAX_CORES].
__global__ __launch_bounds__(256) void k_core_count(int64_t nq, const int32_t* __restrict__ owner, int32_t* __restrict__ meta) {
  __shared__ int s_n[256];
  const int tid = threadIdx.x, c = blockIdx.x;
  int n = 0;
  for (int64_t g = tid; g < nq; g += 256) n += owner[g] == c ? 1 : 0;
  s_n[tid] = n;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) s_n[tid] += s_n[tid + h];
    __syncthreads();
  }
  if (tid == 0) meta[c] = s_n[0];
}

__global__ __launch_bounds__(256) void k_core_fill(int64_t nq, const int32_t* __restrict__ owner, int32_t* __restrict__ meta,
                                                   int32_t* __restrict__ list) {
  __shared__ int s_wave[4];
  const int tid = threadIdx.x, c = blockIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int j = 0; j < c; ++j) base += meta[j];
  if (tid == 0) meta[MAX_CORES + c] = base;
  for (int64_t g0 = 0; g0 < nq; g0 += 256) {
    const int64_t g = g0 + tid;
    const bool mine = g < nq && owner[g] == c;
    const unsigned long long votes = __ballot(mine);
    if (lane == 0) s_wave[wave] = __popcll(votes);
    __syncthreads();
    int before = __popcll(votes & ((1ull << lane) - 1ull)), total = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) before += s_wave[w];
      total += s_wave[w];
    }
    if (mine) list[base + before] = (int32_t)g;
    base += total;
    __syncthreads();
  }
}

// Pass 3, k_core_grams: grid = (slice, chunk pair, core).  The workgroup walks tiles of GT points of its core's list --
// tiles blockIdx.x, blockIdx.x + gridDim.x, ... of that core's ceil(count / GT), so the slices at work follow the core's
// tile count and the others write zeros -- staging and features as in k_mode_grams (gram_stage_point, gram_features; a
// list's last tile is padded with points that contribute nothing).  Every point of the walk is the core's: no region
// branch.  Outputs (ncomp = 2): Mx = hx hx, My = hy hy, K (the form of K_r above); (ncomp = 1): M = u u.  Partials
// [core][output][chunk pair][slice][OC * OC], every slot written: the layout k_overlap_reduce sums with blockIdx.y = core x
// output.
template <int NCOMP>
__global__ __launch_bounds__(256) void k_core_grams(LocArgs L, int k, int64_t nrows, const double* __restrict__ V,
                                                    const int32_t* __restrict__ meta, const int32_t* __restrict__ list,
                                                    int nchunk, double* __restrict__ partial) {
  constexpr int NF = 3 * NCOMP;
  constexpr int NOUT = NCOMP == 2 ? 3 : 1;
  __shared__ GramTile<NCOMP> S;
  GramFrame<NCOMP, NOUT> F(nchunk);
  double (&acc)[NOUT][2][2] = F.acc;
  const int tid = F.tid, core = blockIdx.z;
  const int count = meta[core];
  const int32_t* mine = list + meta[MAX_CORES + core];
  const int ntiles = (count + GT - 1) / GT;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (tid < GT) {
      const int p = tile * GT + tid;
      const bool live = p < count;
      gram_stage_point(L, live ? (int64_t)mine[p] : 0, live, tid, S, [](double, double) {});
    }
    F.features(S, k, nrows, V);
#pragma unroll 1
    for (int t = 0; t < GT; ++t) {
      double2 a[NF], b[NF];
      F.load(S, t, a, b);
      GRAM_ACC(0, 0, 0, 1.0)                    // Mx (M when ncomp = 1)
      if constexpr (NCOMP == 2) {
        GRAM_ACC(1, 1, 1, 1.0)
        GRAM_ACC(2, 3, 3, 1.0) GRAM_ACC(2, 4, 4, 1.0) GRAM_ACC(2, 2, 5, -1.0) GRAM_ACC(2, 5, 2, -1.0)
      }
    }
    __syncthreads();
  }
  F.store(partial, (int64_t)core * NOUT);
}

// Grams of a profile solve (plfem_profile_grams): the forms of k_mode_grams with the permittivity of an index profile in
// place of the two regions.  Grid, tiling, staging and features as in k_mode_grams; the staging lane evaluates
// profile_eps (p2_element.h) at its point, as the profile instance of k_element_matrices does, and puts the point's
// weight -- ncomp = 2: 1 / eps, the division made here; ncomp = 1: eps; 1 for a padding point, whose features are 0 --
// into LDS.  The weight is the same for every lane and enters as GRAM_ACC's factor, so every product is written out:
// (w a) b + acc, the same for the four entries of a lane's block.  Outputs (ncomp = 2): M, M_w, K_w, D; (ncomp = 1):
// M, M_w, S, with M the unweighted u . u' and K, D, S the forms of k_mode_grams.  The layer table is read at indices
// the workgroup shares (uniform loads) by the GT staging lanes only.
// Map...: nothing, or one EpsMap (a sampled map under the layers, plfem_locator_set_index_map): the instances without a
// map keep their argument list and their code.
template <int NCOMP, typename... Map>
__global__ __launch_bounds__(256) void k_profile_grams(LocArgs L, int k, int64_t nrows, const double* __restrict__ V,
                                                       const double* __restrict__ layers, int nlayer, double eps_bg, int nchunk,
                                                       double* __restrict__ partial, Map... map) {
  constexpr int NF = 3 * NCOMP;
  constexpr int NOUT = NCOMP == 2 ? 4 : 3;
  __shared__ GramTile<NCOMP> S;
  __shared__ double s_wt[GT];                 // the material weight of the point
  GramFrame<NCOMP, NOUT> F(nchunk);
  double (&acc)[NOUT][2][2] = F.acc;
  const int tid = F.tid;
  const int64_t nq = (int64_t)6 * L.ne;
  const int64_t ntiles = (nq + GT - 1) / GT;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (tid < GT) {
      const int64_t g = tile * GT + tid;
      double wt = 1.0;
      gram_stage_point(L, g, g < nq, tid, S, [&](double X, double Y) {
        const double eps = profile_eps(X, Y, layers, nlayer, eps_bg, map...);
        wt = NCOMP == 2 ? 1.0 / eps : eps;
      });
      s_wt[tid] = wt;
    }
    F.features(S, k, nrows, V);
#pragma unroll 1
    for (int t = 0; t < GT; ++t) {
      double2 a[NF], b[NF];
      F.load(S, t, a, b);
      const double w = s_wt[t];                 // the same for every lane
      if constexpr (NCOMP == 2) {
        // features 0 hx, 1 hy, 2 dx hx, 3 dy hx, 4 dx hy, 5 dy hy
        GRAM_ACC(0, 0, 0, 1.0) GRAM_ACC(0, 1, 1, 1.0)
        GRAM_ACC(1, 0, 0, w) GRAM_ACC(1, 1, 1, w)
        GRAM_ACC(2, 3, 3, w) GRAM_ACC(2, 4, 4, w) GRAM_ACC(2, 2, 5, -w) GRAM_ACC(2, 5, 2, -w)
        GRAM_ACC(3, 2, 2, 1.0) GRAM_ACC(3, 5, 5, 1.0) GRAM_ACC(3, 3, 4, 1.0) GRAM_ACC(3, 4, 3, 1.0)
      } else {
        // features 0 u, 1 dx u, 2 dy u
        GRAM_ACC(0, 0, 0, 1.0)
        GRAM_ACC(1, 0, 0, w)
        GRAM_ACC(2, 1, 1, 1.0) GRAM_ACC(2, 2, 2, 1.0)
      }
    }
    __syncthreads();
  }
  F.store(partial, 0);
}

// Power Grams of vectorial modes (plfem_flux_grams): with e = E / Z0 from curl H = j w eps0 eps E, the cross power of
// modes m, n is P[m][n] = 1/2 int (Ex_m Hy_n - Ey_m Hx_n) = (beta_m M_w[m][n] + G_w[m][n] / beta_m) / (2 k0) with
//   M_w[m][n] = int w (hx_m hx_n + hy_m hy_n),   G_w[m][n] = int w (gx_m hx_n + gy_m hy_n),   w = 1 / eps,
//   gx = -(hx,xx + hy,xy),  gy = -(hx,xy + hy,yy)   (-grad of the transverse divergence: constant per element for P2),
// so the device sums are free of beta and k0.  Grid, tiling and staging as in k_profile_grams; the staging lane also puts
// the physical Hessians of the six basis functions (p2_basis_hess: 18 values per point) and the point's region -- the
// closed discs of `mat.cores`, whatever the material instance -- into LDS.  Features per (point, mode): hx, hy, gx, gy for
// the row chunk; hx, hy times |det J| w_q for the column chunk (G_w is not symmetric: its rows carry g).  w enters as
// GRAM_ACC's factor as in k_profile_grams.  Outputs: M_w_core, M_w_rest, G_w_core, G_w_rest.  A padding point has rows
// -1, Hessians 0 and weight 0; a boundary DOF of an indexed record is skipped: both contribute 0.
template <bool PROFILE, typename... Map>
__global__ __launch_bounds__(256) void k_flux_grams(LocArgs L, int k, int64_t nrows, const double* __restrict__ V, Material mat,
                                                    int nchunk, double* __restrict__ partial, Map... map) {
  constexpr int NOUT = 4;
  __shared__ double s_fr[4][GT][OC];          // row chunk: hx, hy, gx, gy
  __shared__ double s_fc[2][GT][OC];          // column chunk: hx, hy, times the weight
  __shared__ double s_gx[6][GT], s_gy[6][GT]; // (staged by gram_stage_point; the features here need no gradients)
  __shared__ double s_h[3][6][GT];            // xx, xy, yy of the six basis functions
  __shared__ int s_r[6][GT];
  __shared__ double s_w[GT], s_wt[GT];        // |det J| w_q, and 1 / eps of the point
  __shared__ int s_q[GT], s_core[GT];
  GramFrame<2, NOUT> F(nchunk);               // the frame's indices, accumulators and store; the tile is this kernel's own
  double (&acc)[NOUT][2][2] = F.acc;
  const int tid = F.tid, i0 = F.i0, j0 = F.j0, ti = F.ti, tj = F.tj;
  const int64_t nq = (int64_t)6 * L.ne;
  const int64_t ntiles = (nq + GT - 1) / GT;
  const double* V1 = V + nrows * k;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (tid < GT) {
      const int64_t g = tile * GT + tid;
      double wt = 1.0;
      int core = 0;
      for (int a = 0; a < 6; ++a) s_h[0][a][tid] = s_h[1][a][tid] = s_h[2][a][tid] = 0.0;
      gram_stage_point(L, g, g < nq, tid, s_gx, s_gy, s_r, s_w, s_q, [&](double X, double Y, const double(&inv)[4]) {
        double hxx[6], hxy[6], hyy[6];
        p2_basis_hess(inv, hxx, hxy, hyy);
        for (int a = 0; a < 6; ++a) { s_h[0][a][tid] = hxx[a]; s_h[1][a][tid] = hxy[a]; s_h[2][a][tid] = hyy[a]; }
        const bool in = in_any_core(X, Y, mat.cores.c, mat.ncore);
        core = in ? 1 : 0;
        wt = 1.0 / material_eps<PROFILE>(mat, X, Y, in, map...);
      });
      s_wt[tid] = wt;
      s_core[tid] = core;
    }
    __syncthreads();
    // the features: GT OC (point, mode) pairs per side, the side the same for all lanes of a pass
    for (int idx = tid; idx < 2 * GT * OC; idx += 256) {
      const int i = idx % OC, t = (idx / OC) % GT, side = idx / (OC * GT);
      const int m = (side ? j0 : i0) + i;
      double hx = 0.0, hy = 0.0, sx = 0.0, sy = 0.0;
      if (m < k) {
        double phi[6];
        p2_phi(c_qx[s_q[t]], c_qy[s_q[t]], phi);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          const int r = s_r[a][t];
          if (r < 0) continue;
          const double vx = V[(int64_t)r * k + m], vy = V1[(int64_t)r * k + m];
          hx += phi[a] * vx;
          hy += phi[a] * vy;
          if (!side) {
            const double hxy = s_h[1][a][t];
            sx += s_h[0][a][t] * vx + hxy * vy;
            sy += hxy * vx + s_h[2][a][t] * vy;
          }
        }
      }
      if (side) {
        const double w = s_w[t];
        s_fc[0][t][i] = hx * w;
        s_fc[1][t][i] = hy * w;
      } else {
        s_fr[0][t][i] = hx;
        s_fr[1][t][i] = hy;
        s_fr[2][t][i] = -sx;
        s_fr[3][t][i] = -sy;
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < GT; ++t) {
      double2 a[4], b[2];
#pragma unroll
      for (int c = 0; c < 4; ++c) a[c] = *reinterpret_cast<const double2*>(&s_fr[c][t][2 * ti]);
#pragma unroll
      for (int c = 0; c < 2; ++c) b[c] = *reinterpret_cast<const double2*>(&s_fc[c][t][2 * tj]);
      const double w = s_wt[t];                 // the same for every lane, as is the region
      // row features 0 hx, 1 hy, 2 gx, 3 gy; column features 0 hx, 1 hy
      if (s_core[t]) {
        GRAM_ACC(0, 0, 0, w) GRAM_ACC(0, 1, 1, w)
        GRAM_ACC(2, 2, 0, w) GRAM_ACC(2, 3, 1, w)
      } else {
        GRAM_ACC(1, 0, 0, w) GRAM_ACC(1, 1, 1, w)
        GRAM_ACC(3, 2, 0, w) GRAM_ACC(3, 3, 1, w)
      }
    }
    __syncthreads();
  }
  F.store(partial, 0);
}

// Velocity Grams (plfem_velocity_grams): the first-order change of the forms of k_profile_grams when the mesh moves by
// x -> x + t V with the material convected with the points (the volume form of the shape derivative).  V is P1 on the
// vertices ([nv][2] per velocity), so on an element it has a constant gradient G[2 a + b] = dV_a / dx_b, and with
// tr = G_xx + G_yy and gt(f) = -G^T grad f + (tr / 2) grad f every gradient form changes by P + P^T, P the form with gt on
// the row mode and the plain gradient on the column mode; a mass form changes by sum tr |det J| w_q c u_m . u_n, which
// is Q + Q^T with (tr / 2) u on the row mode.  An element with G = 0 contributes nothing: the walk is over the elements
// with G != 0 only, in four passes as in plfem_core_grams.
constexpr int VG_GROUP = 16;     // most velocities per group: one launch of each pass
constexpr int VG_SLICES = 128;   // most slices (partial blocks) per velocity and chunk pair

// G of element e from the three vertex velocities and the element map: G = [v1 - v0, v2 - v0] adj(J) / det J, every
// product rounded on its own as in P2Map::det, then one division.  Equal vertex velocities give exact zeros, and V = x
// gives the identity exactly on every element, a sliver included: its numerators are det J and 0 bit for bit.
__device__ __forceinline__ void velocity_grad(const LocArgs& L, const double* __restrict__ vel, int e, const P2Map& M, double det,
                                              double G[4]) {
  const int v0 = L.edof[e], v1 = L.edof[L.ne + e], v2 = L.edof[2 * L.ne + e];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const double d1 = vel[2 * v1 + a] - vel[2 * v0 + a], d2 = vel[2 * v2 + a] - vel[2 * v0 + a];
    G[2 * a] = (mul_rn(d1, M.j11) - mul_rn(d2, M.j10)) / det;
    G[2 * a + 1] = (mul_rn(d2, M.j00) - mul_rn(d1, M.j01)) / det;
  }
}

// Pass 1, k_velocity_flag: one lane per (element, velocity = blockIdx.y); flag = any entry of G non-zero.
__global__ __launch_bounds__(256) void k_velocity_flag(LocArgs L, const double* __restrict__ vel, int32_t* __restrict__ flag) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= L.ne) return;
  const P2Map M(L.edof, L.ne, L.pxy, L.pxy + L.nv, e);
  double G[4];
  velocity_grad(L, vel + (int64_t)blockIdx.y * 2 * L.nv, e, M, M.det(), G);
  flag[(int64_t)blockIdx.y * L.ne + e] = (G[0] != 0.0 || G[1] != 0.0 || G[2] != 0.0 || G[3] != 0.0) ? 1 : 0;
}

// Pass 2, compaction, the scheme of k_core_count / k_core_fill: one workgroup per velocity counts its flagged elements,
// then, with the exclusive offsets summed from the counts, fills its ascending list by rank -- ballot and popcount inside
// a wave, the four wave totals in wave order, a running base across the 256-element steps: no atomic decides a position.
// meta = counts [VG_GROUP], then offsets [VG_GROUP].
__global__ __launch_bounds__(256) void k_velocity_count(int ne, const int32_t* __restrict__ flag, int32_t* __restrict__ meta) {
  __shared__ int s_n[256];
  const int tid = threadIdx.x, v = blockIdx.x;
  const int32_t* mine = flag + (int64_t)v * ne;
  int n = 0;
  for (int e = tid; e < ne; e += 256) n += mine[e] ? 1 : 0;
  s_n[tid] = n;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) s_n[tid] += s_n[tid + h];
    __syncthreads();
  }
  if (tid == 0) meta[v] = s_n[0];
}

__global__ __launch_bounds__(256) void k_velocity_fill(int ne, const int32_t* __restrict__ flag, int32_t* __restrict__ meta,
                                                       int32_t* __restrict__ list) {
  __shared__ int s_wave[4];
  const int tid = threadIdx.x, v = blockIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t* mine = flag + (int64_t)v * ne;
  int64_t base = 0;
  for (int j = 0; j < v; ++j) base += meta[j];
  if (tid == 0) meta[VG_GROUP + v] = (int32_t)base;
  for (int e0 = 0; e0 < ne; e0 += 256) {
    const int e = e0 + tid;
    const bool in = e < ne && mine[e] != 0;
    const unsigned long long votes = __ballot(in);
    if (lane == 0) s_wave[wave] = __popcll(votes);
    __syncthreads();
    int before = __popcll(votes & ((1ull << lane) - 1ull)), total = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) before += s_wave[w];
      total += s_wave[w];
    }
    if (in) list[base + before] = e;
    base += total;
    __syncthreads();
  }
}

// Pass 3, k_velocity_grams: grid = (slice, chunk pair, velocity of the group).  The workgroup walks tiles of GT points of
// its velocity's element list (six points per listed element, element-major; tiles blockIdx.x, blockIdx.x + gridDim.x,
// ...), staging and features as in k_profile_grams; the staging lane also forms G of its element (velocity_grad) and the
// point's material weight -- ncomp = 2: 1 / eps, ncomp = 1: eps, by material_eps as in k_flux_grams.  The lane that wrote a
// row-chunk feature then turns it into the transformed one: value -> (tr / 2) value, gradient -> gt.  Outputs, each the
// asymmetric half X of X + X^T (k_velocity_symmetrise): (ncomp = 2) K under w with the signs of k_mode_grams, D, M, M under
// w; (ncomp = 1) S, M, M under w.  Partials [velocity][output][chunk pair][slice][OC * OC], every slot written.
template <int NCOMP, bool PROFILE, typename... Map>
__global__ __launch_bounds__(256) void k_velocity_grams(LocArgs L, int k, int64_t nrows, const double* __restrict__ V, Material mat,
                                                        const double* __restrict__ vel, const int32_t* __restrict__ meta,
                                                        const int32_t* __restrict__ list, int nchunk,
                                                        double* __restrict__ partial, Map... map) {
  constexpr int NF = 3 * NCOMP;
  constexpr int NOUT = NCOMP == 2 ? 4 : 3;
  __shared__ GramTile<NCOMP> S;
  __shared__ double s_wt[GT], s_G[4][GT];
  GramFrame<NCOMP, NOUT> F(nchunk);
  double (&acc)[NOUT][2][2] = F.acc;
  double (&s_f)[2][NF][GT][OC] = S.f;
  const int tid = F.tid, v = blockIdx.z;
  const int64_t npts = (int64_t)6 * meta[v];
  const int32_t* mine = list + meta[VG_GROUP + v];
  const double* myvel = vel + (int64_t)v * 2 * L.nv;
  const int64_t ntiles = (npts + GT - 1) / GT;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (tid < GT) {
      const int64_t p = tile * GT + tid;
      const bool live = p < npts;
      const int e = live ? mine[p / 6] : 0;
      double wt = 1.0, G[4] = {0.0, 0.0, 0.0, 0.0};
      gram_stage_point(L, (int64_t)6 * e + p % 6, live, tid, S, [&](double X, double Y) {
        bool in = false;
        if constexpr (!PROFILE) in = in_any_core(X, Y, mat.cores.c, mat.ncore);
        const double eps = material_eps<PROFILE>(mat, X, Y, in, map...);
        wt = NCOMP == 2 ? 1.0 / eps : eps;
        const P2Map M(L.edof, L.ne, L.pxy, L.pxy + L.nv, e);
        velocity_grad(L, myvel, e, M, M.det(), G);
      });
      s_wt[tid] = wt;
      for (int c = 0; c < 4; ++c) s_G[c][tid] = G[c];
    }
    F.features(S, k, nrows, V, false);          // no barrier yet: it follows the transform
    // the row chunk (side 0 of gram_features: the same idx -> (mode, point) map, so every lane reads what it wrote)
    for (int idx = tid; idx < GT * OC; idx += 256) {
      const int i = idx % OC, t = idx / OC;
      const double gxx = s_G[0][t], gxy = s_G[1][t], gyx = s_G[2][t], gyy = s_G[3][t];
      const double h = 0.5 * (gxx + gyy);
#pragma unroll
      for (int c = 0; c < NCOMP; ++c) {
        const double fx = s_f[0][NCOMP + 2 * c][t][i], fy = s_f[0][NCOMP + 2 * c + 1][t][i];
        s_f[0][c][t][i] *= h;
        s_f[0][NCOMP + 2 * c][t][i] = h * fx - (gxx * fx + gyx * fy);
        s_f[0][NCOMP + 2 * c + 1][t][i] = h * fy - (gxy * fx + gyy * fy);
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < GT; ++t) {
      double2 a[NF], b[NF];
      F.load(S, t, a, b);
      const double w = s_wt[t];                 // the same for every lane
      if constexpr (NCOMP == 2) {
        // features 0 hx, 1 hy, 2 dx hx, 3 dy hx, 4 dx hy, 5 dy hy (row chunk: transformed)
        GRAM_ACC(0, 3, 3, w) GRAM_ACC(0, 4, 4, w) GRAM_ACC(0, 2, 5, -w) GRAM_ACC(0, 5, 2, -w)
        GRAM_ACC(1, 2, 2, 1.0) GRAM_ACC(1, 5, 5, 1.0) GRAM_ACC(1, 3, 4, 1.0) GRAM_ACC(1, 4, 3, 1.0)
        GRAM_ACC(2, 0, 0, 1.0) GRAM_ACC(2, 1, 1, 1.0)
        GRAM_ACC(3, 0, 0, w) GRAM_ACC(3, 1, 1, w)
      } else {
        // features 0 u, 1 dx u, 2 dy u (row chunk: transformed)
        GRAM_ACC(0, 1, 1, 1.0) GRAM_ACC(0, 2, 2, 1.0)
        GRAM_ACC(1, 0, 0, 1.0)
        GRAM_ACC(2, 0, 0, w)
      }
    }
    __syncthreads();
  }
  F.store(partial, (int64_t)v * NOUT);
}

// Pass 4, after k_overlap_reduce: O[m] <- O[m] + O[m]^T in place, blockIdx.y = matrix.  One lane per pair i <= j reads both
// entries, adds them once and writes the one sum to both places: the matrices are bitwise symmetric.
__global__ __launch_bounds__(256) void k_velocity_symmetrise(int k, double* __restrict__ O) {
  O += (int64_t)blockIdx.y * k * k;
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < k * k; idx += 256 * gridDim.x) {
    const int i = idx / k, j = idx % k;
    if (i > j) continue;
    const double s = O[(int64_t)i * k + j] + O[(int64_t)j * k + i];
    O[(int64_t)i * k + j] = s;
    O[(int64_t)j * k + i] = s;
  }
}

// Posed flux overlap (plfem_flux_overlap_posed): the cross flux int (E_a x H_b + E_b x H_a) . z of two vectorial mode sets
// on two meshes under a pose, as the four sums the host needs, free of beta, k0 and m.  Pose, location and the turn of A's
// value are those of k_field_overlap_posed, operation for operation (xa, ya through mul_rn and an IEEE division; the
// identity pose gives (X, Y) bit for bit).  With hA' = R hA(xa, ya), gA' = R gA (g = -(hx,xx + hy,xy), -(hx,xy + hy,yy)
// from the physical Hessians of A's element, p2_basis_hess, as in k_flux_grams; no factor of m), hB and gB B's own at its
// quadrature point, wA = 1 / eps_A at (xa, ya) in A's frame and wB = 1 / eps_B at (X, Y):
//   MA[i][j] = sum wA (hA'_i . hB_j)    GA[i][j] = sum wA (gA'_i . hB_j)
//   MB[i][j] = sum wB (hA'_i . hB_j)    GB[i][j] = sum wB (hA'_i . gB_j)
// over B's elements and six-point rule with |det J| w_q.  Each side's material is discs or a layer profile (material_eps:
// in_any_core / profile_eps, the helpers of the assembly): four instances.  Sampled index maps are out of scope here: the
// entry point refuses a locator that carries one.  A point in no element of A has both weights 0 and contributes 0 to all
// four; a boundary DOF of an indexed record is skipped.
// Grid = (slice of B's tiles, chunk pair, pose of the batch) as in k_field_overlap_posed, gridDim.x a function of B's
// element count alone.  Tiles of FT = 32 points: the features -- hA', gA', hB, gB, two components each, for 32 modes per
// side -- are 64 KiB of LDS, 78 KiB with the staging, so two workgroups share a CU.  Per point pair a lane forms
// hA' . hB, gA' . hB and hA' . gB of its 2 x 2 block once, each as one product and one fused multiply-add in a written
// order, and adds them with the two weights (the same for every lane) to its four accumulator blocks: an entry's bits
// depend neither on its place in the block nor on the chunk.  Partials [pose][output][chunk pair][slice][OC * OC], every
// slot written: what k_overlap_reduce sums with blockIdx.y = 4 pose + output.  Outputs in the order MA, GA, MB, GB.
constexpr int FT = 32;                  // quadrature points per tile
constexpr int FLUX_POSED_OUTPUTS = 4;   // MA, GA, MB, GB

// one entry (r, s) of the lane's block: p, q pick the row / column mode of the double2 features
#define FLUX_POSED_ACC(r, s, p, q)                                          \
      {                                                                     \
        const double d = fma(a[0].p, b[0].q, a[1].p * b[1].q);              \
        const double ga = fma(a[2].p, b[0].q, a[3].p * b[1].q);             \
        const double gb = fma(a[0].p, b[2].q, a[1].p * b[3].q);             \
        acc[0][r][s] = fma(wa, d, acc[0][r][s]);                            \
        acc[1][r][s] = fma(wa, ga, acc[1][r][s]);                           \
        acc[2][r][s] = fma(wb, d, acc[2][r][s]);                            \
        acc[3][r][s] = fma(wb, gb, acc[3][r][s]);                           \
      }

template <bool PROFILE_A, bool PROFILE_B>
__global__ __launch_bounds__(256) void k_flux_overlap_posed(LocArgs A, LocArgs B, int ka, int64_t nrows_a,
                                                            const double* __restrict__ Va, Material mat_a, int kb,
                                                            int64_t nrows_b, const double* __restrict__ Vb, Material mat_b,
                                                            int nchunk_b, const double* __restrict__ poses,
                                                            double* __restrict__ partial) {
  __shared__ double s_fa[4][FT][OC];          // A's chunk: hA'x, hA'y, gA'x, gA'y
  __shared__ double s_fb[4][FT][OC];          // B's chunk: hBx, hBy, gBx, gBy
  __shared__ double s_phi[6][FT];             // A's basis at the located point
  __shared__ double s_ha[3][6][FT];           // xx, xy, yy of the six basis functions of A's element
  __shared__ double s_hb[3][6][FT];           // and of B's
  __shared__ int s_ra[6][FT], s_rb[6][FT];
  __shared__ double s_wa[FT], s_wb[FT];       // |det J| w_q / eps_A and / eps_B
  __shared__ int s_q[FT];
  const int tid = threadIdx.x;
  const int ca = blockIdx.y / nchunk_b, cb = blockIdx.y % nchunk_b;
  const int ia0 = ca * OC, jb0 = cb * OC;
  const double* pose = poses + (int64_t)blockIdx.z * POSE_DOUBLES;     // the same for every lane
  const double tx = pose[0], ty = pose[1], pc = pose[2], ps = pose[3], pm = pose[4];
  const int64_t nq = (int64_t)6 * B.ne;
  const int64_t ntiles = (nq + FT - 1) / FT;
  const int ti = tid >> 4, tj = tid & 15;
  const double* Va1 = Va + nrows_a * ka;
  const double* Vb1 = Vb + nrows_b * kb;
  double acc[FLUX_POSED_OUTPUTS][2][2];
#pragma unroll
  for (int o = 0; o < FLUX_POSED_OUTPUTS; ++o) acc[o][0][0] = acc[o][0][1] = acc[o][1][0] = acc[o][1][1] = 0.0;
  const double* pbx = B.pxy;
  const double* pby = B.pxy + B.nv;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (tid < FT) {
      const int64_t g = tile * FT + tid;
      double wa = 0.0, wb = 0.0;
      int q = 0;
      for (int a = 0; a < 6; ++a) {
        s_ra[a][tid] = -1; s_rb[a][tid] = -1; s_phi[a][tid] = 0.0;
        s_ha[0][a][tid] = s_ha[1][a][tid] = s_ha[2][a][tid] = 0.0;
        s_hb[0][a][tid] = s_hb[1][a][tid] = s_hb[2][a][tid] = 0.0;
      }
      if (g < nq) {
        const int e = (int)(g / 6);
        q = (int)(g % 6);
        const P2Map M(B.edof, B.ne, pbx, pby, e);
        double X, Y;
        M.point(c_qx[q], c_qy[q], X, Y);
        const double detb = M.det();
        const double dx = X - tx, dy = Y - ty;
        const double xa = (mul_rn(pc, dx) + mul_rn(ps, dy)) / pm;
        const double ya = (mul_rn(pc, dy) - mul_rn(ps, dx)) / pm;
        double axi, aeta, inva[4];
        const int ea = dev_locate(A, xa, ya, axi, aeta, inva);
        if (ea >= 0) {
          const double w = fabs(detb) * c_qw[q];
          const double eps_a = material_eps<PROFILE_A>(mat_a, xa, ya, PROFILE_A ? false : in_any_core(xa, ya, mat_a.cores.c, mat_a.ncore));
          const double eps_b = material_eps<PROFILE_B>(mat_b, X, Y, PROFILE_B ? false : in_any_core(X, Y, mat_b.cores.c, mat_b.ncore));
          wa = w * (1.0 / eps_a);
          wb = w * (1.0 / eps_b);
          double phi[6], hxx[6], hxy[6], hyy[6], invb[4];
          p2_phi(axi, aeta, phi);
          p2_basis_hess(inva, hxx, hxy, hyy);
          for (int a = 0; a < 6; ++a) {
            s_phi[a][tid] = phi[a];
            s_ha[0][a][tid] = hxx[a]; s_ha[1][a][tid] = hxy[a]; s_ha[2][a][tid] = hyy[a];
            s_ra[a][tid] = dev_row(A, ea, a);
            s_rb[a][tid] = dev_row(B, e, a);
          }
          M.inverse(detb, invb);
          p2_basis_hess(invb, hxx, hxy, hyy);
          for (int a = 0; a < 6; ++a) { s_hb[0][a][tid] = hxx[a]; s_hb[1][a][tid] = hxy[a]; s_hb[2][a][tid] = hyy[a]; }
        }
      }
      s_wa[tid] = wa;
      s_wb[tid] = wb;
      s_q[tid] = q;
    }
    __syncthreads();
    // the features of every (point, mode): a lane holds both components, so that it can turn A's h and g
    for (int idx = tid; idx < FT * OC; idx += 256) {
      const int i = idx % OC, t = idx / OC;
      const int q = s_q[t];
      const bool la = ia0 + i < ka, lb = jb0 + i < kb;
      double hax = 0.0, hay = 0.0, sax = 0.0, say = 0.0, hbx = 0.0, hby = 0.0, sbx = 0.0, sby = 0.0;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const int ra = s_ra[a][t], rb = s_rb[a][t];
        if (la && ra >= 0) {
          const double vx = Va[(int64_t)ra * ka + ia0 + i], vy = Va1[(int64_t)ra * ka + ia0 + i];
          const double ph = s_phi[a][t], hxy = s_ha[1][a][t];
          hax += ph * vx;
          hay += ph * vy;
          sax += s_ha[0][a][t] * vx + hxy * vy;
          say += hxy * vx + s_ha[2][a][t] * vy;
        }
        if (lb && rb >= 0) {
          const double vx = Vb[(int64_t)rb * kb + jb0 + i], vy = Vb1[(int64_t)rb * kb + jb0 + i];
          const double ph = p2_phi(a, c_qx[q], c_qy[q]), hxy = s_hb[1][a][t];   // B's basis at its own quadrature point q
          hbx += ph * vx;
          hby += ph * vy;
          sbx += s_hb[0][a][t] * vx + hxy * vy;
          sby += hxy * vx + s_hb[2][a][t] * vy;
        }
      }
      const double gax = -sax, gay = -say;
      s_fa[0][t][i] = mul_rn(pc, hax) - mul_rn(ps, hay);
      s_fa[1][t][i] = mul_rn(ps, hax) + mul_rn(pc, hay);
      s_fa[2][t][i] = mul_rn(pc, gax) - mul_rn(ps, gay);
      s_fa[3][t][i] = mul_rn(ps, gax) + mul_rn(pc, gay);
      s_fb[0][t][i] = hbx;
      s_fb[1][t][i] = hby;
      s_fb[2][t][i] = -sbx;
      s_fb[3][t][i] = -sby;
    }
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < FT; ++t) {
      double2 a[4], b[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        a[c] = *reinterpret_cast<const double2*>(&s_fa[c][t][2 * ti]);
        b[c] = *reinterpret_cast<const double2*>(&s_fb[c][t][2 * tj]);
      }
      const double wa = s_wa[t], wb = s_wb[t];  // the same for every lane
      FLUX_POSED_ACC(0, 0, x, x) FLUX_POSED_ACC(0, 1, x, y)
      FLUX_POSED_ACC(1, 0, y, x) FLUX_POSED_ACC(1, 1, y, y)
    }
    __syncthreads();
  }
  const int64_t npair = (int64_t)gridDim.y;
#pragma unroll
  for (int o = 0; o < FLUX_POSED_OUTPUTS; ++o) {
    double* out = partial + ((((int64_t)blockIdx.z * FLUX_POSED_OUTPUTS + o) * npair + blockIdx.y) * gridDim.x + blockIdx.x) * (OC * OC);
    for (int r = 0; r < 2; ++r)
      for (int s = 0; s < 2; ++s) out[(2 * ti + r) * OC + 2 * tj + s] = acc[o][r][s];
  }
}
#undef FLUX_POSED_ACC

// Coordinate-weighted Grams (plfem_moment_grams): the M_r (and K_r) of k_mode_grams weighted by the point's X = x - ox,
// Y = y - oy, and the unweighted M by X^2, XY, Y^2.  Grid, tiling, staging and features as in k_mode_grams; the staging
// lanes also put X, Y, X^2, XY, Y^2 of their point into LDS (0 for a padding point, whose weight is 0).  Per point every
// lane forms the unweighted 2 x 2 products of its block once -- m = u u' (hx hx' + hy hy') or kk = the form of K_r -- and
// adds them, times the point's coordinates, to the outputs of the point's region: the coordinates and the region are
// the same for every lane.  Every product and sum is an explicit multiply or fused multiply-add in one written order,
// the same for the four entries of the block, so an entry's bits do not depend on its place in the block or the chunk.
// KPART = false: the seven outputs made of m (M_core_X, M_core_Y, M_clad_X, M_clad_Y, M_XX, M_XY, M_YY: all of the
// scalar call); KPART = true (NCOMP = 2): the four made of kk (K_core_X, K_core_Y, K_clad_X, K_clad_Y).  The vectorial
// call runs both instances: 11 outputs x 4 accumulators do not fit 128 VGPRs beside the features.  Partials
// [output][chunk pair][workgroup][OC * OC] at the outputs' places in the call's list, every slot written.
template <int NCOMP, bool KPART>
__global__ __launch_bounds__(256) void k_moment_grams(LocArgs L, int k, int64_t nrows, const double* __restrict__ V,
                                                      CoreTable cores, int ncore, double ox, double oy, int nchunk,
                                                      double* __restrict__ partial) {
  static_assert(NCOMP == 2 || !KPART, "the scalar call has no K");
  constexpr int NF = 3 * NCOMP;
  constexpr int NOUT = KPART ? 4 : 7;
  __shared__ GramTile<NCOMP> S;
  __shared__ double s_mx[5][GT];              // X, Y, X^2, XY, Y^2 of the tile's points
  __shared__ int s_core[GT];
  GramFrame<NCOMP, NOUT> F(nchunk);
  double (&acc)[NOUT][2][2] = F.acc;
  const int tid = F.tid;
  const int64_t nq = (int64_t)6 * L.ne;
  const int64_t ntiles = (nq + GT - 1) / GT;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (tid < GT) {
      const int64_t g = tile * GT + tid;
      int core = 0;
      double X = 0.0, Y = 0.0;
      gram_stage_point(L, g, g < nq, tid, S, [&](double x, double y) {
        core = in_any_core(x, y, cores.c, ncore) ? 1 : 0;
        X = x - ox;
        Y = y - oy;
      });
      s_core[tid] = core;
      s_mx[0][tid] = X;
      s_mx[1][tid] = Y;
      s_mx[2][tid] = mul_rn(X, X);
      s_mx[3][tid] = mul_rn(X, Y);
      s_mx[4][tid] = mul_rn(Y, Y);
    }
    F.features(S, k, nrows, V);
#pragma unroll 1
    for (int t = 0; t < GT; ++t) {
      constexpr int C0 = KPART ? 2 : 0, C1 = KPART ? NF : NCOMP;   // the features this instance reads
      double2 a[NF], b[NF];
      F.template load<C0, C1>(S, t, a, b);
      const double X = s_mx[0][t], Y = s_mx[1][t];
      const bool core = s_core[t] != 0;         // the same for every lane
      double p[2][2];
      if constexpr (KPART) gram_k_block(a, b, p);
      else gram_m_block<NCOMP>(a, b, p);
      if (core) { GRAM_WACC(0, X, p) GRAM_WACC(1, Y, p) } else { GRAM_WACC(2, X, p) GRAM_WACC(3, Y, p) }
      if constexpr (!KPART) {
        const double XX = s_mx[2][t], XY = s_mx[3][t], YY = s_mx[4][t];
        GRAM_WACC(4, XX, p) GRAM_WACC(5, XY, p) GRAM_WACC(6, YY, p)
      }
    }
    __syncthreads();
  }
  // the output's place in the call's list
  F.store(partial, 0, [](int o) { return KPART ? 4 + o : (o < 4 ? o : 4 * NCOMP + (o - 4)); });
}

// Tangent Grams of a profile solve (plfem_profile_tangent_grams): the M_w (and K_w) of k_profile_grams under a batch of
// point weights ("columns") in place of w -- the first-order change dw of w along a tangent of the profile's values, or
// w X, w Y for a bend -- in two kernels per group of NW columns.
//
// The pre-pass, k_profile_point_weights: one lane per quadrature point of the six-point rule, element-major; the point
// formed as the assembly forms it (P2Map::point).  The lane walks the layer table once (profile_top_layer: the topmost
// layer and t^g), finds the cell and the bilinear weights of the map (sampled_cell) where there is one and no layer
// holds the point, forms eps with the bits of profile_eps and w = 1 / eps (NCOMP = 2) or eps (NCOMP = 1) as
// k_profile_grams does, and then writes one weight per column c0 .. c0 + NW - 1 of the group to wbuf[column][point]:
//   a tangent t (row[1 + 2 nlayer] = d_eps_bg, then (d_a, d_b) per layer; tmap_of[t] its map among tmaps, or -1):
//     d_eps = layer_value(d_a, d_b) of the topmost layer, or the bilinear interpolant of its map in the cell, or row[0];
//     the weight is -(d_eps w) w (NCOMP = 2), d_eps (NCOMP = 1), every product rounded on its own;
//   with `moments`, columns ntan and ntan + 1: w X and w Y, X = x - ox, Y = y - oy;
//   a column past the call's last: 0.
// A column's weight depends on the point and the column alone, not on the group it is in.  The rows are gathered at
// the lane's own layer; the walk is over indices every lane shares (uniform loads).
template <int NCOMP, int NW, typename... Map>
__global__ __launch_bounds__(256) void k_profile_point_weights(LocArgs L, const double* __restrict__ layers, int nlayer,
                                                               double eps_bg, const double* __restrict__ tangents,
                                                               const int32_t* __restrict__ tmap_of,
                                                               const double* __restrict__ tmaps, int ntan, int c0, int moments,
                                                               double ox, double oy, double* __restrict__ wbuf, Map... map) {
  const int64_t nq = (int64_t)6 * L.ne;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= nq) return;
  const int e = (int)(g / 6), q = (int)(g % 6);
  const P2Map M(L.edof, L.ne, L.pxy, L.pxy + L.nv, e);
  double X, Y, tg;
  M.point(c_qx[q], c_qy[q], X, Y);
  const int top = profile_top_layer(X, Y, layers, nlayer, tg);
  const double gl = top >= 0 ? layers[LAYER_DOUBLES * top + 6] : 0.0;
  [[maybe_unused]] bool in_map = false;
  [[maybe_unused]] int i0 = 0, j0 = 0, nx = 0, ny = 0;
  [[maybe_unused]] double a = 0.0, b = 0.0;
  double eps = eps_bg;
  if constexpr (sizeof...(Map) == 1) {
    const EpsMap& em = (map, ...);
    const SampledGrid G = em.grid();
    nx = G.nx;
    ny = G.ny;
    in_map = sampled_cell(G, X, Y, i0, j0, a, b);
    if (in_map && top < 0) eps = map_bilinear(em.eps(), nx, i0, j0, a, b);
  }
  if (top >= 0) eps = layer_value(layers[LAYER_DOUBLES * top + 4], layers[LAYER_DOUBLES * top + 5], gl, tg);
  const double w = NCOMP == 2 ? 1.0 / eps : eps;
  const int nrow = 1 + 2 * nlayer;
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    const int c = c0 + j;
    double v = 0.0;
    if (c < ntan) {
      const double* row = tangents + (int64_t)c * nrow;
      double d = row[0];
      if (top >= 0) {
        d = layer_value(row[1 + 2 * top], row[2 + 2 * top], gl, tg);
      } else if constexpr (sizeof...(Map) == 1) {
        const int mi = tmap_of[c];
        if (in_map && mi >= 0) d = map_bilinear(tmaps + (int64_t)mi * nx * ny, nx, i0, j0, a, b);
      }
      v = NCOMP == 2 ? -mul_rn(mul_rn(d, w), w) : d;
    } else if (moments && c < ntan + 2) {
      v = mul_rn(w, c == ntan ? X - ox : Y - oy);
    }
    wbuf[(int64_t)j * nq + g] = v;
  }
}

// The Gram kernel, k_weighted_grams: grid, tiling, staging and features of k_mode_grams; the weights of the tile's
// points come from the pre-pass (NW x GT loads by lanes of the second wave, beside the staging lanes of the first; 0 for
// a padding point).  Per point every lane forms the unweighted 2 x 2 products of its block once, as k_moment_grams
// does -- m = u u' (hx hx' + hy hy') and, NCOMP = 2, kk = the form of K_r -- and adds them, times the column's weight,
// to the column's outputs: M_col (and K_col).  Every product and sum is an explicit multiply or fused multiply-add in one
// written order, the same for the four entries of the block and for every column, so an entry's bits depend neither on
// its place in the block nor on the column's place in the group.  Partials [column of the group][output][chunk pair]
// [workgroup][OC * OC], every slot written.
template <int NCOMP, int NW>
__global__ __launch_bounds__(256) void k_weighted_grams(LocArgs L, int k, int64_t nrows, const double* __restrict__ V,
                                                        const double* __restrict__ wbuf, int nchunk,
                                                        double* __restrict__ partial) {
  static_assert(NW * GT <= 192, "the weights are loaded by lanes GT .. of one pass");
  constexpr int NF = 3 * NCOMP;
  constexpr int NOUT = NCOMP == 2 ? 2 : 1;
  __shared__ GramTile<NCOMP> S;
  __shared__ double s_wt[NW][GT];             // the columns' weights of the point
  GramFrame<NCOMP, NW * NOUT> F(nchunk);      // output o of column c at c NOUT + o: the slot order
  double (&acc)[NW * NOUT][2][2] = F.acc;
  const int tid = F.tid;
  const int64_t nq = (int64_t)6 * L.ne;
  const int64_t ntiles = (nq + GT - 1) / GT;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (tid < GT) {
      const int64_t g = tile * GT + tid;
      gram_stage_point(L, g, g < nq, tid, S, [](double, double) {});
    } else if (tid >= 64 && tid < 64 + NW * GT) {
      const int c = (tid - 64) / GT, t = (tid - 64) % GT;
      const int64_t g = tile * GT + t;
      s_wt[c][t] = g < nq ? wbuf[(int64_t)c * nq + g] : 0.0;
    }
    F.features(S, k, nrows, V);
#pragma unroll 1
    for (int t = 0; t < GT; ++t) {
      double p[2][2];
      {
        double2 a[NF], b[NF];
        F.template load<0, NCOMP>(S, t, a, b);
        gram_m_block<NCOMP>(a, b, p);
      }
#pragma unroll
      for (int c = 0; c < NW; ++c) {
        const double wt = s_wt[c][t];           // the same for every lane
        GRAM_WACC(c * NOUT, wt, p)
      }
      if constexpr (NCOMP == 2) {
        double2 a[NF], b[NF];
        F.template load<2, NF>(S, t, a, b);
        gram_k_block(a, b, p);
#pragma unroll
        for (int c = 0; c < NW; ++c) {
          const double wt = s_wt[c][t];
          GRAM_WACC(c * NOUT + NOUT - 1, wt, p)
        }
      }
    }
    __syncthreads();
  }
  F.store(partial, 0);
}
#undef GRAM_ACC
#undef GRAM_WACC

// Pixel densities of a sampled map (plfem_index_map_gradients): the derivative of the diagonal of M_w (and K_w) of
// k_profile_grams in the value of every pixel of the locator's map -- the adjoint of the bilinear interpolant of
// profile_eps, one pass over the quadrature points whatever the number of pixels.  A point CONTRIBUTES when it lies in
// the closed extent of the map and no layer holds it; it then adds c = |det J| w_q dw, dw = -(w w) (NCOMP = 2) or 1
// (NCOMP = 1), times a density of the field -- m = hx^2 + hy^2 (u^2), kk = the form of K_r at m = n -- times a corner
// weight to the four nodes of its cell.  No floating-point atomics: the points are sorted by cell and every node sums
// its own lists in a fixed order.
//
// k_map_point_keys: one lane per quadrature point, the walk of k_profile_point_weights.  key = j0 (nx - 1) + i0 of a
// contributing point, (nx - 1)(ny - 1) -- past every cell, so it sorts last -- of any other; val = the point; (a, b) the
// weights of sampled_cell and c as above (0 where the point does not contribute).
template <int NCOMP>
__global__ __launch_bounds__(256) void k_map_point_keys(LocArgs L, const double* __restrict__ layers, int nlayer,
                                                        uint32_t* __restrict__ key, uint32_t* __restrict__ val,
                                                        double* __restrict__ pa, double* __restrict__ pb,
                                                        double* __restrict__ pc, EpsMap em) {
  const int64_t nq = (int64_t)6 * L.ne;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= nq) return;
  const int e = (int)(g / 6), q = (int)(g % 6);
  const P2Map M(L.edof, L.ne, L.pxy, L.pxy + L.nv, e);
  double X, Y, tg;
  M.point(c_qx[q], c_qy[q], X, Y);
  const int top = profile_top_layer(X, Y, layers, nlayer, tg);
  const SampledGrid G = em.grid();
  int i0 = 0, j0 = 0;
  double a = 0.0, b = 0.0, c = 0.0;
  uint32_t kk = (uint32_t)(G.nx - 1) * (uint32_t)(G.ny - 1);
  if (sampled_cell(G, X, Y, i0, j0, a, b) && top < 0) {
    const double eps = map_bilinear(em.eps(), G.nx, i0, j0, a, b);
    const double w = NCOMP == 2 ? 1.0 / eps : eps;
    const double dw = NCOMP == 2 ? -mul_rn(w, w) : 1.0;
    c = mul_rn(mul_rn(fabs(M.det()), c_qw[q]), dw);
    kk = (uint32_t)j0 * (uint32_t)(G.nx - 1) + (uint32_t)i0;
  } else {
    a = b = 0.0;
  }
  key[g] = kk;
  val[g] = (uint32_t)g;
  pa[g] = a;
  pb[g] = b;
  pc[g] = c;
}

// k_map_cell_ranges: one lane per place p of the sorted keys; where a cell's run begins (ends) it writes first[cell]
// (last[cell], one past).  The arrays are zeroed before: a cell no point lies in keeps the empty range [0, 0).
__global__ __launch_bounds__(256) void k_map_cell_ranges(int64_t nq, uint32_t ncell, const uint32_t* __restrict__ skey,
                                                         int32_t* __restrict__ first, int32_t* __restrict__ last) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= nq) return;
  const uint32_t kk = skey[p];
  if (kk >= ncell) return;
  if (p == 0 || skey[p - 1] != kk) first[kk] = (int32_t)p;
  if (p == nq - 1 || skey[p + 1] != kk) last[kk] = (int32_t)(p + 1);
}

// k_point_densities: one lane per quadrature point, element-major, for the fields f0 .. f0 + nf - 1 of the call: the
// features of the Gram kernels at the point (P2Map, p2_grad, p2_phi; the staged rows of dev_row) and from them
// dens[f][0][g] = m, dens[f][1][g] = kk (NCOMP = 2).  Every sum is a chain of explicit fused multiply-adds in one written
// order, and the fields are walked by a loop that is not unrolled: a field's bits do not depend on its place in the call.
// A point that does not contribute (key = ncell) is skipped: no list holds it, so its slots are never read.
constexpr int MAPG_FC = 16;     // fields per chunk: 32 accumulators per lane of k_map_gather

template <int NCOMP>
__global__ __launch_bounds__(256) void k_point_densities(LocArgs L, int k, int64_t nrows, const double* __restrict__ V, int f0,
                                                         int nf, uint32_t ncell, const uint32_t* __restrict__ key,
                                                         double* __restrict__ dens) {
  constexpr int NOUT = NCOMP == 2 ? 2 : 1;
  const int64_t nq = (int64_t)6 * L.ne;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= nq || key[g] >= ncell) return;
  const int e = (int)(g / 6), q = (int)(g % 6);
  const P2Map M(L.edof, L.ne, L.pxy, L.pxy + L.nv, e);
  const double xi = c_qx[q], eta = c_qy[q];
  double inv[4], gx[6], gy[6], phi[6];
  M.inverse(M.det(), inv);
  p2_grad(inv, xi, eta, gx, gy);
  p2_phi(xi, eta, phi);
  int64_t row[6];
  dev_row_offsets(L, e, k, row);
#pragma unroll 1
  for (int f = 0; f < nf; ++f) {
    const int m = f0 + f;
    double u[NCOMP], ux[NCOMP], uy[NCOMP];
#pragma unroll
    for (int c = 0; c < NCOMP; ++c) {
      u[c] = ux[c] = uy[c] = 0.0;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const double v = row[a] < 0 ? 0.0 : V[(int64_t)c * nrows * k + row[a] + m];
        u[c] = fma(phi[a], v, u[c]);
        ux[c] = fma(gx[a], v, ux[c]);
        uy[c] = fma(gy[a], v, uy[c]);
      }
    }
    double mm = mul_rn(u[0], u[0]);
    if constexpr (NCOMP == 2) {
      mm = fma(u[1], u[1], mm);
      // dy hx dy hx + dx hy dx hy - dx hx dy hy - dy hy dx hx at m = n
      double kk = mul_rn(uy[0], uy[0]);
      kk = fma(ux[1], ux[1], kk);
      kk = fma(-ux[0], uy[1], kk);
      kk = fma(-uy[1], ux[0], kk);
      dens[((int64_t)f * NOUT + 1) * nq + g] = kk;
    }
    dens[((int64_t)f * NOUT) * nq + g] = mm;
  }
}

// k_map_gather: one wavefront per map node (four per workgroup) for the nf fields of the chunk.  The node (j, i) is a
// corner of up to four cells, walked in ascending key: (j - 1, i - 1) with the corner weight a b, (j - 1, i) with a1 b,
// (j, i - 1) with a b1, (j, i) with a1 b1 (a1 = 1 - a, b1 = 1 - b, every product rounded on its own).  Lane l takes the
// places first + l, first + l + 64, .. of each cell's run of the sorted points -- ascending point order -- and adds
// (c beta) dens by fused multiply-adds; the fixed butterfly of multi_reduce sums the lanes.  A field's sum depends on
// the node's lists alone: the same bits whatever other fields share the chunk, in any place of it.  A node whose four
// runs are empty writes nothing: the result and the support are zeroed before the launch.  support = the runs' lengths.
template <int NCOMP>
__global__ __launch_bounds__(256) void k_map_gather(int nx, int ny, int64_t nq, int nf, const int32_t* __restrict__ first,
                                                    const int32_t* __restrict__ last, const uint32_t* __restrict__ sval,
                                                    const double* __restrict__ pa, const double* __restrict__ pb,
                                                    const double* __restrict__ pc, const double* __restrict__ dens,
                                                    double* __restrict__ out, int32_t* __restrict__ support) {
  constexpr int NOUT = NCOMP == 2 ? 2 : 1;
  constexpr int NV = MAPG_FC * NOUT;
  const int lane = threadIdx.x & 63;
  const int64_t npix = (int64_t)nx * ny;
  const int64_t node = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (node >= npix) return;                   // (the whole wavefront)
  const int j = (int)(node / nx), i = (int)(node % nx);
  int lo[4], hi[4], total = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int cj = j - 1 + (s >> 1), ci = i - 1 + (s & 1);
    lo[s] = hi[s] = 0;
    if (cj >= 0 && cj < ny - 1 && ci >= 0 && ci < nx - 1) {
      const int64_t cell = (int64_t)cj * (nx - 1) + ci;
      lo[s] = first[cell];
      hi[s] = last[cell];
    }
    total += hi[s] - lo[s];
  }
  if (total == 0) return;
  double acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = 0.0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    for (int p = lo[s] + lane; p < hi[s]; p += 64) {
      const int64_t g = sval[p];
      const double a = pa[g], b = pb[g];
      const double wa = (s & 1) ? 1.0 - a : a, wb = (s >> 1) ? 1.0 - b : b;
      const double cb = mul_rn(pc[g], mul_rn(wa, wb));
#pragma unroll
      for (int v = 0; v < NV; ++v)
        if (v < nf * NOUT) acc[v] = fma(cb, dens[(int64_t)v * nq + g], acc[v]);
    }
  }
  multi_reduce<NV>(acc, lane);
  const int v = multi_reduce_index<NV>(lane);
  if (lane < NV && v < nf * NOUT) out[(int64_t)v * npix + node] = acc[0];
  if (support && lane == 0) support[node] = total;
}

// Quartic mode-overlap tensor (plfem_mode_quartic): Q[p(i,j)][p(l,m)] = sum over the points of the 16-point degree-8 rule
// of |det J| w_q wt(x) (u_i . u_j)(u_l . u_m), i.e. Q = R^T diag(w) R with R[point][pair] = u_i . u_j.  R never reaches
// HBM: one workgroup owns one 64 x 64 tile of Q on or above the diagonal (blockIdx.y, upper-triangle order) and walks
// the elements blockIdx.x, blockIdx.x + gridDim.x, ...  Per element: the six staged DOF rows of all k modes go to LDS;
// u[c][t][m] = sum_a phi_a(q_t) v[c][a][m] at the 16 points (the basis at the rule's points is one table, no J^-1);
// the pair products of the tile's 64 row pairs (plain) and 64 column pairs (times the point's weight) go to LDS as the
// A and B operands of v_mfma_f64_16x16x4_f64; each wave accumulates a 32 x 32 block (2 x 2 MFMA tiles) over the 16
// points in four K-steps.  No region branch sits in the reduction: the weight is folded into B.  The workgroup's
// partial tile goes to its own slot (no atomics); k_quartic_reduce sums the slots in a fixed order.
constexpr int QP = 64;          // pairs per side of an output tile
constexpr int QKMAX = 64;       // most modes per call (LDS rows of the element)
constexpr int QB_MAX = 128;     // most element slices (partial tiles) per output tile
constexpr int QWG = 2048;       // most partial tiles in all: slices = min(QB_MAX, QWG / tile pairs)
constexpr int QLD = QP + 2;     // padded LDS row of the pair products

typedef double dbl4 __attribute__((ext_vector_type(4)));

// upper-triangle tile pair t -> (ti, tj), ti <= tj, over an nt x nt tiling
__device__ __forceinline__ void quartic_tile(int t, int nt, int& ti, int& tj) {
  ti = 0;
  while (t >= nt - ti) { t -= nt - ti; ++ti; }
  tj = ti + t;
}

template <int NCOMP>
__global__ __launch_bounds__(256) void k_mode_quartic(LocArgs L, int k, int64_t nrows, const double* __restrict__ V,
                                                      CoreTable cores, int ncore, double w_core, double w_clad, int npair,
                                                      int ntile, double* __restrict__ partial) {
  __shared__ double s_v[NCOMP][6][QKMAX];     // the element's DOF rows (0 for a boundary DOF of an indexed record)
  __shared__ double s_u[NCOMP][16][QKMAX + 1];
  __shared__ double s_r[2][16][QLD];          // [0]: row pairs' products, [1]: column pairs' products times the weight
  __shared__ double s_phi[16][6];
  __shared__ double s_w[16];
  __shared__ int s_pi[2][QP], s_pj[2][QP];    // modes (i, j) of the tile's row / column pairs; -1 past np
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int ti, tj;
  quartic_tile(blockIdx.y, ntile, ti, tj);
  if (tid < 2 * QP) {
    const int side = tid / QP, a = tid % QP;
    const int P = (side ? tj : ti) * QP + a;
    int i = -1, j = -1;
    if (P < npair) {
      int r = P;
      i = 0;
      while (r >= k - i) { r -= k - i; ++i; }
      j = i + r;
    }
    s_pi[side][a] = i;
    s_pj[side][a] = j;
  }
  if (tid < 96) s_phi[tid / 6][tid % 6] = p2_phi(tid % 6, c_q16x[tid / 6], c_q16y[tid / 6]);
  const double* px = L.pxy;
  const double* py = L.pxy + L.nv;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;   // this wave's 32 x 32 block of the tile
  const int l16 = lane & 15, l4 = lane >> 4;
  dbl4 acc[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int s = 0; s < 2; ++s) acc[r][s] = dbl4{0.0, 0.0, 0.0, 0.0};
  for (int e = blockIdx.x; e < L.ne; e += gridDim.x) {
    for (int idx = tid; idx < NCOMP * 6 * QKMAX; idx += 256) {
      const int m = idx % QKMAX, a = (idx / QKMAX) % 6, c = idx / (6 * QKMAX);
      double v = 0.0;
      if (m < k) {
        const int r = dev_row(L, e, a);
        if (r >= 0) v = V[(int64_t)c * nrows * k + (int64_t)r * k + m];
      }
      s_v[c][a][m] = v;
    }
    if (tid < 16) {
      const P2Map M(L.edof, L.ne, px, py, e);
      double w = fabs(M.det()) * c_q16w[tid];
      if (ncore >= 0) {
        double X, Y;
        M.point(c_q16x[tid], c_q16y[tid], X, Y);
        w *= in_any_core(X, Y, cores.c, ncore) ? w_core : w_clad;
      }
      s_w[tid] = w;
    }
    __syncthreads();
    for (int idx = tid; idx < NCOMP * 16 * QKMAX; idx += 256) {
      const int m = idx % QKMAX, t = (idx / QKMAX) % 16, c = idx / (16 * QKMAX);
      double u = 0.0;
#pragma unroll
      for (int a = 0; a < 6; ++a) u += s_phi[t][a] * s_v[c][a][m];
      s_u[c][t][m] = u;
    }
    __syncthreads();
    for (int idx = tid; idx < 2 * 16 * QP; idx += 256) {
      const int a = idx % QP, t = (idx / QP) % 16, side = idx / (16 * QP);
      const int i = s_pi[side][a], j = s_pj[side][a];
      double r = 0.0;
      if (i >= 0) {
#pragma unroll
        for (int c = 0; c < NCOMP; ++c) r += s_u[c][t][i] * s_u[c][t][j];
        if (side) r *= s_w[t];
      }
      s_r[side][t][a] = r;
    }
    __syncthreads();
    // A[row][kk] = R[t = 4 ks + kk][row pair], B[kk][col] = w R[t][col pair]; lane: row / col = lane & 15, kk = lane >> 4
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int t = 4 * ks + l4;
      const double a0 = s_r[0][t][wr + l16], a1 = s_r[0][t][wr + 16 + l16];
      const double b0 = s_r[1][t][wc + l16], b1 = s_r[1][t][wc + 16 + l16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
  // D of v_mfma_f64_16x16x4_f64: entry g of a lane is (row (lane >> 4) + 4 g, col lane & 15)
  double* out = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (QP * QP);
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int g = 0; g < 4; ++g) out[(wr + 16 * r + l4 + 4 * g) * QP + wc + 16 * s + l16] = acc[r][s][g];
}

// Second stage of k_mode_quartic: blockIdx.x = tile pair, its nblk partial tiles summed in slice order (one lane per
// entry, the same bits on every run); entries with P <= P' < np are written to O[P][P'] and mirrored to O[P'][P], so the
// np x np result is exactly symmetric.  blockIdx.z = slice of the tile's entries.
__global__ __launch_bounds__(256) void k_quartic_reduce(int npair, int ntile, int nblk, const double* __restrict__ partial,
                                                        double* __restrict__ O) {
  int ti, tj;
  quartic_tile(blockIdx.x, ntile, ti, tj);
  const double* pp = partial + (int64_t)blockIdx.x * nblk * (QP * QP);
  for (int v = blockIdx.z * 256 + threadIdx.x; v < QP * QP; v += 256 * gridDim.z) {
    const int P = ti * QP + v / QP, P2 = tj * QP + v % QP;
    if (P2 >= npair || P > P2) continue;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += pp[(int64_t)b * (QP * QP) + v];
    O[(int64_t)P * npair + P2] = s;
    O[(int64_t)P2 * npair + P] = s;
  }
}

// Projection of the modes on separable analytic fields (plfem_mode_project): a factor (c, s, kappa) is
// phi(t) = exp(-s (t - c)^2) (cos(kappa t) - i sin(kappa t)) -- s = 0: a plane wave, the Gaussian part exactly 1 -- and
//   P[field][b][a] = sum over the elements and the 16 points of |det J| w_q u_field(x_q) phi(X_q; xfac_a) phi(Y_q; yfac_b),
// field = (component, mode).  A real GEMM over the quadrature points whose operands are generated on the fly: rows
// (field, x-factor, re | im) of value u phi_x, columns (y-factor, re | im) of value |det J| w phi_y.  One workgroup
// owns, for ALL fields, the tile of PJ_X x-factors (blockIdx.x % ntx) against PJ_Y y-factors (blockIdx.x / ntx) and walks
// the elements blockIdx.y, blockIdx.y + gridDim.y, ...  Per element: the six staged DOF rows of every field go to LDS
// and u at the 16 points follows from one basis table, as in k_mode_quartic; thread (point, factor of the tile)
// evaluates its factor at its point with the full-precision sincos / exp -- 16 (PJ_X + PJ_Y) = 256 evaluations, one per
// thread, shared by all fields -- and stores re, im (the y-factors times the point's weight).  The 16 rows of one field
// are then u[field][t] times the SAME 16 x-values (x-factor a, re: row a; im: row PJ_X + a), so a lane keeps its x-value
// and its B operand in registers per K-step and forms the A operand of each field with one broadcast LDS read and
// one product; wave w accumulates the 16 x 16 tiles of the fields w, w + 4, ... on v_mfma_f64_16x16x4_f64.  The factor
// values are double-buffered, so two barriers per element suffice.  The workgroup's partial tiles
// [field][row][column] go to its own slot (no atomics); k_project_reduce sums the slots in a fixed order and combines
// the four real products: re = RR - II, im = RI + IR.
constexpr int PJ_X = 8;          // x-factors per tile: 16 rows per field
constexpr int PJ_Y = 8;          // y-factors per tile: 16 columns
constexpr int PJ_KMAX = 64;      // most modes per call
constexpr int PJ_LMAX = 4096;    // most x- or y-factors per call
constexpr int PJ_SLICES = 256;   // most element slices (partial tiles) per tile
constexpr int PJ_WG = 1024;      // workgroups aimed at: slices = min(PJ_SLICES, PJ_WG / tiles), at least 1
constexpr int PJ_LD = 17;        // padded LDS row of the factor values

template <int MAXT>              // most fields per wave: ncomp k <= 4 MAXT
__global__ __launch_bounds__(256) void k_mode_project(LocArgs L, int ncomp, int k, int64_t nrows, const double* __restrict__ V,
                                                      int la, const double* __restrict__ xfac, int lb,
                                                      const double* __restrict__ yfac, int ntx, double* __restrict__ partial) {
  constexpr int FMAX = 4 * MAXT;
  __shared__ double s_v[6][FMAX];              // the element's DOF rows (0 for a boundary DOF of an indexed record)
  __shared__ double s_u[16][FMAX + 1];
  __shared__ double s_f[2][2][16][PJ_LD];      // [buffer][x | y][factor, re: + 0, im: + 8][point]
  __shared__ double s_phi[16][6];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nf = ncomp * k;
  const int ta = blockIdx.x % ntx, tb = blockIdx.x / ntx;
  // this thread's factor of the tile and its point
  const int pt = tid & 15, fj = tid >> 4;
  const bool isy = fj >= PJ_X;
  const int fi = isy ? tb * PJ_Y + (fj - PJ_X) : ta * PJ_X + fj;
  const bool live = fi < (isy ? lb : la);      // past the table: the row / column is 0
  const double* fp = (isy ? yfac : xfac) + 3 * (live ? fi : 0);
  const double fc = fp[0], fs = fp[1], fk = fp[2];
  const int frow = isy ? fj - PJ_X : fj;
  if (tid < 96) s_phi[tid / 6][tid % 6] = p2_phi(tid % 6, c_q16x[tid / 6], c_q16y[tid / 6]);
  for (int idx = tid; idx < 16 * (FMAX + 1); idx += 256) (&s_u[0][0])[idx] = 0.0;   // (the columns past nf stay 0)
  const double* px = L.pxy;
  const double* py = L.pxy + L.nv;
  const int l16 = lane & 15, l4 = lane >> 4;
  dbl4 acc[MAXT];
#pragma unroll
  for (int i = 0; i < MAXT; ++i) acc[i] = dbl4{0.0, 0.0, 0.0, 0.0};
  // This thread's entries of the element's DOF rows and the element's map are fetched one element ahead: the dependent
  // global loads (edof, int_index, the mode row; the vertices, their coordinates) then overlap the u and MFMA phases of the
  // element before.  (blockIdx.y < ne: the host launches no more slices than elements.)
  constexpr int NV = (6 * FMAX + 255) / 256;
  double vn[NV];
  auto fetch_rows = [&](int e) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int idx = tid + 256 * j;
      vn[j] = 0.0;
      if (idx < 6 * nf) {
        const int f = idx % nf, r = dev_row(L, e, idx / nf);
        if (r >= 0) vn[j] = V[((int64_t)(f / k) * nrows + r) * k + f % k];
      }
    }
  };
  fetch_rows(blockIdx.y);
  P2Map Mn(L.edof, L.ne, px, py, blockIdx.y);
  int buf = 0;
  for (int e = blockIdx.y; e < L.ne; e += gridDim.y, buf ^= 1) {
    const P2Map M = Mn;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int idx = tid + 256 * j;
      if (idx < 6 * nf) s_v[idx / nf][idx % nf] = vn[j];
    }
    {
      double X, Y, re = 0.0, im = 0.0;
      M.point(c_q16x[pt], c_q16y[pt], X, Y);
      if (live) {
        const double t = isy ? Y : X;
        double sn, cs, g = 1.0;
        sincos(mul_rn(fk, t), &sn, &cs);        // the phase is the single rounded product
        if (fs != 0.0) {
          const double d = t - fc;
          g = exp(-mul_rn(fs, mul_rn(d, d)));
        }
        if (isy) g *= fabs(M.det()) * c_q16w[pt];
        re = g * cs;
        im = -(g * sn);
      }
      s_f[buf][isy][frow][pt] = re;
      s_f[buf][isy][8 + frow][pt] = im;
    }
    __syncthreads();
    if (e + (int)gridDim.y < L.ne) {
      fetch_rows(e + gridDim.y);
      Mn = P2Map(L.edof, L.ne, px, py, e + gridDim.y);
    }
    for (int idx = tid; idx < 16 * nf; idx += 256) {
      const int f = idx % nf, t = idx / nf;
      double u = 0.0;
#pragma unroll
      for (int a = 0; a < 6; ++a) u += s_phi[t][a] * s_v[a][f];
      s_u[t][f] = u;
    }
    __syncthreads();
    // A[row][kk] = u[field][t = 4 ks + kk] x[row][t], B[kk][col] = y[col][t]; lane: row / col = lane & 15, kk = lane >> 4
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int t = 4 * ks + l4;
      const double xv = s_f[buf][0][l16][t], bv = s_f[buf][1][l16][t];
      // no branch on the field count here: a tile past nf multiplies the zero columns of s_u and is never stored, and
      // the straight-line code lets the LDS reads run ahead of the MFMAs
#pragma unroll
      for (int i = 0; i < MAXT; ++i)
        acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(s_u[t][wave + 4 * i] * xv, bv, acc[i], 0, 0, 0);
    }
    // (no barrier: the next element writes s_v and the other buffer of s_f, and s_u only behind its first barrier)
  }
  // D of v_mfma_f64_16x16x4_f64: entry g of a lane is (row (lane >> 4) + 4 g, col lane & 15)
  double* out = partial + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * nf * 256;
#pragma unroll
  for (int i = 0; i < MAXT; ++i) {
    const int f = wave + 4 * i;
    if (f >= nf) continue;
#pragma unroll
    for (int g = 0; g < 4; ++g) out[(int64_t)f * 256 + (l4 + 4 * g) * 16 + l16] = acc[i][g];
  }
}

// Second stage of k_mode_project: one lane per complex entry (field, b, a) of O [nf][lb][la][2]; the nblk partial tiles
// of its tile summed in slice order (the same bits on every run), each slice's four real products combined first.
__global__ __launch_bounds__(256) void k_project_reduce(int nf, int la, int lb, int ntx, int nblk, const double* __restrict__ partial,
                                                        double* __restrict__ O) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= (int64_t)nf * lb * la) return;
  const int a = (int)(v % la), b = (int)((v / la) % lb), f = (int)(v / ((int64_t)la * lb));
  const int64_t tile = (int64_t)(b / PJ_Y) * ntx + a / PJ_X;
  const int ai = a % PJ_X, bi = b % PJ_Y;
  const double* pp = partial + (tile * nblk * nf + f) * 256;
  double re = 0.0, im = 0.0;
  for (int s = 0; s < nblk; ++s) {
    const double* q = pp + (int64_t)s * nf * 256;
    re += q[ai * 16 + bi] - q[(8 + ai) * 16 + 8 + bi];
    im += q[ai * 16 + 8 + bi] + q[(8 + ai) * 16 + bi];
  }
  O[2 * v] = re;
  O[2 * v + 1] = im;
}

// Projection of the modes on sampled complex fields (plfem_mode_project_sampled): frame f is a complex image on the node
// grid x_i = x0 + i dx, y_j = y0 + j dy, F_f its bilinear interpolant (0 outside the closed extent), and
//   P[field][f] = sum over the elements and the 16 points of |det J| w_q u_field(x_q) F_f(x_q),
// field = (component, mode).  The GEMM of k_mode_project with the B operand gathered instead of evaluated: rows = fields
// (A[row][kk] = u[field][t], 16 fields per MFMA tile), columns = (frame, re | im) of value |det J| w F.  The frames lie
// pixel-major, frame-minor ([ny][nx][nf][2]), so the PS_COLS columns of a workgroup's tile at one pixel corner are one
// contiguous 512-byte run: wave w gathers the points w, w + 4, w + 8, w + 12, lane = column, four coalesced loads per
// point, fetched one element ahead (with the DOF rows and the element map) and interpolated into the other LDS buffer
// at the top of the next element.  Wave w then accumulates the 16-column tile w of every field tile on
// v_mfma_f64_16x16x4_f64.  A workgroup owns the frame tile blockIdx.x for ALL fields and walks the elements blockIdx.y,
// blockIdx.y + gridDim.y, ...; its partial tiles [field][column] go to its own slot (no atomics) and
// k_project_sampled_reduce sums the slots in slice order.  The slice count depends on the mesh alone, never on the
// frame count, and a column's arithmetic never on its neighbours: the bits of a frame do not depend on the frames it is
// batched with.
constexpr int PS_F = 32;             // frames per workgroup tile
constexpr int PS_COLS = 2 * PS_F;    // its columns: one 16-column MFMA tile per wave
constexpr int PS_NMAX = 8192;        // most pixels per axis
constexpr int PS_FRAMES = 4096;      // most frames per call
constexpr int PS_SLICES = 128;       // element slices (partial tiles) per frame tile, fewer only on a mesh with fewer elements
constexpr int PS_GROUP = 16;         // frame tiles per launch: the partial tiles of one group share the work buffer
constexpr int PS_LDB = PS_COLS + 16; // padded LDS row of the B operand: the four K-rows of a read 32 banks apart

// (SampledGrid and sampled_cell, the pixel grid and its cell: p2_element.h)
template <int NFT>                   // field tiles: ncomp k <= 16 NFT
__global__ __launch_bounds__(256) void k_mode_project_sampled(LocArgs L, int ncomp, int k, int64_t nrows, const double* __restrict__ V,
                                                              SampledGrid G, int nfr, int tile0, const double* __restrict__ F,
                                                              double* __restrict__ partial) {
  constexpr int FMAX = 16 * NFT;
  constexpr int LDU = FMAX % 32 == 0 ? FMAX + 16 : FMAX;   // the four K-rows of an A read 32 banks apart
  __shared__ double s_v[6][FMAX];              // the element's DOF rows (0 for a boundary DOF of an indexed record)
  __shared__ double s_u[16][LDU];
  __shared__ double s_b[2][16][PS_LDB];        // [buffer][point][column]
  __shared__ double s_phi[16][6];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nf = ncomp * k;
  const int f0 = (tile0 + (int)blockIdx.x) * PS_F;
  const int ncol = 2 * min(PS_F, nfr - f0);    // live columns of the tile (the host launches no tile past the frames)
  const bool live = lane < ncol;
  const int64_t pix = 2 * (int64_t)nfr;        // doubles per pixel
  const double* Fc = F + 2 * (int64_t)f0 + lane;   // this lane's column at pixel (0, 0)
  if (tid < 96) s_phi[tid / 6][tid % 6] = p2_phi(tid % 6, c_q16x[tid / 6], c_q16y[tid / 6]);
  for (int idx = tid; idx < 16 * LDU; idx += 256) (&s_u[0][0])[idx] = 0.0;   // (the columns past nf stay 0)
  const double* px = L.pxy;
  const double* py = L.pxy + L.nv;
  const int l16 = lane & 15, l4 = lane >> 4;
  dbl4 acc[NFT];
#pragma unroll
  for (int i = 0; i < NFT; ++i) acc[i] = dbl4{0.0, 0.0, 0.0, 0.0};
  // Fetched one element ahead, as in k_mode_project: this thread's entries of the DOF rows, the element's map, and the
  // four pixel corners of this lane's column at the wave's four points (zeros with zero weights outside the extent).
  constexpr int NV = (6 * FMAX + 255) / 256;
  double vn[NV];
  auto fetch_rows = [&](int e) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int idx = tid + 256 * j;
      vn[j] = 0.0;
      if (idx < 6 * nf) {
        const int f = idx % nf, r = dev_row(L, e, idx / nf);
        if (r >= 0) vn[j] = V[((int64_t)(f / k) * nrows + r) * k + f % k];
      }
    }
  };
  double c00[4], c01[4], c10[4], c11[4], wa[4], wb[4];
  auto fetch_corners = [&](const P2Map& M) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int pt = wave + 4 * j;
      double X, Y;
      M.point(c_q16x[pt], c_q16y[pt], X, Y);
      int i0 = 0, j0 = 0;
      wa[j] = wb[j] = 0.0;
      c00[j] = c01[j] = c10[j] = c11[j] = 0.0;
      if (sampled_cell(G, X, Y, i0, j0, wa[j], wb[j]) && live) {
        const double* p = Fc + ((int64_t)j0 * G.nx + i0) * pix;
        const int64_t up = (int64_t)G.nx * pix;
        c00[j] = p[0];
        c01[j] = p[pix];
        c10[j] = p[up];
        c11[j] = p[up + pix];
      }
    }
  };
  fetch_rows(blockIdx.y);
  P2Map Mn(L.edof, L.ne, px, py, blockIdx.y);
  fetch_corners(Mn);
  int buf = 0;
  for (int e = blockIdx.y; e < L.ne; e += gridDim.y, buf ^= 1) {
    const P2Map M = Mn;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int idx = tid + 256 * j;
      if (idx < 6 * nf) s_v[idx / nf][idx % nf] = vn[j];
    }
    {
      const double adet = fabs(M.det());
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int pt = wave + 4 * j;
        const double a = wa[j], b = wb[j], a1 = 1.0 - a, b1 = 1.0 - b;
        const double lo = mul_rn(a1, c00[j]) + mul_rn(a, c01[j]), hi = mul_rn(a1, c10[j]) + mul_rn(a, c11[j]);
        s_b[buf][pt][lane] = mul_rn(adet * c_q16w[pt], mul_rn(lo, b1) + mul_rn(hi, b));
      }
    }
    __syncthreads();
    if (e + (int)gridDim.y < L.ne) {
      Mn = P2Map(L.edof, L.ne, px, py, e + gridDim.y);
      fetch_rows(e + gridDim.y);
      fetch_corners(Mn);
    }
    for (int idx = tid; idx < 16 * nf; idx += 256) {
      const int f = idx % nf, t = idx / nf;
      double u = 0.0;
#pragma unroll
      for (int a = 0; a < 6; ++a) u += s_phi[t][a] * s_v[a][f];
      s_u[t][f] = u;
    }
    __syncthreads();
    // A[row][kk] = u[field 16 i + row][t = 4 ks + kk], B[kk][col] = s_b[t][16 wave + col]; lane: row / col = lane & 15,
    // kk = lane >> 4.  A wave whose 16 columns are all past the frames has nothing to add.
    if (16 * wave < ncol) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int t = 4 * ks + l4;
        const double bv = s_b[buf][t][16 * wave + l16];
#pragma unroll
        for (int i = 0; i < NFT; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(s_u[t][16 * i + l16], bv, acc[i], 0, 0, 0);
      }
    }
    // (no barrier: the next element writes s_v and the other buffer of s_b, and s_u only behind its first barrier)
  }
  // D of v_mfma_f64_16x16x4_f64: entry g of a lane is (row (lane >> 4) + 4 g, col lane & 15)
  double* out = partial + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * nf * PS_COLS;
#pragma unroll
  for (int i = 0; i < NFT; ++i) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int f = 16 * i + l4 + 4 * g;
      if (f < nf) out[(int64_t)f * PS_COLS + 16 * wave + l16] = acc[i][g];
    }
  }
}

// Second stage of k_mode_project_sampled: one lane per double (field, column) of the launch's frame tiles, columns
// [c0, c1) of O [nf][nfr][2]; the nblk partial tiles of its tile summed in slice order (the same bits on every run).
__global__ __launch_bounds__(256) void k_project_sampled_reduce(int nf, int nfr, int c0, int c1, int nblk,
                                                                const double* __restrict__ partial, double* __restrict__ O) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int w = c1 - c0;
  if (v >= (int64_t)nf * w) return;
  const int c = (int)(v % w), f = (int)(v / w);
  const double* pp = partial + ((int64_t)(c / PS_COLS) * nblk * nf + f) * PS_COLS + c % PS_COLS;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += pp[(int64_t)b * nf * PS_COLS];
  O[(int64_t)f * 2 * nfr + c0 + c] = s;
}


// A-posteriori error indicators of k staged modes (plfem_mode_indicators): per element T and mode m
//   eta2[m][T] = |det J| sum_q |det J| w_q |r(x_q)|^2 + sum_e c_e |e| int_e |[F . n]|^2 ds,
// the strong residual r of the pencil on the assembly's six-point rule and the jump of the flux F across the three edges
// on a two-point Gauss rule (exact: the jump is linear along an edge); c_e = 1/2 inside, on the outer boundary 1 for the
// scalar pencil (natural boundary) and 0 for the vectorial one (Dirichlet).  With t = x_hi - x_lo the edge vector and
// n = (t_y, -t_x) / |e|, c_e |e| int_e (F . n)^2 ds = (c_e / 2) sum_g (F_g . (t_y, -t_x))^2: no square root is taken.
// A workgroup owns IND_E consecutive elements.  Stage: 4 IND_E lanes form J^-1 and the six staged rows of every element
// and of its three neighbours, and find the local edge each neighbour shares (by the id of the edge DOF); 12 IND_E lanes
// evaluate the permittivity at the six quadrature points (P2Map::point, the assembly's) and at the 3 x 2 edge points
// x_lo + fl(s (x_hi - x_lo)), which both neighbours of an edge form identically from the sorted vertex pair.  Compute:
// lane (element, mode) = (tid / IND_M, tid % IND_M), IND_M modes per pass, so the 16 lanes of an element read 16
// consecutive doubles of each staged row; one lane forms one value in one fixed operation order -- nothing is summed
// across lanes, so the bits of eta2[m][T] do not depend on k or on the other modes -- and the pass is written out through
// LDS, 16 consecutive elements per mode.  Every out[m][T] is written.
constexpr int IND_E = 16;          // elements per workgroup
constexpr int IND_M = 16;          // modes per pass
constexpr double IND_G0 = 0.21132486540518708, IND_G1 = 0.7886751345948129;   // 1/2 -+ 1/(2 sqrt 3), as NumPy forms them

// reference coordinates of the point at parameter s (from the lower to the higher vertex) of local edge l
__device__ __forceinline__ void ind_edge_point(int l, double s, double& xi, double& eta) {
  xi = l == 0 ? s : (l == 1 ? 1.0 - s : 0.0);
  eta = l == 0 ? 0.0 : s;
}

// Map...: nothing, or one EpsMap: the point's permittivity is then the profile's over that map, whatever nlayer is
// (the instances without a map keep their argument list and their code).
template <int NCOMP, typename... Map>
__global__ __launch_bounds__(256) void k_mode_indicators(LocArgs L, int k, int64_t nrows, const double* __restrict__ V,
                                                         const int32_t* __restrict__ nbr, const double* __restrict__ lam,
                                                         double k0sq, double alpha, CoreTable cores, int ncore, double eps_core,
                                                         double eps_clad, const double* __restrict__ layers, int nlayer,
                                                         double eps_bg, double* __restrict__ out, Map... map) {
  __shared__ double s_inv[IND_E][4][4];      // J^-1 of the element (slot 0) and of its neighbours (slots 1-3)
  __shared__ int s_row[IND_E][4][6];         // their staged rows, -1 = contributes nothing
  __shared__ int s_nl[IND_E][3];             // the neighbour's local index of the shared edge, -1 = outer boundary
  __shared__ double s_det[IND_E];            // |det J|
  __shared__ double s_tx[IND_E][3], s_ty[IND_E][3];
  __shared__ double s_eps[IND_E][12];        // permittivity at the 6 quadrature and the 3 x 2 edge points
  __shared__ double s_phi[6][6];             // [q][i] basis values at the quadrature points
  __shared__ double s_out[IND_M][IND_E + 1];
  const int tid = threadIdx.x;
  const int ne = L.ne;
  const int e0 = blockIdx.x * IND_E;
  const double* px = L.pxy;
  const double* py = L.pxy + L.nv;
  if (tid < 36) s_phi[tid / 6][tid % 6] = p2_phi(tid % 6, c_qx[tid / 6], c_qy[tid / 6]);
  if (tid < 4 * IND_E) {
    const int el = tid >> 2, slot = tid & 3, e = e0 + el;
    int id = -1;
    if (e < ne) id = slot == 0 ? e : nbr[(int64_t)(slot - 1) * ne + e];
    if (id >= 0) {
      const P2Map M(L.edof, ne, px, py, id);
      const double det = M.det();
      M.inverse(det, s_inv[el][slot]);
#pragma unroll
      for (int a = 0; a < 6; ++a) s_row[el][slot][a] = dev_row(L, id, a);
      if (slot == 0) {
        s_det[el] = fabs(det);
      } else {
        const int node = L.edof[(int64_t)(2 + slot) * ne + e];
        int nl = 0;
#pragma unroll
        for (int l = 1; l < 3; ++l)
          if (L.edof[(int64_t)(3 + l) * ne + id] == node) nl = l;
        s_nl[el][slot - 1] = nl;
      }
    } else if (slot > 0) {
      s_nl[el][slot - 1] = -1;
    }
  } else {
    const int idx = tid - 4 * IND_E, el = idx / 12, pt = idx % 12, e = e0 + el;
    if (e < ne) {
      double X, Y;
      if (pt < 6) {
        const P2Map M(L.edof, ne, px, py, e);
        M.point(c_qx[pt], c_qy[pt], X, Y);
      } else {
        const int l = (pt - 6) >> 1;
        const int va = L.edof[(int64_t)(l == 1 ? 1 : 0) * ne + e], vb = L.edof[(int64_t)(l == 0 ? 1 : 2) * ne + e];
        const double tx = px[vb] - px[va], ty = py[vb] - py[va];
        const double s = (pt & 1) ? IND_G1 : IND_G0;
        X = px[va] + mul_rn(s, tx);
        Y = py[va] + mul_rn(s, ty);
        if (!(pt & 1)) { s_tx[el][l] = tx; s_ty[el][l] = ty; }
      }
      if constexpr (sizeof...(Map) > 0)
        s_eps[el][pt] = profile_eps(X, Y, layers, nlayer, eps_bg, map...);
      else
        s_eps[el][pt] = nlayer > 0 ? profile_eps(X, Y, layers, nlayer, eps_bg)
                                   : (in_any_core(X, Y, cores.c, ncore) ? eps_core : eps_clad);
    }
  }
  __syncthreads();
  const int el = tid / IND_M, ml = tid % IND_M, e = e0 + el;
  const int64_t plane = nrows * k;
  for (int m0 = 0; m0 < k; m0 += IND_M) {
    const int m = m0 + ml;
    if (m < k && e < ne) {
      double u[NCOMP][6], uxx[NCOMP], uxy[NCOMP], uyy[NCOMP];
#pragma unroll
      for (int c = 0; c < NCOMP; ++c) {
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          const int r = s_row[el][0][a];
          u[c][a] = r < 0 ? 0.0 : V[c * plane + (int64_t)r * k + m];
        }
        p2_hess(s_inv[el][0], u[c], uxx[c], uxy[c], uyy[c]);
      }
      const double lm = lam[m];
      // the element residual on the six-point rule
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        double uq[NCOMP];
#pragma unroll
        for (int c = 0; c < NCOMP; ++c) {
          uq[c] = 0.0;
#pragma unroll
          for (int a = 0; a < 6; ++a) uq[c] += s_phi[q][a] * u[c][a];
        }
        const double eps = s_eps[el][q];
        double r2;
        if constexpr (NCOMP == 2) {
          const double w = 1.0 / eps;
          const double dfx = -w * uxy[1] + alpha * uxx[0] + w * uyy[0] + alpha * uxy[1];
          const double dfy = w * uxx[1] + alpha * uxy[0] - w * uxy[0] + alpha * uyy[1];
          const double rx = -dfx - (k0sq + lm * w) * uq[0], ry = -dfy - (k0sq + lm * w) * uq[1];
          r2 = rx * rx + ry * ry;
        } else {
          const double r = -(uxx[0] + uyy[0]) - (k0sq * eps + lm) * uq[0];
          r2 = r * r;
        }
        acc += c_qw[q] * r2;
      }
      const double det = s_det[el];
      double eta = det * (det * acc);
      // the flux jumps across the three edges
#pragma unroll 1
      for (int l = 0; l < 3; ++l) {
        const int nl = s_nl[el][l];
        if (NCOMP == 2 && nl < 0) continue;        // Dirichlet boundary: no term
        double un[NCOMP][6];
#pragma unroll
        for (int c = 0; c < NCOMP; ++c)
#pragma unroll
          for (int a = 0; a < 6; ++a) {
            const int r = nl < 0 ? -1 : s_row[el][1 + l][a];
            un[c][a] = r < 0 ? 0.0 : V[c * plane + (int64_t)r * k + m];
          }
        const double tx = s_tx[el][l], ty = s_ty[el][l];
        double j2 = 0.0;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const double s = g ? IND_G1 : IND_G0;
          double f[2][NCOMP];                       // F . (t_y, -t_x) of every component, this side and the other
#pragma unroll
          for (int side = 0; side < 2; ++side) {
            double xi, eta_r, gx[6], gy[6], ux[NCOMP], uy[NCOMP];
            ind_edge_point(side == 0 ? l : (nl < 0 ? 0 : nl), s, xi, eta_r);
            p2_grad(s_inv[el][side == 0 ? 0 : 1 + l], xi, eta_r, gx, gy);
#pragma unroll
            for (int c = 0; c < NCOMP; ++c) {
              ux[c] = uy[c] = 0.0;
#pragma unroll
              for (int a = 0; a < 6; ++a) {
                const double v = side == 0 ? u[c][a] : un[c][a];
                ux[c] += gx[a] * v;
                uy[c] += gy[a] * v;
              }
            }
            if constexpr (NCOMP == 2) {
              const double w = 1.0 / s_eps[el][6 + 2 * l + g];
              const double fxx = -w * uy[1] + alpha * ux[0], fxy = w * uy[0] + alpha * ux[1];
              const double fyx = w * ux[1] + alpha * uy[0], fyy = -w * ux[0] + alpha * uy[1];
              f[side][0] = fxx * ty - fxy * tx;
              f[side][1] = fyx * ty - fyy * tx;
            } else {
              f[side][0] = ux[0] * ty - uy[0] * tx;
            }
          }
#pragma unroll
          for (int c = 0; c < NCOMP; ++c) {
            const double j = nl < 0 ? f[0][c] : f[0][c] - f[1][c];
            j2 += j * j;
          }
        }
        eta += (nl < 0 ? 0.5 : 0.25) * j2;
      }
      s_out[ml][el] = eta;
    }
    __syncthreads();
    {
      const int mo = tid / IND_E, eo = tid % IND_E;
      if (m0 + mo < k && e0 + eo < ne) out[(int64_t)(m0 + mo) * ne + e0 + eo] = s_out[mo][eo];
    }
    __syncthreads();
  }
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace
}  // namespace plfem

using namespace plfem;

namespace {
struct LocLayout { size_t off_ptr, off_elems, off_edof, off_idx, off_pxy, off_layers, total; };
LocLayout loc_layout(const Symbolic& S) {
  LocLayout l;
  size_t o = 0;
  l.off_ptr = o;   o += align256(S.loc_cell_ptr.size() * sizeof(int32_t));
  l.off_elems = o; o += align256(std::max<size_t>(1, S.loc_cell_elems.size()) * sizeof(int32_t));
  l.off_edof = o;  o += align256((size_t)6 * S.ne * sizeof(int32_t));
  l.off_idx = o;   o += align256((size_t)S.N * sizeof(int32_t));
  l.off_pxy = o;   o += align256((size_t)2 * S.nv * sizeof(double));
  l.off_layers = o; o += align256((size_t)MAX_LAYERS * LAYER_DOUBLES * sizeof(double));
  l.total = o;
  return l;
}
}  // namespace

extern "C" int plfem_locator_bytes(const plfem_symbolic* sym, int64_t* bytes) try {
  if (!sym || !bytes) return PLFEM_EINVAL;
  ensure_locator(sym->S);
  *bytes = (int64_t)loc_layout(sym->S).total;
  return PLFEM_OK;
} catch (...) { return host_failure(nullptr, 0); }

extern "C" int plfem_locator_create(const plfem_symbolic* sym, int32_t device, void* hip_stream, void* mem_dev,
                                    int64_t mem_bytes, plfem_locator** out, char* err, int32_t errlen) try {
  if (!out) return PLFEM_EINVAL;
  *out = nullptr;
  if (!sym || !mem_dev) return write_err(err, errlen, "plfem_locator_create: null analysis or device memory", PLFEM_EINVAL);
  if ((uintptr_t)mem_dev & 255) return write_err(err, errlen, "plfem_locator_create: device memory must be 256-byte aligned", PLFEM_EINVAL);
  const Symbolic& S = sym->S;
  ensure_locator(S);
  const LocLayout lay = loc_layout(S);
  if (mem_bytes < (int64_t)lay.total)
    return write_err(err, errlen, "plfem_locator_create: device memory smaller than plfem_locator_bytes", PLFEM_EINVAL);
  Owned<plfem_locator> L(new plfem_locator());
  L->S = &S;
  L->device = device;
  L->stream = (hipStream_t)hip_stream;
  L->nv = S.nv; L->ne = S.ne; L->N = S.N; L->nsolve = S.nsolve;
  L->x0 = S.loc_grid[0]; L->y0 = S.loc_grid[1]; L->inv_hx = S.loc_grid[2]; L->inv_hy = S.loc_grid[3];
  L->nx = (int)S.loc_grid[4]; L->ny = (int)S.loc_grid[5];
  char* base = (char*)mem_dev;
  L->d_cell_ptr = (int32_t*)(base + lay.off_ptr);
  L->d_cell_elems = (int32_t*)(base + lay.off_elems);
  L->d_edof = (int32_t*)(base + lay.off_edof);
  L->d_int_index = (int32_t*)(base + lay.off_idx);
  L->d_pxy = (double*)(base + lay.off_pxy);
  L->d_layers = (double*)(base + lay.off_layers);
  // vertex coordinates = the first nv entries of both doflocs rows
  std::vector<double> pxy((size_t)2 * S.nv);
  std::memcpy(pxy.data(), S.doflocs.data(), sizeof(double) * S.nv);
  std::memcpy(pxy.data() + S.nv, S.doflocs.data() + S.N, sizeof(double) * S.nv);
  struct { void* d; const void* h; size_t b; } up[] = {
      {L->d_cell_ptr, S.loc_cell_ptr.data(), S.loc_cell_ptr.size() * sizeof(int32_t)},
      {L->d_cell_elems, S.loc_cell_elems.data(), S.loc_cell_elems.size() * sizeof(int32_t)},
      {L->d_edof, S.edof.data(), S.edof.size() * sizeof(int32_t)},
      {L->d_int_index, S.int_index.data(), S.int_index.size() * sizeof(int32_t)},
      {L->d_pxy, pxy.data(), pxy.size() * sizeof(double)}};
  auto upload = [&] {
    HIP_TRY(L, hipSetDevice(device));
    for (auto& u : up)
      if (u.b > 0) HIP_TRY(L, hipMemcpyAsync(u.d, u.h, u.b, hipMemcpyHostToDevice, L->stream));
    HIP_TRY(L, hipStreamSynchronize(L->stream));       // (pxy is a local buffer)
    return PLFEM_OK;
  };
  const int rc = upload();
  if (rc != PLFEM_OK) return write_err(err, errlen, L->err, rc);
  *out = L.release();
  return PLFEM_OK;
} catch (...) { return host_failure(err, errlen); }

extern "C" void plfem_locator_destroy(plfem_locator* loc) {
  if (!loc) return;
  (void)hipSetDevice(loc->device);
  (void)hipStreamSynchronize(loc->stream);     // nothing in flight may still read the caller's memory
  free_index_map(loc->map);
  delete loc;
}

extern "C" int plfem_locator_set_index_map(plfem_locator* L, const double* eps_host, int32_t nx, int32_t ny, double x0,
                                           double y0, double dx, double dy) try {
  if (!L) return PLFEM_EINVAL;
  return set_index_map(L, "plfem_locator_set_index_map", eps_host, nx, ny, x0, y0, dx, dy);
} catch (...) { return host_failure(L); }

extern "C" const char* plfem_locator_last_error(const plfem_locator* loc) { return loc ? loc->err.c_str() : "null locator"; }

// ---- the field entry points ---------------------------------------------------------------------------------------
// Every one has the same shape ("The shape of a field entry point"): null locator; the call's own argument
// checks, each one expression `return call.reject(...)`, in a fixed order; FieldCall::enter (interior DOFs, work buffer,
// device); the launches, each followed by check_launch; result_to_host.
namespace {
int overlap_chunks(int k) { return (k + OC - 1) / OC; }

// ncomp 1 or 2 and 1 <= k <= kmax: what the mode calls and their sizers accept
bool modes_ok(int ncomp, int k, int kmax = INT32_MAX) { return ncomp >= 1 && ncomp <= 2 && k >= 1 && k <= kmax; }

// a core count: at most MAX_CORES, and negative ("no weight") only in the calls that have an unweighted form
bool ncore_ok(int ncore, bool unweighted_ok) { return ncore <= MAX_CORES && (ncore >= 0 || unweighted_ok); }

// the cores as the kernels' by-value table, zero past ncore
CoreTable pack_cores(const double* cores_host, int ncore) {
  CoreTable ct;
  std::memset(&ct, 0, sizeof(ct));
  if (ncore > 0) std::memcpy(ct.c, cores_host, sizeof(double) * 3 * ncore);
  return ct;
}

// A field call on its way from its arguments to its launches: the locator that takes the error text and whose stream
// runs the call, the entry point's name, and what enter() makes of `indexed` and the work buffer
struct FieldCall {
  plfem_locator* L;
  const char* fn;
  plfem_locator* Lb = nullptr;               // the second mesh of an overlap (pair())
  int64_t nrows = 0, nrows_b = 0;            // rows of the staged modes
  LocArgs loc{}, loc_b{};
  double *O = nullptr, *partial = nullptr;   // the work buffer: the result at its start, the partial sums behind it

  int reject(const std::string& what) const {
    L->err = std::string(fn) + ": " + what;
    return PLFEM_EINVAL;
  }
  int pair(plfem_locator* other) {
    if (!other || L->device != other->device) return reject("the two locators must be on one device");
    Lb = other;
    return PLFEM_OK;
  }
  // interior-indexed modes need interior DOFs; the rows and the kernels' locator arguments of each mesh
  int modes(int indexed, int indexed_b = 0) {
    if ((indexed && L->nsolve == 0) || (Lb && indexed_b && Lb->nsolve == 0)) return reject("the analysis has no interior DOFs");
    nrows = indexed ? L->nsolve : L->N;
    loc = loc_args(L, indexed != 0);
    if (Lb) {
      nrows_b = indexed_b ? Lb->nsolve : Lb->N;
      loc_b = loc_args(Lb, indexed_b != 0);
    }
    return PLFEM_OK;
  }
  // the caller's work buffer: at least `need` bytes (what `sizer` returns), 256-byte aligned, partial sums from
  // `off_partial`; then the device
  int work(const char* sizer, void* work_dev, int64_t work_bytes, size_t need, size_t off_partial) {
    if (work_bytes < (int64_t)need) return reject(std::string("work buffer smaller than ") + sizer);
    if ((uintptr_t)work_dev & 255) return reject("work buffer must be 256-byte aligned");
    HIP_TRY(L, hipSetDevice(L->device));
    O = (double*)work_dev;
    partial = (double*)((char*)work_dev + off_partial);
    return PLFEM_OK;
  }
  // what follows a call's own checks
  int enter(int indexed, const char* sizer, void* work_dev, int64_t work_bytes, size_t need, size_t off_partial,
            int indexed_b = 0) {
    TRY(modes(indexed, indexed_b));
    return work(sizer, work_dev, work_bytes, need, off_partial);
  }
};

// f(map) with the locator's sampled map when it carries one, f() otherwise: a kernel template <..., typename... Map> is
// launched as its EpsMap or its plain instance by one line, `kernel<..., decltype(map)...>` with `map...` as last argument
template <typename F>
void with_map(const plfem_locator* L, F&& f) {
  if (L->map.set()) f(eps_map(L->map));
  else f();
}

// how a call ends: the first `n` doubles of the work buffer to `out_host`, the stream synchronised
int result_to_host(plfem_locator* L, const double* O, size_t n, double* out_host) {
  HIP_TRY(L, hipMemcpyAsync(out_host, O, sizeof(double) * n, hipMemcpyDeviceToHost, L->stream));
  HIP_TRY(L, hipStreamSynchronize(L->stream));
  return PLFEM_OK;
}

// k_overlap_reduce over `grid` (chunk pairs, output matrices, entry slices), then O [grid.y][ka][kb] to the host
int reduce_to_host(plfem_locator* L, dim3 grid, int ka, int kb, int nblk, int nchunk_b, const double* partial, double* O,
                   double* out_host) {
  hipLaunchKernelGGL(k_overlap_reduce, grid, dim3(256), 0, L->stream, ka, kb, nblk, nchunk_b, partial, O);
  TRY(check_launch(L, "k_overlap_reduce"));
  return result_to_host(L, O, (size_t)grid.y * ka * kb, out_host);
}

// at most `slices` element slices, one per element of a small mesh, at least 1
int element_slices(int slices, int ne) { return std::max(1, std::min(slices, ne)); }

// A field call's work buffer: the result (`result` doubles), then, 256-byte aligned, `partial` doubles of partial sums
struct WorkLayout { size_t off_partial, total; };   // bytes
WorkLayout work_layout(size_t result, size_t partial) {
  const size_t off = align256(result * sizeof(double));
  return {off, off + partial * sizeof(double)};
}
WorkLayout overlap_layout(int ka, int kb) {
  return work_layout((size_t)ka * kb, (size_t)overlap_chunks(ka) * overlap_chunks(kb) * OVL_BLOCKS * OC * OC);
}
}  // namespace

extern "C" int plfem_stage_modes(plfem_locator* L, int32_t ncomp, int32_t k, int32_t nrows, const double* src_dev, double* dst_dev) try {
  if (!L) return PLFEM_EINVAL;
  const FieldCall call{L, "plfem_stage_modes"};
  if (ncomp < 1 || ncomp > 2 || k < 0 || nrows < 0 || ((!src_dev || !dst_dev) && k > 0 && nrows > 0))
    return call.reject("bad arguments");
  if (k == 0 || nrows == 0) return PLFEM_OK;
  HIP_TRY(L, hipSetDevice(L->device));
  dim3 grid((nrows + 31) / 32, (k + 31) / 32, ncomp);
  hipLaunchKernelGGL(k_stage_modes, grid, dim3(256), 0, L->stream, (int)k, (int)nrows, src_dev, dst_dev);
  return check_launch(L, "k_stage_modes");
} catch (...) { return host_failure(L); }

extern "C" int plfem_sample_fields(plfem_locator* L, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                                   const double* beta_dev, int32_t npts, const double* points_dev, double* out_dev,
                                   int32_t* elem_dev) try {
  if (!L) return PLFEM_EINVAL;
  FieldCall call{L, "plfem_sample_fields"};
  if (ncomp < 1 || ncomp > 2 || k < 0 || npts < 0) return call.reject("ncomp must be 1 or 2, k and npts >= 0");
  if (npts == 0) return PLFEM_OK;
  if (!points_dev || !elem_dev || (k > 0 && (!modes_dev || !out_dev))) return call.reject("null device array");
  TRY(call.modes(indexed));
  HIP_TRY(L, hipSetDevice(L->device));
  hipLaunchKernelGGL(k_sample_fields, dim3((npts + 255) / 256), dim3(256), 0, L->stream, call.loc, (int)ncomp, (int)k, call.nrows,
                     modes_dev, ncomp == 2 ? beta_dev : nullptr, (int)npts, points_dev, out_dev, elem_dev);
  return check_launch(L, "k_sample_fields");
} catch (...) { return host_failure(L); }

extern "C" int plfem_overlap_work_bytes(int32_t ka, int32_t kb, int64_t* bytes) {
  if (!bytes || ka < 0 || kb < 0) return PLFEM_EINVAL;
  *bytes = (int64_t)overlap_layout(ka, kb).total;
  return PLFEM_OK;
}

extern "C" int plfem_field_overlap(plfem_locator* La, const double* modes_a_dev, int32_t ka, int32_t indexed_a,
                                   plfem_locator* Lb, const double* modes_b_dev, int32_t kb, int32_t indexed_b, int32_t ncomp,
                                   const double* cores_host, int32_t ncore, double eps_core, double eps_clad,
                                   void* work_dev, int64_t work_bytes, double* out_host) try {
  if (!La) return PLFEM_EINVAL;
  FieldCall call{La, "plfem_field_overlap"};
  TRY(call.pair(Lb));
  if (ncomp < 1 || ncomp > 2 || ka < 0 || kb < 0) return call.reject("bad ncomp / ka / kb");
  if (ka == 0 || kb == 0) return PLFEM_OK;
  if (!modes_a_dev || !modes_b_dev || !work_dev || !out_host) return call.reject("null array");
  if (!ncore_ok(ncore, true) || (ncore > 0 && !cores_host)) return call.reject("at most 64 cores");
  const WorkLayout lay = overlap_layout(ka, kb);
  TRY(call.enter(indexed_a, "plfem_overlap_work_bytes", work_dev, work_bytes, lay.total, lay.off_partial, indexed_b));
  const int nca = overlap_chunks(ka), ncb = overlap_chunks(kb);
  const int64_t ntiles = ((int64_t)6 * Lb->ne + OT - 1) / OT;
  const int nblk = (int)std::min<int64_t>(OVL_BLOCKS, ntiles);
  hipLaunchKernelGGL(k_field_overlap, dim3(nblk, nca * ncb), dim3(256), 0, La->stream, call.loc, call.loc_b, (int)ncomp, (int)ka,
                     call.nrows, modes_a_dev, (int)kb, call.nrows_b, modes_b_dev, pack_cores(cores_host, ncore),
                     ncore < 0 ? -1 : (int)ncore, 1.0 / eps_core, 1.0 / eps_clad, ncb, call.partial);
  TRY(check_launch(La, "k_field_overlap"));
  return reduce_to_host(La, dim3(nca * ncb), (int)ka, (int)kb, nblk, ncb, call.partial, call.O, out_host);
} catch (...) { return host_failure(La); }

namespace {
constexpr int POSE_BATCH = 4096;                       // most poses per internal batch
constexpr int POSE_MAX_PAIRS = 256;                    // most chunk pairs of a posed call
constexpr int64_t POSE_SCRATCH = (int64_t)512 << 20;   // what the work buffer never exceeds
// Batches, slices and work buffer of a posed overlap: the results of a batch [batch][ka][kb], then its partials
// [batch][chunk pair][slice][OC * OC], then its pose rows, each part 256-byte aligned
struct PosedPlan {
  int nca, ncb, slices, batch;
  size_t off_partial, off_poses, total;   // bytes
};
// (`tile` points per tile of B and `nout` matrices per pose: OT and 1 for plfem_field_overlap_posed, FT and 4 for
// plfem_flux_overlap_posed, whose results are [batch][nout][ka][kb] and partials [batch][nout][chunk pair][slice][OC * OC])
PosedPlan posed_plan(int ne_b, int ka, int kb, int nposes, int tile = OT, int nout = 1) {
  PosedPlan p;
  p.nca = overlap_chunks(ka);
  p.ncb = overlap_chunks(kb);
  const int64_t ntiles = ((int64_t)6 * ne_b + tile - 1) / tile;
  p.slices = (int)std::max<int64_t>(1, std::min<int64_t>(POSE_SLICES, ntiles));
  const int64_t per_pose = (int64_t)sizeof(double) * ((int64_t)nout * ka * kb + (int64_t)nout * p.nca * p.ncb * p.slices * OC * OC + POSE_DOUBLES);
  p.batch = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(nposes, POSE_BATCH), (POSE_SCRATCH - 768) / per_pose));
  size_t o = align256(sizeof(double) * p.batch * nout * ka * kb);
  p.off_partial = o; o += align256(sizeof(double) * p.batch * nout * p.nca * p.ncb * p.slices * OC * OC);
  p.off_poses = o;   o += align256(sizeof(double) * p.batch * POSE_DOUBLES);
  p.total = o;
  return p;
}
const char* posed_sizes(int ka, int kb, int nposes, int max_pairs = POSE_MAX_PAIRS) {
  if (ka < 1 || kb < 1) return "ka and kb must be >= 1";
  if (nposes < 1) return "nposes must be >= 1";
  if ((int64_t)overlap_chunks(ka) * overlap_chunks(kb) > max_pairs)
    return max_pairs == POSE_MAX_PAIRS ? "at most 256 pairs of 32-mode chunks" : "at most 64 pairs of 32-mode chunks";
  return nullptr;
}
// every entry finite, m > 0, |c^2 + s^2 - 1| <= 1e-12
bool poses_ok(const double* poses, int n) {
  for (int i = 0; i < n; ++i) {
    const double* p = poses + (size_t)POSE_DOUBLES * i;
    for (int j = 0; j < POSE_DOUBLES; ++j)
      if (!std::isfinite(p[j])) return false;
    if (!(p[4] > 0.0) || !(std::fabs(p[2] * p[2] + p[3] * p[3] - 1.0) <= 1e-12)) return false;
  }
  return true;
}
}  // namespace

extern "C" int plfem_overlap_posed_work_bytes(const plfem_locator* Lb, int32_t ka, int32_t kb, int32_t nposes, int64_t* bytes) try {
  if (!Lb || !bytes || posed_sizes(ka, kb, nposes)) return PLFEM_EINVAL;
  *bytes = (int64_t)posed_plan(Lb->ne, ka, kb, nposes).total;
  return PLFEM_OK;
} catch (...) { return host_failure(nullptr, 0); }

extern "C" int plfem_field_overlap_posed(plfem_locator* La, const double* modes_a_dev, int32_t ka, int32_t indexed_a,
                                         plfem_locator* Lb, const double* modes_b_dev, int32_t kb, int32_t indexed_b, int32_t ncomp,
                                         const double* cores_host, int32_t ncore, double eps_core, double eps_clad,
                                         int32_t nposes, const double* poses_host, void* work_dev, int64_t work_bytes,
                                         double* out_host) try {
  if (!La) return PLFEM_EINVAL;
  FieldCall call{La, "plfem_field_overlap_posed"};
  TRY(call.pair(Lb));
  if (ncomp < 1 || ncomp > 2) return call.reject("ncomp must be 1 or 2");
  if (const char* bad = posed_sizes(ka, kb, nposes)) return call.reject(bad);
  if (!modes_a_dev || !modes_b_dev || !poses_host || !work_dev || !out_host) return call.reject("null array");
  if (!ncore_ok(ncore, true) || (ncore > 0 && !cores_host)) return call.reject("at most 64 cores");
  TRY(call.modes(indexed_a, indexed_b));
  if (!poses_ok(poses_host, nposes))
    return call.reject("every pose (tx, ty, c, s, m) must be finite with m > 0 and |c^2 + s^2 - 1| <= 1e-12");
  const PosedPlan plan = posed_plan(Lb->ne, ka, kb, nposes);
  TRY(call.work("plfem_overlap_posed_work_bytes", work_dev, work_bytes, plan.total, plan.off_partial));
  double* poses = (double*)((char*)work_dev + plan.off_poses);
  const CoreTable ct = pack_cores(cores_host, ncore);
  const int npair = plan.nca * plan.ncb;
  // the batches follow each other on one stream: a batch's pose rows, partials and results are read before the next
  // batch's copies and kernels overwrite them
  for (int p0 = 0; p0 < nposes; p0 += plan.batch) {
    const int nb = std::min(plan.batch, nposes - p0);
    HIP_TRY(La, hipMemcpyAsync(poses, poses_host + (size_t)POSE_DOUBLES * p0, sizeof(double) * POSE_DOUBLES * nb,
                               hipMemcpyHostToDevice, La->stream));
    hipLaunchKernelGGL(k_field_overlap_posed, dim3(plan.slices, npair, nb), dim3(256), 0, La->stream, call.loc, call.loc_b,
                       (int)ncomp, (int)ka, call.nrows, modes_a_dev, (int)kb, call.nrows_b, modes_b_dev, ct,
                       ncore < 0 ? -1 : (int)ncore, 1.0 / eps_core, 1.0 / eps_clad, plan.ncb, poses, call.partial);
    TRY(check_launch(La, "k_field_overlap_posed"));
    hipLaunchKernelGGL(k_overlap_reduce, dim3(npair, nb, OC * OC / 256), dim3(256), 0, La->stream, (int)ka, (int)kb, plan.slices,
                       plan.ncb, call.partial, call.O);
    TRY(check_launch(La, "k_overlap_reduce"));
    HIP_TRY(La, hipMemcpyAsync(out_host + (size_t)p0 * ka * kb, call.O, sizeof(double) * nb * ka * kb, hipMemcpyDeviceToHost,
                               La->stream));
  }
  HIP_TRY(La, hipStreamSynchronize(La->stream));
  return PLFEM_OK;
} catch (...) { return host_failure(La); }

namespace {
// The Gram calls on the whole mesh (plfem_mode_grams, plfem_profile_grams, plfem_moment_grams) share one grid and one work
// buffer: `nout` matrices [k][k], then per matrix and chunk pair GRAM_BLOCKS partial blocks
int gram_outputs(int ncomp) { return ncomp == 2 ? 5 : 3; }
int profile_gram_outputs(int ncomp) { return ncomp == 2 ? 4 : 3; }
int moment_gram_outputs(int ncomp) { return ncomp == 2 ? 11 : 7; }
WorkLayout gram_layout(int nout, int k) {
  const size_t no = nout, nc = overlap_chunks(k);
  return work_layout(no * k * k, no * nc * nc * GRAM_BLOCKS * OC * OC);
}
// blocks per chunk pair: a function of the mesh alone, so the bits of an entry do not change with the number of modes
int gram_blocks(int ne) { return (int)std::max<int64_t>(1, std::min<int64_t>(GRAM_BLOCKS, ((int64_t)6 * ne + GT - 1) / GT)); }
// the partial blocks (`nblk` per chunk pair) summed into `nmat` matrices [k][k], and those to the host
int grams_to_host(const FieldCall& call, int nmat, int k, int nblk, double* out_host) {
  const int nc = overlap_chunks(k);
  return reduce_to_host(call.L, dim3(nc * nc, nmat, OC * OC / 256), k, k, nblk, nc, call.partial, call.O, out_host);
}
}  // namespace

extern "C" int plfem_gram_work_bytes(int32_t ncomp, int32_t k, int64_t* bytes) {
  if (!bytes || !modes_ok(ncomp, k)) return PLFEM_EINVAL;
  *bytes = (int64_t)gram_layout(gram_outputs(ncomp), k).total;
  return PLFEM_OK;
}

extern "C" int plfem_mode_grams(plfem_locator* L, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                                const double* cores_host, int32_t ncore, void* work_dev, int64_t work_bytes, double* out_host) try {
  if (!L) return PLFEM_EINVAL;
  FieldCall call{L, "plfem_mode_grams"};
  if (!modes_ok(ncomp, k)) return call.reject("ncomp must be 1 or 2 and k > 0");
  if (!ncore_ok(ncore, false)) return call.reject("ncore must be in [0, 64]");
  if (!modes_dev || !work_dev || !out_host || (ncore > 0 && !cores_host)) return call.reject("null array");
  const WorkLayout lay = gram_layout(gram_outputs(ncomp), k);
  TRY(call.enter(indexed, "plfem_gram_work_bytes", work_dev, work_bytes, lay.total, lay.off_partial));
  const CoreTable ct = pack_cores(cores_host, ncore);
  const int nc = overlap_chunks(k), nblk = gram_blocks(L->ne);
  with_constant<2, 1>(ncomp, [&](auto nco) {
    hipLaunchKernelGGL(k_mode_grams<decltype(nco)::value>, dim3(nblk, nc * nc), dim3(256), 0, L->stream, call.loc, (int)k,
                       call.nrows, modes_dev, ct, (int)ncore, nc, call.partial);
  });
  TRY(check_launch(L, "k_mode_grams"));
  return grams_to_host(call, gram_outputs(ncomp), k, nblk, out_host);
} catch (...) { return host_failure(L); }

extern "C" int plfem_profile_gram_work_bytes(int32_t ncomp, int32_t k, int64_t* bytes) {
  if (!bytes || !modes_ok(ncomp, k)) return PLFEM_EINVAL;
  *bytes = (int64_t)gram_layout(profile_gram_outputs(ncomp), k).total;
  return PLFEM_OK;
}

extern "C" int plfem_profile_grams(plfem_locator* L, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                                   const double* layers_host, int32_t nlayer, double eps_bg, void* work_dev, int64_t work_bytes,
                                   double* out_host) try {
  if (!L) return PLFEM_EINVAL;
  FieldCall call{L, "plfem_profile_grams"};
  if (!modes_ok(ncomp, k)) return call.reject("ncomp must be 1 or 2 and k > 0");
  if (const char* bad = profile_table_error(layers_host, nlayer, eps_bg)) return call.reject(bad);
  if (!modes_dev || !work_dev || !out_host) return call.reject("null array");
  const WorkLayout lay = gram_layout(profile_gram_outputs(ncomp), k);
  TRY(call.enter(indexed, "plfem_profile_gram_work_bytes", work_dev, work_bytes, lay.total, lay.off_partial));
  // (every call of a locator that reads the table ends with a stream synchronisation: nothing in flight reads the old one)
  if (nlayer > 0)
    HIP_TRY(L, hipMemcpyAsync(L->d_layers, layers_host, sizeof(double) * LAYER_DOUBLES * nlayer, hipMemcpyHostToDevice, L->stream));
  const int nc = overlap_chunks(k), nblk = gram_blocks(L->ne);
  with_constant<2, 1>(ncomp, [&](auto nco) {
    with_map(L, [&](auto... map) {
      hipLaunchKernelGGL((k_profile_grams<decltype(nco)::value, decltype(map)...>), dim3(nblk, nc * nc), dim3(256), 0, L->stream,
                         call.loc, (int)k, call.nrows, modes_dev, L->d_layers, (int)nlayer, eps_bg, nc, call.partial, map...);
    });
  });
  TRY(check_launch(L, "k_profile_grams"));
  return grams_to_host(call, profile_gram_outputs(ncomp), k, nblk, out_host);
} catch (...) { return host_failure(L); }

namespace {
constexpr int FLUX_GRAM_OUTPUTS = 4;   // M_w_core, M_w_rest, G_w_core, G_w_rest

// The material arguments of the electric-field calls (plfem_flux_grams, plfem_sample_efields): nullptr if they are
// acceptable, otherwise what is wrong with them.  use_profile: the layer table as plfem_set_index_profile takes it, over
// the locator's map if one is set; otherwise eps_core / eps_clad, and a map on the locator is an error, not ignored.
const char* material_error(const plfem_locator* L, double eps_core, double eps_clad, const double* layers_host, int nlayer,
                           double eps_bg, int use_profile) {
  if (use_profile) return profile_table_error(layers_host, nlayer, eps_bg);
  if (!std::isfinite(eps_core) || !std::isfinite(eps_clad) || !(eps_core > 0.0) || !(eps_clad > 0.0))
    return "eps_core and eps_clad must be finite and positive";
  if (L->map.set()) return "the locator carries a sampled index map: use_profile must be set (or the map cleared)";
  return nullptr;
}

// the kernels' Material; the layer table of a profile goes to the locator's device buffer on its stream (the call ends with
// a stream synchronisation: the host table outlives the copy and nothing in flight reads the table of an earlier call).
// `owner`: the locator whose buffer carries the table when it is not L's own -- the second mesh of
// plfem_flux_overlap_posed; the copy still runs on L's stream, which runs the call
int stage_material(plfem_locator* L, const double* cores_host, int ncore, double eps_core, double eps_clad,
                   const double* layers_host, int nlayer, double eps_bg, int use_profile, Material& mat,
                   plfem_locator* owner = nullptr) {
  double* d_layers = owner ? owner->d_layers : L->d_layers;
  if (use_profile && nlayer > 0)
    HIP_TRY(L, hipMemcpyAsync(d_layers, layers_host, sizeof(double) * LAYER_DOUBLES * nlayer, hipMemcpyHostToDevice, L->stream));
  mat = Material{pack_cores(cores_host, ncore), ncore, eps_core, eps_clad, d_layers, use_profile ? nlayer : 0, eps_bg};
  return PLFEM_OK;
}

// f(profile, map...) for the three material instances: discs (std::false_type), profile, profile over the locator's map
template <typename F>
void with_material(const plfem_locator* L, int use_profile, F&& f) {
  if (use_profile) with_map(L, [&](auto... map) { f(std::true_type{}, map...); });
  else f(std::false_type{});
}
}  // namespace

extern "C" int plfem_flux_gram_work_bytes(int32_t k, int64_t* bytes) {
  if (!bytes || k < 1) return PLFEM_EINVAL;
  *bytes = (int64_t)gram_layout(FLUX_GRAM_OUTPUTS, k).total;
  return PLFEM_OK;
}

extern "C" int plfem_flux_grams(plfem_locator* L, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                                const double* cores_host, int32_t ncore, double eps_core, double eps_clad,
                                const double* layers_host, int32_t nlayer, double eps_bg, int32_t use_profile, void* work_dev,
                                int64_t work_bytes, double* out_host) try {
  if (!L) return PLFEM_EINVAL;
  FieldCall call{L, "plfem_flux_grams"};
  if (ncomp != 2 || k < 1) return call.reject("ncomp must be 2 (vectorial records) and k > 0");
  if (!ncore_ok(ncore, false)) return call.reject("ncore must be in [0, 64]");
  if (!modes_dev || !work_dev || !out_host || (ncore > 0 && !cores_host)) return call.reject("null array");
  if (const char* bad = material_error(L, eps_core, eps_clad, layers_host, nlayer, eps_bg, use_profile)) return call.reject(bad);
  const WorkLayout lay = gram_layout(FLUX_GRAM_OUTPUTS, k);
  TRY(call.enter(indexed, "plfem_flux_gram_work_bytes", work_dev, work_bytes, lay.total, lay.off_partial));
  Material mat;
  TRY(stage_material(L, cores_host, ncore, eps_core, eps_clad, layers_host, nlayer, eps_bg, use_profile, mat));
  const int nc = overlap_chunks(k), nblk = gram_blocks(L->ne);
  with_material(L, use_profile, [&](auto profile, auto... map) {
    hipLaunchKernelGGL((k_flux_grams<decltype(profile)::value, decltype(map)...>), dim3(nblk, nc * nc), dim3(256), 0, L->stream,
                       call.loc, (int)k, call.nrows, modes_dev, mat, nc, call.partial, map...);
  });
  TRY(check_launch(L, "k_flux_grams"));
  return grams_to_host(call, FLUX_GRAM_OUTPUTS, k, nblk, out_host);
} catch (...) { return host_failure(L); }

extern "C" int plfem_sample_efields(plfem_locator* L, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                                    const double* beta_dev, double k0, const double* cores_host, int32_t ncore, double eps_core,
                                    double eps_clad, const double* layers_host, int32_t nlayer, double eps_bg,
                                    int32_t use_profile, int32_t npts, const double* points_dev, double* out_dev,
                                    double* eps_dev, int32_t* elem_dev) try {
  if (!L) return PLFEM_EINVAL;
  FieldCall call{L, "plfem_sample_efields"};
  if (ncomp != 2 || k < 1 || npts < 0) return call.reject("ncomp must be 2 (vectorial records), k > 0 and npts >= 0");
  if (!ncore_ok(ncore, false)) return call.reject("ncore must be in [0, 64]");
  if (npts == 0) return PLFEM_OK;
  if (!modes_dev || !beta_dev || !points_dev || !out_dev || !elem_dev || (ncore > 0 && !cores_host))
    return call.reject("null array");
  if (const char* bad = material_error(L, eps_core, eps_clad, layers_host, nlayer, eps_bg, use_profile)) return call.reject(bad);
  if (!std::isfinite(k0) || !(k0 > 0.0)) return call.reject("k0 must be finite and positive");
  TRY(call.modes(indexed));
  HIP_TRY(L, hipSetDevice(L->device));
  Material mat;
  TRY(stage_material(L, cores_host, ncore, eps_core, eps_clad, layers_host, nlayer, eps_bg, use_profile, mat));
  with_material(L, use_profile, [&](auto profile, auto... map) {
    hipLaunchKernelGGL((k_sample_efields<decltype(profile)::value, decltype(map)...>), dim3((npts + 255) / 256), dim3(256), 0,
                       L->stream, call.loc, (int)k, call.nrows, modes_dev, beta_dev, k0, mat, (int)npts, points_dev, out_dev,
                       eps_dev, elem_dev, map...);
  });
  TRY(check_launch(L, "k_sample_efields"));
  HIP_TRY(L, hipStreamSynchronize(L->stream));
  return PLFEM_OK;
} catch (...) { return host_failure(L); }

namespace {
// Most chunk pairs of a posed flux call.  Four outputs make a pose's partials four times those of plfem_field_overlap_posed:
// with 128 slices, 64 pairs are 256 MiB of them, so one pose of the largest call fits POSE_SCRATCH (256 pairs would not)
constexpr int FLUX_POSE_MAX_PAIRS = 64;

// one side's material of plfem_flux_overlap_posed: the rules of material_error, and no sampled map on its locator
const char* flux_side_error(const plfem_locator* L, double eps_core, double eps_clad, const double* layers_host, int nlayer,
                            double eps_bg, int use_profile) {
  if (const char* bad = material_error(L, eps_core, eps_clad, layers_host, nlayer, eps_bg, use_profile)) return bad;
  if (L->map.set()) return "the locator carries a sampled index map: maps are out of scope of this call (clear the map)";
  return nullptr;
}

// f(std::true_type / std::false_type) by a run-time flag
template <typename F>
void with_flag(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}
}  // namespace

extern "C" int plfem_flux_overlap_posed_work_bytes(const plfem_locator* Lb, int32_t ka, int32_t kb, int32_t nposes, int64_t* bytes) try {
  if (!Lb || !bytes || posed_sizes(ka, kb, nposes, FLUX_POSE_MAX_PAIRS)) return PLFEM_EINVAL;
  *bytes = (int64_t)posed_plan(Lb->ne, ka, kb, nposes, FT, FLUX_POSED_OUTPUTS).total;
  return PLFEM_OK;
} catch (...) { return host_failure(nullptr, 0); }

extern "C" int plfem_flux_overlap_posed(plfem_locator* La, const double* modes_a_dev, int32_t ka, int32_t indexed_a,
                                        const double* cores_a_host, int32_t ncore_a, double eps_core_a, double eps_clad_a,
                                        const double* layers_a_host, int32_t nlayer_a, double eps_bg_a, int32_t use_profile_a,
                                        plfem_locator* Lb, const double* modes_b_dev, int32_t kb, int32_t indexed_b,
                                        const double* cores_b_host, int32_t ncore_b, double eps_core_b, double eps_clad_b,
                                        const double* layers_b_host, int32_t nlayer_b, double eps_bg_b, int32_t use_profile_b,
                                        int32_t nposes, const double* poses_host, void* work_dev, int64_t work_bytes,
                                        double* out_host) try {
  if (!La) return PLFEM_EINVAL;
  FieldCall call{La, "plfem_flux_overlap_posed"};
  TRY(call.pair(Lb));
  if (const char* bad = posed_sizes(ka, kb, nposes, FLUX_POSE_MAX_PAIRS)) return call.reject(bad);
  if (!ncore_ok(ncore_a, false) || !ncore_ok(ncore_b, false)) return call.reject("ncore of each side must be in [0, 64]");
  if (!modes_a_dev || !modes_b_dev || !poses_host || !work_dev || !out_host || (ncore_a > 0 && !cores_a_host) ||
      (ncore_b > 0 && !cores_b_host))
    return call.reject("null array");
  if (const char* bad = flux_side_error(La, eps_core_a, eps_clad_a, layers_a_host, nlayer_a, eps_bg_a, use_profile_a))
    return call.reject(std::string("side A: ") + bad);
  if (const char* bad = flux_side_error(Lb, eps_core_b, eps_clad_b, layers_b_host, nlayer_b, eps_bg_b, use_profile_b))
    return call.reject(std::string("side B: ") + bad);
  // each side's layer table travels through its own locator's buffer: one locator on both sides has one table
  if (La == Lb && use_profile_a && use_profile_b &&
      (nlayer_a != nlayer_b ||
       (nlayer_a > 0 && std::memcmp(layers_a_host, layers_b_host, sizeof(double) * LAYER_DOUBLES * nlayer_a) != 0)))
    return call.reject("one locator on both sides carries one layer table: the two profiles must have the same layers");
  TRY(call.modes(indexed_a, indexed_b));
  if (!poses_ok(poses_host, nposes))
    return call.reject("every pose (tx, ty, c, s, m) must be finite with m > 0 and |c^2 + s^2 - 1| <= 1e-12");
  const PosedPlan plan = posed_plan(Lb->ne, ka, kb, nposes, FT, FLUX_POSED_OUTPUTS);
  TRY(call.work("plfem_flux_overlap_posed_work_bytes", work_dev, work_bytes, plan.total, plan.off_partial));
  double* poses = (double*)((char*)work_dev + plan.off_poses);
  Material mat_a, mat_b;
  TRY(stage_material(La, cores_a_host, ncore_a, eps_core_a, eps_clad_a, layers_a_host, nlayer_a, eps_bg_a, use_profile_a, mat_a));
  TRY(stage_material(La, cores_b_host, ncore_b, eps_core_b, eps_clad_b, layers_b_host, nlayer_b, eps_bg_b, use_profile_b, mat_b, Lb));
  const int npair = plan.nca * plan.ncb;
  const size_t per_pose = (size_t)FLUX_POSED_OUTPUTS * ka * kb;
  // the batches follow each other on one stream, as in plfem_field_overlap_posed
  for (int p0 = 0; p0 < nposes; p0 += plan.batch) {
    const int nb = std::min(plan.batch, nposes - p0);
    HIP_TRY(La, hipMemcpyAsync(poses, poses_host + (size_t)POSE_DOUBLES * p0, sizeof(double) * POSE_DOUBLES * nb,
                               hipMemcpyHostToDevice, La->stream));
    with_flag(use_profile_a != 0, [&](auto pa) {
      with_flag(use_profile_b != 0, [&](auto pb) {
        hipLaunchKernelGGL((k_flux_overlap_posed<decltype(pa)::value, decltype(pb)::value>), dim3(plan.slices, npair, nb),
                           dim3(256), 0, La->stream, call.loc, call.loc_b, (int)ka, call.nrows, modes_a_dev, mat_a, (int)kb,
                           call.nrows_b, modes_b_dev, mat_b, plan.ncb, poses, call.partial);
      });
    });
    TRY(check_launch(La, "k_flux_overlap_posed"));
    hipLaunchKernelGGL(k_overlap_reduce, dim3(npair, nb * FLUX_POSED_OUTPUTS, OC * OC / 256), dim3(256), 0, La->stream, (int)ka,
                       (int)kb, plan.slices, plan.ncb, call.partial, call.O);
    TRY(check_launch(La, "k_overlap_reduce"));
    HIP_TRY(La, hipMemcpyAsync(out_host + per_pose * p0, call.O, sizeof(double) * per_pose * nb, hipMemcpyDeviceToHost, La->stream));
  }
  HIP_TRY(La, hipStreamSynchronize(La->stream));
  return PLFEM_OK;
} catch (...) { return host_failure(La); }

namespace {
// plfem_mode_indicators: the result [k][ne], then the element-neighbour table [3][ne] int32, then the k eigenvalues
struct IndicatorLayout { size_t off_nbr, off_lam, total; };
IndicatorLayout indicator_layout(int ne, int k) {
  IndicatorLayout l;
  l.off_nbr = align256((size_t)k * ne * sizeof(double));
  l.off_lam = l.off_nbr + align256((size_t)3 * ne * sizeof(int32_t));
  l.total = l.off_lam + align256((size_t)k * sizeof(double));
  return l;
}
}  // namespace

extern "C" int plfem_indicator_work_bytes(const plfem_locator* L, int32_t ncomp, int32_t k, int64_t* bytes) {
  if (!L || !bytes || !modes_ok(ncomp, k)) return PLFEM_EINVAL;
  *bytes = (int64_t)indicator_layout(L->ne, k).total;
  return PLFEM_OK;
}

extern "C" int plfem_mode_indicators(plfem_locator* L, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                                     const double* lambda_host, double k0, double alpha_p, const double* cores_host,
                                     int32_t ncore, double eps_core, double eps_clad, const double* layers_host,
                                     int32_t nlayer, double eps_bg, void* work_dev, int64_t work_bytes, double* out_host) try {
  if (!L) return PLFEM_EINVAL;
  FieldCall call{L, "plfem_mode_indicators"};
  if (!modes_ok(ncomp, k)) return call.reject("ncomp must be 1 or 2 and k > 0");
  if (!modes_dev || !lambda_host || !work_dev || !out_host) return call.reject("null array");
  if (!std::isfinite(k0) || !std::isfinite(alpha_p)) return call.reject("k0 and alpha_p must be finite");
  for (int m = 0; m < k; ++m)
    if (!std::isfinite(lambda_host[m])) return call.reject("every eigenvalue must be finite");
  const bool profile = nlayer != 0 || L->map.set();   // the profile path: layers, a map (plfem_locator_set_index_map) or both
  if (profile) {
    if (const char* bad = profile_table_error(layers_host, nlayer, eps_bg)) return call.reject(bad);
  } else {
    if (!ncore_ok(ncore, false) || (ncore > 0 && !cores_host)) return call.reject("ncore must be in [0, 64], with a core table");
    if (!std::isfinite(eps_core) || !std::isfinite(eps_clad) || !(eps_core > 0.0) || !(eps_clad > 0.0))
      return call.reject("eps_core and eps_clad must be finite and positive");
  }
  const IndicatorLayout lay = indicator_layout(L->ne, k);
  TRY(call.enter(indexed, "plfem_indicator_work_bytes", work_dev, work_bytes, lay.total, 0));
  ensure_elem_nbr(*L->S);
  int32_t* d_nbr = (int32_t*)((char*)work_dev + lay.off_nbr);
  double* d_lam = (double*)((char*)work_dev + lay.off_lam);
  // (the call ends with a stream synchronisation: the host arrays outlive the copies, and nothing in flight reads the
  // locator's layer table of an earlier call)
  HIP_TRY(L, hipMemcpyAsync(d_nbr, L->S->elem_nbr.data(), sizeof(int32_t) * 3 * (size_t)L->ne, hipMemcpyHostToDevice, L->stream));
  HIP_TRY(L, hipMemcpyAsync(d_lam, lambda_host, sizeof(double) * k, hipMemcpyHostToDevice, L->stream));
  if (nlayer > 0)
    HIP_TRY(L, hipMemcpyAsync(L->d_layers, layers_host, sizeof(double) * LAYER_DOUBLES * nlayer, hipMemcpyHostToDevice, L->stream));
  const int kcore = profile ? 0 : (int)ncore;          // the profile path reads no cores
  const CoreTable ct = pack_cores(cores_host, kcore);
  with_constant<2, 1>(ncomp, [&](auto nco) {
    with_map(L, [&](auto... map) {
      hipLaunchKernelGGL((k_mode_indicators<decltype(nco)::value, decltype(map)...>), dim3((L->ne + IND_E - 1) / IND_E), dim3(256), 0,
                         L->stream, call.loc, (int)k, call.nrows, modes_dev, d_nbr, d_lam, k0 * k0, alpha_p, ct, kcore, eps_core,
                         eps_clad, L->d_layers, (int)nlayer, eps_bg, call.O, map...);
    });
  });
  TRY(check_launch(L, "k_mode_indicators"));
  return result_to_host(L, call.O, (size_t)k * L->ne, out_host);
} catch (...) { return host_failure(L); }

namespace {
constexpr int CG_SLICES = 256;   // most slices (partial blocks) per core and chunk pair
constexpr int CG_WG = 1024;      // workgroups of k_core_grams per chunk pair aimed at: slices = min(CG_SLICES, CG_WG / cores)
int core_gram_outputs(int ncomp) { return ncomp == 2 ? 3 : 1; }
// Work buffer of plfem_core_grams: the result [ncore][nout][k][k], the partials [ncore][nout][chunk pair][slice][OC * OC],
// the owner of every quadrature point and the per-core point lists (6 ne int32 each), counts and offsets; every part
// 256-byte aligned.  Slices: no more than the mesh has tiles, at least 1, and a function of the mesh and the core count
// alone -- the tiles a slice sums, and so the bits of an entry, must not change with the number of modes.  k_core_grams
// thus runs at most CG_WG workgroups per chunk pair and the partials take at most nout x CG_WG blocks of 8 KiB per chunk
// pair.
struct CoreGramLayout { int slices; size_t off_partial, off_owner, off_list, off_meta, total; };
CoreGramLayout core_gram_layout(int ne, int ncomp, int k, int ncore) {
  const size_t nout = core_gram_outputs(ncomp), nc = overlap_chunks(k), nq = (size_t)6 * ne;
  const int64_t ntiles = ((int64_t)nq + GT - 1) / GT;
  CoreGramLayout l;
  l.slices = (int)std::max<int64_t>(1, std::min<int64_t>({CG_SLICES, ntiles, CG_WG / ncore}));
  size_t o = align256((size_t)ncore * nout * k * k * sizeof(double));
  l.off_partial = o; o += align256((size_t)ncore * nout * nc * nc * l.slices * OC * OC * sizeof(double));
  l.off_owner = o;   o += align256(std::max<size_t>(1, nq) * sizeof(int32_t));
  l.off_list = o;    o += align256(std::max<size_t>(1, nq) * sizeof(int32_t));
  l.off_meta = o;    o += align256((size_t)2 * MAX_CORES * sizeof(int32_t));
  l.total = o;
  return l;
}
const char* core_gram_args(int ncomp, int k, int ncore) {
  if (ncomp < 1 || ncomp > 2) return "ncomp must be 1 or 2";
  if (k < 1) return "k must be >= 1";
  if (ncore < 1 || ncore > MAX_CORES) return "ncore must be in [1, 64]";
  return nullptr;
}
}  // namespace

extern "C" int plfem_core_gram_work_bytes(const plfem_locator* L, int32_t ncomp, int32_t k, int32_t ncore, int64_t* bytes) try {
  if (!L || !bytes || core_gram_args(ncomp, k, ncore)) return PLFEM_EINVAL;
  *bytes = (int64_t)core_gram_layout(L->ne, ncomp, k, ncore).total;
  return PLFEM_OK;
} catch (...) { return host_failure(nullptr, 0); }

extern "C" int plfem_core_grams(plfem_locator* L, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                                const double* cores_host, int32_t ncore, void* work_dev, int64_t work_bytes, double* out_host,
                                int64_t* count_host) try {
  if (!L) return PLFEM_EINVAL;
  FieldCall call{L, "plfem_core_grams"};
  if (const char* bad = core_gram_args(ncomp, k, ncore)) return call.reject(bad);
  if (!modes_dev || !cores_host || !work_dev || !out_host || !count_host) return call.reject("null array");
  const CoreGramLayout lay = core_gram_layout(L->ne, ncomp, k, ncore);
  TRY(call.enter(indexed, "plfem_core_gram_work_bytes", work_dev, work_bytes, lay.total, lay.off_partial));
  const CoreTable ct = pack_cores(cores_host, ncore);
  const int nc = overlap_chunks(k);
  const int64_t nq = (int64_t)6 * L->ne;
  char* base = (char*)work_dev;
  int32_t *owner = (int32_t*)(base + lay.off_owner), *list = (int32_t*)(base + lay.off_list), *meta = (int32_t*)(base + lay.off_meta);
  if (nq > 0) {
    hipLaunchKernelGGL(k_core_owner, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, L->stream, call.loc, ct, (int)ncore, owner);
    TRY(check_launch(L, "k_core_owner"));
  }
  hipLaunchKernelGGL(k_core_count, dim3(ncore), dim3(256), 0, L->stream, nq, owner, meta);
  TRY(check_launch(L, "k_core_count"));
  hipLaunchKernelGGL(k_core_fill, dim3(ncore), dim3(256), 0, L->stream, nq, owner, meta, list);
  TRY(check_launch(L, "k_core_fill"));
  with_constant<2, 1>(ncomp, [&](auto nco) {
    hipLaunchKernelGGL(k_core_grams<decltype(nco)::value>, dim3(lay.slices, nc * nc, ncore), dim3(256), 0, L->stream, call.loc,
                       (int)k, call.nrows, modes_dev, meta, list, nc, call.partial);
  });
  TRY(check_launch(L, "k_core_grams"));
  int32_t counts[MAX_CORES];
  HIP_TRY(L, hipMemcpyAsync(counts, meta, sizeof(int32_t) * ncore, hipMemcpyDeviceToHost, L->stream));
  TRY(grams_to_host(call, ncore * core_gram_outputs(ncomp), k, lay.slices, out_host));
  for (int c = 0; c < ncore; ++c) count_host[c] = counts[c];   // (the stream is synchronised)
  return PLFEM_OK;
} catch (...) { return host_failure(L); }

namespace {
constexpr int VG_MAX = 256;      // most velocities per call
constexpr size_t VG_PARTIAL_BYTES = (size_t)256 << 20;   // most partial blocks of one group
int velocity_gram_outputs(int ncomp) { return ncomp == 2 ? 4 : 3; }
// Work buffer of plfem_velocity_grams: the result [nvel][nout][k][k]; then for ONE group of `group` velocities -- at most
// VG_GROUP, and no more than VG_PARTIAL_BYTES of partial blocks hold (7 at k = 70) -- the partials
// [group][nout][chunk pair][slice][OC * OC], the vertex velocities [group][nv][2], the element flags [group][ne], the
// element lists (group x ne int32), counts and offsets; every part 256-byte aligned.  Slices: no more than the mesh has
// tiles, at least 1, a function of the mesh alone -- the tiles a slice sums, and so the bits of an entry, must change
// neither with the number of modes nor with the velocities of the call.
struct VelocityGramLayout { int slices, group; size_t off_partial, off_vel, off_flag, off_list, off_meta, total; };
VelocityGramLayout velocity_gram_layout(const plfem_locator* L, int ncomp, int k, int nvel) {
  const size_t nout = velocity_gram_outputs(ncomp), nc = overlap_chunks(k);
  const size_t ne = std::max(1, L->ne), nv = std::max(1, L->nv);
  const int64_t ntiles = ((int64_t)6 * L->ne + GT - 1) / GT;
  VelocityGramLayout l;
  l.slices = (int)std::max<int64_t>(1, std::min<int64_t>(VG_SLICES, ntiles));
  const size_t per_vel = nout * nc * nc * l.slices * OC * OC * sizeof(double);
  l.group = (int)std::max<size_t>(1, std::min<size_t>({(size_t)VG_GROUP, (size_t)nvel, VG_PARTIAL_BYTES / per_vel}));
  const size_t g = l.group;
  size_t o = align256((size_t)nvel * nout * k * k * sizeof(double));
  l.off_partial = o; o += align256(g * per_vel);
  l.off_vel = o;     o += align256(g * nv * 2 * sizeof(double));
  l.off_flag = o;    o += align256(g * ne * sizeof(int32_t));
  l.off_list = o;    o += align256(g * ne * sizeof(int32_t));
  l.off_meta = o;    o += align256((size_t)2 * VG_GROUP * sizeof(int32_t));
  l.total = o;
  return l;
}
const char* velocity_gram_args(int ncomp, int k, int nvel) {
  if (!modes_ok(ncomp, k)) return "ncomp must be 1 or 2 and k >= 1";
  if (nvel < 1 || nvel > VG_MAX) return "nvel must be in [1, 256]";
  return nullptr;
}
}  // namespace

extern "C" int plfem_velocity_gram_work_bytes(const plfem_locator* L, int32_t ncomp, int32_t k, int32_t nvel, int64_t* bytes) try {
  if (!L || !bytes || velocity_gram_args(ncomp, k, nvel)) return PLFEM_EINVAL;
  *bytes = (int64_t)velocity_gram_layout(L, ncomp, k, nvel).total;
  return PLFEM_OK;
} catch (...) { return host_failure(nullptr, 0); }

extern "C" int plfem_velocity_grams(plfem_locator* L, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                                    const double* cores_host, int32_t ncore, double eps_core, double eps_clad,
                                    const double* layers_host, int32_t nlayer, double eps_bg, int32_t use_profile,
                                    const double* velocities_host, int32_t nvel, void* work_dev, int64_t work_bytes,
                                    double* out_host, int64_t* count_host) try {
  if (!L) return PLFEM_EINVAL;
  FieldCall call{L, "plfem_velocity_grams"};
  if (const char* bad = velocity_gram_args(ncomp, k, nvel)) return call.reject(bad);
  if (!ncore_ok(ncore, false)) return call.reject("ncore must be in [0, 64]");
  if (!modes_dev || !velocities_host || !work_dev || !out_host || !count_host || (ncore > 0 && !cores_host))
    return call.reject("null array");
  const size_t per_vel = (size_t)2 * L->nv;
  for (size_t i = 0, n = (size_t)nvel * per_vel; i < n; ++i)
    if (!std::isfinite(velocities_host[i])) return call.reject("every velocity entry must be finite");
  if (const char* bad = material_error(L, eps_core, eps_clad, layers_host, nlayer, eps_bg, use_profile)) return call.reject(bad);
  const VelocityGramLayout lay = velocity_gram_layout(L, ncomp, k, nvel);
  TRY(call.enter(indexed, "plfem_velocity_gram_work_bytes", work_dev, work_bytes, lay.total, lay.off_partial));
  Material mat;
  TRY(stage_material(L, cores_host, ncore, eps_core, eps_clad, layers_host, nlayer, eps_bg, use_profile, mat));
  char* base = (char*)work_dev;
  double* d_vel = (double*)(base + lay.off_vel);
  int32_t *flag = (int32_t*)(base + lay.off_flag), *list = (int32_t*)(base + lay.off_list), *meta = (int32_t*)(base + lay.off_meta);
  const int nc = overlap_chunks(k), nout = velocity_gram_outputs(ncomp);
  int32_t counts[VG_MAX];
  for (int v0 = 0; v0 < nvel; v0 += lay.group) {
    const int nhere = std::min(lay.group, nvel - v0);
    double* O = call.O + (size_t)v0 * nout * k * k;
    if (per_vel > 0)
      HIP_TRY(L, hipMemcpyAsync(d_vel, velocities_host + (size_t)v0 * per_vel, sizeof(double) * nhere * per_vel,
                                hipMemcpyHostToDevice, L->stream));
    if (L->ne > 0) {
      hipLaunchKernelGGL(k_velocity_flag, dim3((unsigned)((L->ne + 255) / 256), nhere), dim3(256), 0, L->stream, call.loc, d_vel, flag);
      TRY(check_launch(L, "k_velocity_flag"));
    }
    hipLaunchKernelGGL(k_velocity_count, dim3(nhere), dim3(256), 0, L->stream, L->ne, flag, meta);
    TRY(check_launch(L, "k_velocity_count"));
    hipLaunchKernelGGL(k_velocity_fill, dim3(nhere), dim3(256), 0, L->stream, L->ne, flag, meta, list);
    TRY(check_launch(L, "k_velocity_fill"));
    with_constant<2, 1>(ncomp, [&](auto nco) {
      with_material(L, use_profile, [&](auto profile, auto... map) {
        hipLaunchKernelGGL((k_velocity_grams<decltype(nco)::value, decltype(profile)::value, decltype(map)...>),
                           dim3(lay.slices, nc * nc, nhere), dim3(256), 0, L->stream, call.loc, (int)k, call.nrows, modes_dev, mat,
                           d_vel, meta, list, nc, call.partial, map...);
      });
    });
    TRY(check_launch(L, "k_velocity_grams"));
    hipLaunchKernelGGL(k_overlap_reduce, dim3(nc * nc, nhere * nout, OC * OC / 256), dim3(256), 0, L->stream, (int)k, (int)k,
                       lay.slices, nc, call.partial, O);
    TRY(check_launch(L, "k_overlap_reduce"));
    hipLaunchKernelGGL(k_velocity_symmetrise, dim3((k * k + 255) / 256, nhere * nout), dim3(256), 0, L->stream, (int)k, O);
    TRY(check_launch(L, "k_velocity_symmetrise"));
    HIP_TRY(L, hipMemcpyAsync(counts + v0, meta, sizeof(int32_t) * nhere, hipMemcpyDeviceToHost, L->stream));
  }
  TRY(result_to_host(L, call.O, (size_t)nvel * nout * k * k, out_host));
  for (int v = 0; v < nvel; ++v) count_host[v] = counts[v];   // (the stream is synchronised)
  return PLFEM_OK;
} catch (...) { return host_failure(L); }

extern "C" int plfem_moment_gram_work_bytes(int32_t ncomp, int32_t k, int64_t* bytes) {
  if (!bytes || !modes_ok(ncomp, k)) return PLFEM_EINVAL;
  *bytes = (int64_t)gram_layout(moment_gram_outputs(ncomp), k).total;
  return PLFEM_OK;
}

extern "C" int plfem_moment_grams(plfem_locator* L, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                                  const double* cores_host, int32_t ncore, const double* origin_host, void* work_dev,
                                  int64_t work_bytes, double* out_host) try {
  if (!L) return PLFEM_EINVAL;
  FieldCall call{L, "plfem_moment_grams"};
  if (!modes_ok(ncomp, k)) return call.reject("ncomp must be 1 or 2 and k >= 1");
  if (!ncore_ok(ncore, false)) return call.reject("ncore must be in [0, 64]");
  if (!modes_dev || !work_dev || !out_host || !origin_host || (ncore > 0 && !cores_host)) return call.reject("null array");
  if (!std::isfinite(origin_host[0]) || !std::isfinite(origin_host[1])) return call.reject("the origin must be finite");
  const WorkLayout lay = gram_layout(moment_gram_outputs(ncomp), k);
  TRY(call.enter(indexed, "plfem_moment_gram_work_bytes", work_dev, work_bytes, lay.total, lay.off_partial));
  const CoreTable ct = pack_cores(cores_host, ncore);
  const int nc = overlap_chunks(k), nblk = gram_blocks(L->ne);
  const dim3 grid(nblk, nc * nc);
  const double ox = origin_host[0], oy = origin_host[1];
  if (ncomp == 2) {                           // a second instance for the four outputs made of K
    hipLaunchKernelGGL((k_moment_grams<2, true>), grid, dim3(256), 0, L->stream, call.loc, (int)k, call.nrows, modes_dev, ct,
                       (int)ncore, ox, oy, nc, call.partial);
    TRY(check_launch(L, "k_moment_grams"));
  }
  with_constant<2, 1>(ncomp, [&](auto nco) {
    hipLaunchKernelGGL((k_moment_grams<decltype(nco)::value, false>), grid, dim3(256), 0, L->stream, call.loc, (int)k, call.nrows,
                       modes_dev, ct, (int)ncore, ox, oy, nc, call.partial);
  });
  TRY(check_launch(L, "k_moment_grams"));
  return grams_to_host(call, moment_gram_outputs(ncomp), k, nblk, out_host);
} catch (...) { return host_failure(L); }

namespace {
constexpr int TAN_NW = 4;        // columns per group: one launch of k_profile_point_weights and of k_weighted_grams
constexpr int TAN_MAX = 256;     // most tangents per call
constexpr int TAN_MAPS = 8;      // most tangent maps per call
int tangent_gram_outputs(int ncomp) { return ncomp == 2 ? 2 : 1; }
// Work buffer of plfem_profile_tangent_grams: the result [column][nout][k][k]; the partials of ONE column group
// [TAN_NW][nout][chunk pair][GRAM_BLOCKS][OC * OC]; the point weights of one group [TAN_NW][6 ne]; the tangent rows
// [ntan][1 + 2 MAX_LAYERS] (room for the largest table: the sizer does not know nlayer), their map indices [ntan] and
// the tangent maps [nmap][ny][nx] on the locator's map grid; every part 256-byte aligned.
struct TangentGramLayout { size_t off_partial, off_weights, off_rows, off_mapidx, off_maps, total; };
TangentGramLayout tangent_gram_layout(const plfem_locator* L, int ncomp, int k, int ntan, int nmap, int moments) {
  const size_t nout = tangent_gram_outputs(ncomp), nc = overlap_chunks(k), ncol = (size_t)ntan + (moments ? 2 : 0);
  const size_t nq = std::max<size_t>(1, (size_t)6 * L->ne), npix = (size_t)L->map.nx * L->map.ny;
  TangentGramLayout l;
  size_t o = align256(ncol * nout * k * k * sizeof(double));
  l.off_partial = o; o += align256((size_t)TAN_NW * nout * nc * nc * GRAM_BLOCKS * OC * OC * sizeof(double));
  l.off_weights = o; o += align256((size_t)TAN_NW * nq * sizeof(double));
  l.off_rows = o;    o += align256(std::max<size_t>(1, ntan) * (1 + 2 * MAX_LAYERS) * sizeof(double));
  l.off_mapidx = o;  o += align256(std::max<size_t>(1, ntan) * sizeof(int32_t));
  l.off_maps = o;    o += align256(std::max<size_t>(1, (size_t)nmap * npix) * sizeof(double));
  l.total = o;
  return l;
}
const char* tangent_gram_args(const plfem_locator* L, int ncomp, int k, int ntan, int nmap, int moments) {
  if (!modes_ok(ncomp, k)) return "ncomp must be 1 or 2 and k >= 1";
  if (ntan < 0 || ntan > TAN_MAX || ntan + (moments ? 2 : 0) < 1)
    return "ntan must be in [0, 256], with at least one column (ntan + 2 moments >= 1)";
  if (nmap < 0 || nmap > std::min(ntan, TAN_MAPS)) return "nmap must be in [0, min(ntan, 8)]";
  if (nmap > 0 && !L->map.set()) return "tangent maps need a map on the locator (plfem_locator_set_index_map)";
  return nullptr;
}
}  // namespace

extern "C" int plfem_profile_tangent_gram_work_bytes(const plfem_locator* L, int32_t ncomp, int32_t k, int32_t ntan,
                                                     int32_t nmap, int32_t moments, int64_t* bytes) try {
  if (!L || !bytes || tangent_gram_args(L, ncomp, k, ntan, nmap, moments)) return PLFEM_EINVAL;
  *bytes = (int64_t)tangent_gram_layout(L, ncomp, k, ntan, nmap, moments).total;
  return PLFEM_OK;
} catch (...) { return host_failure(nullptr, 0); }

extern "C" int plfem_profile_tangent_grams(plfem_locator* L, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                                           const double* layers_host, int32_t nlayer, double eps_bg,
                                           const double* tangents_host, int32_t ntan, const double* tangent_maps_host,
                                           int32_t nmap, const int32_t* tangent_map_host, int32_t moments,
                                           const double* origin_host, void* work_dev, int64_t work_bytes,
                                           double* out_host) try {
  if (!L) return PLFEM_EINVAL;
  FieldCall call{L, "plfem_profile_tangent_grams"};
  if (const char* bad = tangent_gram_args(L, ncomp, k, ntan, nmap, moments)) return call.reject(bad);
  if (const char* bad = profile_table_error(layers_host, nlayer, eps_bg)) return call.reject(bad);
  if (!modes_dev || !work_dev || !out_host || !origin_host || (ntan > 0 && !tangents_host) ||
      (nmap > 0 && (!tangent_maps_host || !tangent_map_host)))
    return call.reject("null array");
  const int nrow = 1 + 2 * nlayer;
  const size_t npix = (size_t)L->map.nx * L->map.ny;
  for (int t = 0; t < ntan && nmap > 0; ++t)
    if (tangent_map_host[t] < -1 || tangent_map_host[t] >= nmap) return call.reject("every tangent map index must be in [-1, nmap)");
  for (size_t i = 0, n = (size_t)ntan * nrow; i < n; ++i)
    if (!std::isfinite(tangents_host[i])) return call.reject("every tangent entry must be finite");
  for (size_t i = 0, n = (size_t)nmap * npix; i < n; ++i)
    if (!std::isfinite(tangent_maps_host[i])) return call.reject("every tangent entry must be finite");
  if (!std::isfinite(origin_host[0]) || !std::isfinite(origin_host[1])) return call.reject("the origin must be finite");
  const TangentGramLayout lay = tangent_gram_layout(L, ncomp, k, ntan, nmap, moments);
  TRY(call.enter(indexed, "plfem_profile_tangent_gram_work_bytes", work_dev, work_bytes, lay.total, lay.off_partial));
  char* base = (char*)work_dev;
  double *wbuf = (double*)(base + lay.off_weights), *d_rows = (double*)(base + lay.off_rows), *d_maps = (double*)(base + lay.off_maps);
  int32_t* d_mapidx = (int32_t*)(base + lay.off_mapidx);
  // (every call of a locator that reads the table ends with a stream synchronisation: nothing in flight reads the old one)
  if (nlayer > 0)
    HIP_TRY(L, hipMemcpyAsync(L->d_layers, layers_host, sizeof(double) * LAYER_DOUBLES * nlayer, hipMemcpyHostToDevice, L->stream));
  if (ntan > 0)
    HIP_TRY(L, hipMemcpyAsync(d_rows, tangents_host, sizeof(double) * ntan * nrow, hipMemcpyHostToDevice, L->stream));
  if (nmap > 0) {
    HIP_TRY(L, hipMemcpyAsync(d_mapidx, tangent_map_host, sizeof(int32_t) * ntan, hipMemcpyHostToDevice, L->stream));
    HIP_TRY(L, hipMemcpyAsync(d_maps, tangent_maps_host, sizeof(double) * nmap * npix, hipMemcpyHostToDevice, L->stream));
  } else if (ntan > 0) {
    HIP_TRY(L, hipMemsetAsync(d_mapidx, 0xff, sizeof(int32_t) * ntan, L->stream));   // -1: no tangent has a map
  }
  const int nc = overlap_chunks(k), nblk = gram_blocks(L->ne), nout = tangent_gram_outputs(ncomp);
  const int ncol = ntan + (moments ? 2 : 0);
  const int64_t nq = (int64_t)6 * L->ne;
  const double ox = origin_host[0], oy = origin_host[1];
  for (int c0 = 0; c0 < ncol; c0 += TAN_NW) {
    const int nhere = std::min(TAN_NW, ncol - c0);
    if (nq > 0) {
      with_constant<2, 1>(ncomp, [&](auto nco) {
        with_map(L, [&](auto... map) {
          hipLaunchKernelGGL((k_profile_point_weights<decltype(nco)::value, TAN_NW, decltype(map)...>),
                             dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, L->stream, call.loc, L->d_layers, (int)nlayer,
                             eps_bg, d_rows, d_mapidx, d_maps, (int)ntan, c0, (int)(moments != 0), ox, oy, wbuf, map...);
        });
      });
      TRY(check_launch(L, "k_profile_point_weights"));
    }
    with_constant<2, 1>(ncomp, [&](auto nco) {
      hipLaunchKernelGGL((k_weighted_grams<decltype(nco)::value, TAN_NW>), dim3(nblk, nc * nc), dim3(256), 0, L->stream,
                         call.loc, (int)k, call.nrows, modes_dev, wbuf, nc, call.partial);
    });
    TRY(check_launch(L, "k_weighted_grams"));
    hipLaunchKernelGGL(k_overlap_reduce, dim3(nc * nc, nhere * nout, OC * OC / 256), dim3(256), 0, L->stream, (int)k, (int)k, nblk,
                       nc, call.partial, call.O + (size_t)c0 * nout * k * k);
    TRY(check_launch(L, "k_overlap_reduce"));
  }
  return result_to_host(L, call.O, (size_t)ncol * nout * k * k, out_host);
} catch (...) { return host_failure(L); }

namespace {
constexpr int MAPG_KMAX = 256;                 // most fields per call
constexpr int MAPG_KEY_BITS = 25;              // a key is at most (nx - 1)(ny - 1) < nx ny <= 2^24 (MAP_SAMPLES)
constexpr int64_t MAPG_MAX_RESULT = (int64_t)1 << 27;   // most doubles of one call's result (1 GiB)
int map_gradient_outputs(int ncomp) { return ncomp == 2 ? 2 : 1; }
// Work buffer of plfem_index_map_gradients: the result [k][nout][ny][nx]; the support [ny][nx]; keys and points before
// and after the sort, 4 x [6 ne] uint32; (a, b, c) of every point, 3 x [6 ne]; the densities of ONE chunk of fields
// [16][nout][6 ne]; first and last place of every cell, 2 x [(nx - 1)(ny - 1)] int32; the sort's temporary storage; every
// part 256-byte aligned.
struct MapGradientLayout { size_t off_support, off_keys, off_abc, off_dens, off_cells, off_temp, temp_bytes, total; };
MapGradientLayout map_gradient_layout(const plfem_locator* L, int ncomp, int k) {
  const size_t nout = map_gradient_outputs(ncomp), npix = (size_t)L->map.nx * L->map.ny;
  const size_t ncell = (size_t)(L->map.nx - 1) * (L->map.ny - 1), nq = std::max<size_t>(1, (size_t)6 * L->ne);
  MapGradientLayout l;
  size_t o = align256((size_t)k * nout * npix * sizeof(double));
  l.off_support = o; o += align256(npix * sizeof(int32_t));
  l.off_keys = o;    o += 4 * align256(nq * sizeof(uint32_t));
  l.off_abc = o;     o += 3 * align256(nq * sizeof(double));
  l.off_dens = o;    o += align256((size_t)MAPG_FC * nout * nq * sizeof(double));
  l.off_cells = o;   o += 2 * align256(ncell * sizeof(int32_t));
  l.temp_bytes = sort_pairs_temp_bytes(nq, MAPG_KEY_BITS);
  l.off_temp = o;    o += align256(std::max<size_t>(1, l.temp_bytes));
  l.total = o;
  return l;
}
const char* map_gradient_args(const plfem_locator* L, int ncomp, int k) {
  if (!modes_ok(ncomp, k, MAPG_KMAX)) return "ncomp must be 1 or 2 and 1 <= k <= 256";
  if (!L->map.set()) return "no map on the locator (plfem_locator_set_index_map)";
  if ((int64_t)k * map_gradient_outputs(ncomp) * L->map.nx * L->map.ny > MAPG_MAX_RESULT)
    return "k nout nx ny must be <= 2^27: call with fewer fields";
  return nullptr;
}
}  // namespace

extern "C" int plfem_index_map_gradient_work_bytes(const plfem_locator* L, int32_t ncomp, int32_t k, int64_t* bytes) try {
  if (!L || !bytes || map_gradient_args(L, ncomp, k)) return PLFEM_EINVAL;
  const MapGradientLayout lay = map_gradient_layout(L, ncomp, k);
  if (lay.temp_bytes == 0) return PLFEM_EHIP;       // (the sort could not be sized: no device)
  *bytes = (int64_t)lay.total;
  return PLFEM_OK;
} catch (...) { return host_failure(nullptr, 0); }

extern "C" int plfem_index_map_gradients(plfem_locator* L, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                                         const double* layers_host, int32_t nlayer, double eps_bg, void* work_dev,
                                         int64_t work_bytes, double* out_host, int32_t* support_host) try {
  if (!L) return PLFEM_EINVAL;
  FieldCall call{L, "plfem_index_map_gradients"};
  if (const char* bad = map_gradient_args(L, ncomp, k)) return call.reject(bad);
  if (const char* bad = profile_table_error(layers_host, nlayer, eps_bg)) return call.reject(bad);
  if (!modes_dev || !work_dev || !out_host) return call.reject("null array");
  const MapGradientLayout lay = map_gradient_layout(L, ncomp, k);
  TRY(call.enter(indexed, "plfem_index_map_gradient_work_bytes", work_dev, work_bytes, lay.total, lay.off_support));
  const int nx = L->map.nx, ny = L->map.ny, nout = map_gradient_outputs(ncomp);
  const size_t npix = (size_t)nx * ny;
  const uint32_t ncell = (uint32_t)(nx - 1) * (uint32_t)(ny - 1);
  const int64_t nq = (int64_t)6 * L->ne;
  const size_t qs = align256(std::max<size_t>(1, (size_t)nq) * sizeof(uint32_t)), ds = align256(std::max<size_t>(1, (size_t)nq) * sizeof(double));
  char* base = (char*)work_dev;
  int32_t* d_support = (int32_t*)(base + lay.off_support);
  uint32_t *key = (uint32_t*)(base + lay.off_keys), *val = (uint32_t*)(base + lay.off_keys + qs);
  uint32_t *skey = (uint32_t*)(base + lay.off_keys + 2 * qs), *sval = (uint32_t*)(base + lay.off_keys + 3 * qs);
  double *pa = (double*)(base + lay.off_abc), *pb = (double*)(base + lay.off_abc + ds), *pc = (double*)(base + lay.off_abc + 2 * ds);
  double* dens = (double*)(base + lay.off_dens);
  const size_t cs = align256((size_t)ncell * sizeof(int32_t));
  int32_t *first = (int32_t*)(base + lay.off_cells), *last = (int32_t*)(base + lay.off_cells + cs);
  // (every call of a locator that reads the table ends with a stream synchronisation: nothing in flight reads the old one)
  if (nlayer > 0)
    HIP_TRY(L, hipMemcpyAsync(L->d_layers, layers_host, sizeof(double) * LAYER_DOUBLES * nlayer, hipMemcpyHostToDevice, L->stream));
  // result, support and cell ranges: zero, whatever the buffer held; the kernels write the non-empty nodes and cells
  HIP_TRY(L, hipMemsetAsync(call.O, 0, lay.off_support + npix * sizeof(int32_t), L->stream));
  HIP_TRY(L, hipMemsetAsync(first, 0, 2 * cs, L->stream));
  if (nq > 0) {
    const dim3 qgrid((unsigned)((nq + 255) / 256));
    with_constant<2, 1>(ncomp, [&](auto nco) {
      hipLaunchKernelGGL(k_map_point_keys<decltype(nco)::value>, qgrid, dim3(256), 0, L->stream, call.loc, L->d_layers,
                         (int)nlayer, key, val, pa, pb, pc, eps_map(L->map));
    });
    TRY(check_launch(L, "k_map_point_keys"));
    HIP_TRY(L, sort_pairs(base + lay.off_temp, lay.temp_bytes, key, skey, val, sval, (size_t)nq, MAPG_KEY_BITS, L->stream));
    hipLaunchKernelGGL(k_map_cell_ranges, qgrid, dim3(256), 0, L->stream, nq, ncell, skey, first, last);
    TRY(check_launch(L, "k_map_cell_ranges"));
    const dim3 ngrid((unsigned)((npix + 3) / 4));
    for (int f0 = 0; f0 < k; f0 += MAPG_FC) {
      const int nf = std::min(MAPG_FC, k - f0);
      with_constant<2, 1>(ncomp, [&](auto nco) {
        hipLaunchKernelGGL(k_point_densities<decltype(nco)::value>, qgrid, dim3(256), 0, L->stream, call.loc, (int)k, call.nrows,
                           modes_dev, f0, nf, ncell, key, dens);
      });
      TRY(check_launch(L, "k_point_densities"));
      with_constant<2, 1>(ncomp, [&](auto nco) {
        hipLaunchKernelGGL(k_map_gather<decltype(nco)::value>, ngrid, dim3(256), 0, L->stream, nx, ny, nq, nf, first, last, sval,
                           pa, pb, pc, dens, call.O + (size_t)f0 * nout * npix, f0 == 0 ? d_support : (int32_t*)nullptr);
      });
      TRY(check_launch(L, "k_map_gather"));
    }
  }
  if (support_host)
    HIP_TRY(L, hipMemcpyAsync(support_host, d_support, sizeof(int32_t) * npix, hipMemcpyDeviceToHost, L->stream));
  return result_to_host(L, call.O, (size_t)k * nout * npix, out_host);
} catch (...) { return host_failure(L); }

namespace {
int quartic_pairs(int k) { return k * (k + 1) / 2; }
int quartic_tiles(int k) { return (quartic_pairs(k) + QP - 1) / QP; }
int quartic_tile_pairs(int k) { return quartic_tiles(k) * (quartic_tiles(k) + 1) / 2; }
// element slices per output tile: at most QB_MAX, and at most QWG partial tiles in all (a tile pair count never exceeds
// 561 = the k = 64 count, so that is always >= 1 slice)
int quartic_slices(int k) { return std::max(1, std::min(QB_MAX, QWG / quartic_tile_pairs(k))); }
WorkLayout quartic_layout(int k) {
  const size_t np = quartic_pairs(k);
  return work_layout(np * np, (size_t)quartic_slices(k) * quartic_tile_pairs(k) * QP * QP);
}
}  // namespace

extern "C" int plfem_quartic_work_bytes(int32_t ncomp, int32_t k, int64_t* bytes) {
  if (!bytes || !modes_ok(ncomp, k, QKMAX)) return PLFEM_EINVAL;
  *bytes = (int64_t)quartic_layout(k).total;
  return PLFEM_OK;
}

extern "C" int plfem_mode_quartic(plfem_locator* L, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                                  const double* cores_host, int32_t ncore, double w_core, double w_clad, void* work_dev,
                                  int64_t work_bytes, double* out_host) try {
  if (!L) return PLFEM_EINVAL;
  FieldCall call{L, "plfem_mode_quartic"};
  if (!modes_ok(ncomp, k, QKMAX)) return call.reject("ncomp must be 1 or 2 and 1 <= k <= 64");
  if (!ncore_ok(ncore, true)) return call.reject("at most 64 cores");
  if (!modes_dev || !work_dev || !out_host || (ncore > 0 && !cores_host)) return call.reject("null array");
  const WorkLayout lay = quartic_layout(k);
  TRY(call.enter(indexed, "plfem_quartic_work_bytes", work_dev, work_bytes, lay.total, lay.off_partial));
  const CoreTable ct = pack_cores(cores_host, ncore);
  const int np = quartic_pairs(k), nt = quartic_tiles(k), ntp = quartic_tile_pairs(k);
  const int nblk = element_slices(quartic_slices(k), L->ne);
  with_constant<2, 1>(ncomp, [&](auto nco) {
    hipLaunchKernelGGL(k_mode_quartic<decltype(nco)::value>, dim3(nblk, ntp), dim3(256), 0, L->stream, call.loc, (int)k, call.nrows,
                       modes_dev, ct, ncore < 0 ? -1 : (int)ncore, w_core, w_clad, np, nt, call.partial);
  });
  TRY(check_launch(L, "k_mode_quartic"));
  hipLaunchKernelGGL(k_quartic_reduce, dim3(ntp, 1, QP * QP / 256), dim3(256), 0, L->stream, np, nt, nblk, call.partial, call.O);
  TRY(check_launch(L, "k_quartic_reduce"));
  return result_to_host(L, call.O, (size_t)np * np, out_host);
} catch (...) { return host_failure(L); }

namespace {
// Tiles, element slices and work buffer of a projection: the result [nf][lb][la][2], then the partial tiles
// [tile][slice][nf][16][16], then the two factor tables, each part 256-byte aligned
struct ProjectPlan {
  int nf, maxt, ntx, nty, slices;
  int64_t tiles;
  size_t off_partial, off_xfac, off_yfac, total;   // bytes
};
ProjectPlan project_plan(int ncomp, int k, int la, int lb) {
  ProjectPlan p;
  p.nf = ncomp * k;
  p.maxt = (p.nf + 3) / 4;                                           // up to the next instance of k_mode_project
  p.maxt += p.maxt <= 16 ? p.maxt % 2 : (4 - p.maxt % 4) % 4;
  p.ntx = (la + PJ_X - 1) / PJ_X;
  p.nty = (lb + PJ_Y - 1) / PJ_Y;
  p.tiles = (int64_t)p.ntx * p.nty;
  p.slices = (int)std::max<int64_t>(1, std::min<int64_t>(PJ_SLICES, PJ_WG / p.tiles));
  size_t o = align256(sizeof(double) * 2 * p.nf * lb * la);
  p.off_partial = o; o += align256(sizeof(double) * p.slices * p.tiles * p.nf * 256);
  p.off_xfac = o;    o += align256(sizeof(double) * 3 * la);
  p.off_yfac = o;    o += align256(sizeof(double) * 3 * lb);
  p.total = o;
  return p;
}
bool project_sizes_ok(int ncomp, int k, int la, int lb) {
  return modes_ok(ncomp, k, PJ_KMAX) && la >= 1 && la <= PJ_LMAX && lb >= 1 && lb <= PJ_LMAX;
}
// every (c, s, kappa) finite and s >= 0
bool factors_ok(const double* fac, int n) {
  for (int i = 0; i < n; ++i) {
    const double* f = fac + 3 * i;
    if (!std::isfinite(f[0]) || !std::isfinite(f[1]) || !std::isfinite(f[2]) || f[1] < 0.0) return false;
  }
  return true;
}
}  // namespace

extern "C" int plfem_project_work_bytes(int32_t ncomp, int32_t k, int32_t la, int32_t lb, int64_t* bytes) {
  if (!bytes || !project_sizes_ok(ncomp, k, la, lb)) return PLFEM_EINVAL;
  *bytes = (int64_t)project_plan(ncomp, k, la, lb).total;
  return PLFEM_OK;
}

extern "C" int plfem_mode_project(plfem_locator* L, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                                  int32_t la, const double* xfac_host, int32_t lb, const double* yfac_host, void* work_dev,
                                  int64_t work_bytes, double* out_host) try {
  if (!L) return PLFEM_EINVAL;
  FieldCall call{L, "plfem_mode_project"};
  if (!project_sizes_ok(ncomp, k, la, lb)) return call.reject("ncomp must be 1 or 2, 1 <= k <= 64 and 1 <= la, lb <= 4096");
  if (!modes_dev || !xfac_host || !yfac_host || !work_dev || !out_host) return call.reject("null array");
  if (!factors_ok(xfac_host, la) || !factors_ok(yfac_host, lb))
    return call.reject("every factor (c, s, kappa) must be finite with s >= 0");
  const ProjectPlan plan = project_plan(ncomp, k, la, lb);
  TRY(call.enter(indexed, "plfem_project_work_bytes", work_dev, work_bytes, plan.total, plan.off_partial));
  double *xfac = (double*)((char*)work_dev + plan.off_xfac), *yfac = (double*)((char*)work_dev + plan.off_yfac);
  HIP_TRY(L, hipMemcpyAsync(xfac, xfac_host, sizeof(double) * 3 * la, hipMemcpyHostToDevice, L->stream));
  HIP_TRY(L, hipMemcpyAsync(yfac, yfac_host, sizeof(double) * 3 * lb, hipMemcpyHostToDevice, L->stream));
  const int nblk = element_slices(plan.slices, L->ne);
  with_constant<2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32>(plan.maxt, [&](auto mt) {
    hipLaunchKernelGGL(k_mode_project<decltype(mt)::value>, dim3((unsigned)plan.tiles, nblk), dim3(256), 0, L->stream, call.loc,
                       (int)ncomp, (int)k, call.nrows, modes_dev, (int)la, xfac, (int)lb, yfac, plan.ntx, call.partial);
  });
  TRY(check_launch(L, "k_mode_project"));
  const int64_t entries = (int64_t)plan.nf * lb * la;
  hipLaunchKernelGGL(k_project_reduce, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, L->stream, plan.nf, (int)la, (int)lb,
                     plan.ntx, nblk, call.partial, call.O);
  TRY(check_launch(L, "k_project_reduce"));
  return result_to_host(L, call.O, (size_t)2 * entries, out_host);
} catch (...) { return host_failure(L); }

namespace {
// Work buffer of a sampled projection: the result [nf][frames][2], then the partial tiles [tile of a launch][slice][nf][PS_COLS]
// of one launch's group of frame tiles, each part 256-byte aligned.  Sized for PS_SLICES slices: a mesh with fewer elements
// uses fewer.
struct SampledPlan {
  int nf, nft, tiles;
  size_t off_partial, total;   // bytes
};
SampledPlan sampled_plan(int ncomp, int k, int nfr) {
  SampledPlan p;
  p.nf = ncomp * k;
  p.nft = (p.nf + 15) / 16;                                          // up to the next instance of k_mode_project_sampled
  if (p.nft == 5) p.nft = 6;
  if (p.nft == 7) p.nft = 8;
  p.tiles = (nfr + PS_F - 1) / PS_F;
  size_t o = align256(sizeof(double) * 2 * p.nf * nfr);
  p.off_partial = o; o += align256(sizeof(double) * std::min(p.tiles, PS_GROUP) * PS_SLICES * p.nf * PS_COLS);
  p.total = o;
  return p;
}
bool sampled_sizes_ok(int ncomp, int k, int nfr) { return modes_ok(ncomp, k, PJ_KMAX) && nfr >= 1 && nfr <= PS_FRAMES; }
}  // namespace

extern "C" int plfem_project_sampled_work_bytes(int32_t ncomp, int32_t k, int32_t nf, int64_t* bytes) {
  if (!bytes || !sampled_sizes_ok(ncomp, k, nf)) return PLFEM_EINVAL;
  *bytes = (int64_t)sampled_plan(ncomp, k, nf).total;
  return PLFEM_OK;
}

extern "C" int plfem_mode_project_sampled(plfem_locator* L, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                                          int32_t nx, int32_t ny, double x0, double y0, double dx, double dy, int32_t nf,
                                          const double* frames_dev, void* work_dev, int64_t work_bytes, double* out_host) try {
  if (!L) return PLFEM_EINVAL;
  FieldCall call{L, "plfem_mode_project_sampled"};
  if (!sampled_sizes_ok(ncomp, k, nf) || nx < 2 || nx > PS_NMAX || ny < 2 || ny > PS_NMAX)
    return call.reject("ncomp must be 1 or 2, 1 <= k <= 64, 2 <= nx, ny <= 8192 and 1 <= nf <= 4096");
  const SampledGrid grid{x0, y0, 1.0 / dx, 1.0 / dy, nx, ny};
  if (!(dx > 0.0) || !(dy > 0.0) || !std::isfinite(dx) || !std::isfinite(dy) || !std::isfinite(x0) || !std::isfinite(y0) ||
      !std::isfinite(grid.inv_dx) || !std::isfinite(grid.inv_dy))
    return call.reject("x0, y0, dx, dy, 1 / dx and 1 / dy must be finite with dx, dy > 0");
  if (!modes_dev || !frames_dev || !work_dev || !out_host) return call.reject("null array");
  const SampledPlan plan = sampled_plan(ncomp, k, nf);
  TRY(call.enter(indexed, "plfem_project_sampled_work_bytes", work_dev, work_bytes, plan.total, plan.off_partial));
  const int nblk = element_slices(PS_SLICES, L->ne);                  // the mesh alone decides: a frame's bits do not depend on nf
  for (int t0 = 0; t0 < plan.tiles; t0 += PS_GROUP) {                 // (stream order keeps a group's partial tiles until its reduce)
    const int nt = std::min(PS_GROUP, plan.tiles - t0);
    with_constant<1, 2, 3, 4, 6, 8>(plan.nft, [&](auto nft) {
      hipLaunchKernelGGL(k_mode_project_sampled<decltype(nft)::value>, dim3(nt, nblk), dim3(256), 0, L->stream, call.loc, (int)ncomp,
                         (int)k, call.nrows, modes_dev, grid, (int)nf, t0, frames_dev, call.partial);
    });
    TRY(check_launch(L, "k_mode_project_sampled"));
    const int c0 = t0 * PS_COLS, c1 = std::min(2 * (int)nf, (t0 + nt) * PS_COLS);
    const int64_t entries = (int64_t)plan.nf * (c1 - c0);
    hipLaunchKernelGGL(k_project_sampled_reduce, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, L->stream, plan.nf, (int)nf,
                       c0, c1, nblk, call.partial, call.O);
    TRY(check_launch(L, "k_project_sampled_reduce"));
  }
  return result_to_host(L, call.O, (size_t)2 * plan.nf * nf, out_host);
} catch (...) { return host_failure(L); }

