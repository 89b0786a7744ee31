// Device-side context of libplfem_hip.so (gfx950).  Internal header.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/plfem.h"
#include "internal.h"
#include "plan.h"

namespace plfem {

// Layout of the context's pinned host block h_pinned, offsets in doubles.  The regions hold for any k <= PLFEM_MAX_NCV
// and ncore <= MAX_CORES (the asserts below).
constexpr size_t PIN_POST = 0;         // post-processing sums, 5 k (post_enqueue / post_finish)
constexpr size_t PIN_RESID = 2048;     // residual check: lambda [0, k), sums [k, 3 k) (resid_enqueue / resid_finish)
constexpr size_t PIN_CORE_QP = 4000;   // one u64: quadrature points inside a core (launch_delta_eps_mass)
// int32 counters, shared in time: post_enqueue copies the 4 device counters here, and each of the two block-step
// slots of the block Lanczos driver writes its 4 into [4 slot, 4 slot + 4); the two never run together
constexpr size_t PIN_COUNTERS = 4096;
constexpr int PIN_COUNTERS_N = 2 * 4;  // int32 entries
constexpr size_t PIN_CORES = 6144;     // core table, 3 MAX_CORES (upload_cores)
constexpr size_t PIN_LAYERS = 6400;    // layer table of an index profile, LAYER_DOUBLES MAX_LAYERS (plfem_set_index_profile)
// projected matrix (max_ncv + 2 + BLOCK_P)^2: d_Hcols mirror, restart / Ritz rotation matrices; h_slots behind it
constexpr size_t PIN_PROJ = 8192;
static_assert(PIN_POST + 5 * PLFEM_MAX_NCV <= PIN_RESID, "pinned layout: post-processing sums");
static_assert(PIN_RESID + 3 * PLFEM_MAX_NCV <= PIN_CORE_QP, "pinned layout: residual check");
static_assert(PIN_CORE_QP + 1 <= PIN_COUNTERS, "pinned layout: core-point counter");
static_assert(PIN_COUNTERS + PIN_COUNTERS_N * sizeof(int32_t) / sizeof(double) <= PIN_CORES, "pinned layout: counters");
static_assert(PIN_CORES + 3 * MAX_CORES <= PIN_LAYERS, "pinned layout: core table");
static_assert(PIN_LAYERS + LAYER_DOUBLES * MAX_LAYERS <= PIN_PROJ, "pinned layout: layer table");

// Phases of a context timed on the device by an event pair each (plfem_timings, the *_us entries of plfem_solve_modes)
enum Phase { PH_ASSEMBLE, PH_FACTOR, PH_LANCZOS, PH_POST, PH_UPLOAD, PH_RESIDUAL, PH_COUNT };
static_assert(PLFEM_SOLVE_T_ASSEMBLE_US + PH_RESIDUAL == PLFEM_SOLVE_T_RESIDUAL_US, "phases in PLFEM_SOLVE_T_* order");

}  // namespace plfem

// Error vocabulary of the C ABI for a handle with a `std::string err` (plfem_ctx, plfem_locator): a failed HIP call or
// launch sets the handle's error text and returns PLFEM_EHIP; TRY passes a non-zero status on.
#define HIP_TRY(owner, call)                                                                 \
  do {                                                                                       \
    hipError_t e__ = (call);                                                                 \
    if (e__ != hipSuccess) {                                                                 \
      (owner)->err = std::string(#call) + ": " + hipGetErrorString(e__);                     \
      return PLFEM_EHIP;                                                                     \
    }                                                                                        \
  } while (0)

#define TRY(x)                         \
  do {                                 \
    int rc__ = (x);                    \
    if (rc__ != PLFEM_OK) return rc__; \
  } while (0)

namespace plfem {
// The sampled map of an index profile as a handle keeps it (plfem_set_index_map, plfem_locator_set_index_map): a device
// buffer of the handle's own -- not part of the context's slab or of the locator's memory, so no other buffer moves --
// that is reused while it is large enough and freed on clear and destroy, and the grid of the map in it.
struct IndexMap {
  double* d = nullptr;            // MAP_HEADER doubles that hold the grid as the kernels read it, then [ny][nx] permittivities
  size_t cap = 0;                 // permittivities the buffer has room for
  int nx = 0, ny = 0;             // 0: no map set
  double x0 = 0, y0 = 0, inv_dx = 0, inv_dy = 0;
  bool set() const { return nx > 0; }
};
// the grid as the first bytes of the buffer hold it: SampledGrid of p2_element.h, field for field
struct IndexMapHeader {
  double x0, y0, inv_dx, inv_dy;
  int nx, ny;
};
static_assert(sizeof(IndexMapHeader) <= MAP_HEADER * sizeof(double), "the grid fits the map buffer's header");
}  // namespace plfem

struct plfem_ctx {
  const plfem::Symbolic* S = nullptr;
  const plfem::LaunchPlan* plan = nullptr;   // S->plan: kernel forms by level, launch order, workgroup lists (plan.h)
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  // sizes
  int nv = 0, ne = 0, N = 0, nnz = 0, nsolve = 0, L = 0, nfronts = 0, max_ncv = 0;
  int dpn = 2, sh = 1;            // unknowns per node (2: Hx, Hy; 1: scalar Helmholtz) and sh = dpn - 1: node = dof >> sh, component = dof & sh
  int64_t fnodes_total = 0;       // sum over fronts of (padded) nodes = fnode_ptr[nfronts]
  int64_t n2 = 0;   // dpn N: length of every global vector (component-major blocks of N)
  // ---- index structures on the device
  int32_t* d_forder = nullptr;    // [nfronts] per level: front ids in order of decreasing s2 (factorisation launches)
  plfem::FrontRec* d_frec = nullptr;   // the same order, with the front's parameters
  int2* d_tiles = nullptr;        // (front, tx | ty << 16) of every useful 64 x 64 workgroup of the factorisation
  plfem::SweepJob* d_blk = nullptr;   // one entry per sweep workgroup, level by level
  int32_t *d_tsorted = nullptr, *d_edof = nullptr, *d_rowptr = nullptr, *d_colind = nullptr;
  int32_t *d_slot_row = nullptr, *d_nptr = nullptr, *d_nadj = nullptr, *d_interior = nullptr;
  uint8_t* d_nloc = nullptr;
  uint8_t* d_bmask = nullptr;
  double* d_doflocs = nullptr;
  int32_t *d_fs2 = nullptr, *d_fm = nullptr;          // per front: owned DOFs (2 fs), front order m = 2 (fs + fb)
  int64_t *d_fnode_ptr = nullptr, *d_foff = nullptr;
  int32_t *d_fnodes = nullptr, *d_cinv0 = nullptr, *d_cinv1 = nullptr;
  int32_t *d_epos = nullptr, *d_leaf_elem_ptr = nullptr, *d_leaf_elems = nullptr;
  // ---- numeric data
  double* d_cores = nullptr;      // [64][3]
  double* d_layers = nullptr;     // [64][8] layer table of the index profile (plfem_set_index_profile)
  int nlayer = 0;                 // > 0: the assembly takes its permittivity from the profile, not from eps_core / eps_clad
  double eps_bg = 0.0;            // the profile's background permittivity (0: none given)
  plfem::IndexMap map;            // the sampled map under the layers (plfem_set_index_map); set: the profile path, layers or not
  double* d_elem = nullptr;       // [ne][8][36]
  double* d_vals[PLFEM_BLK_COUNT] = {nullptr};
  double* d_front = nullptr;      // what a front keeps: [F11; F21] (m x s2) and Z^T (s2 x b2), see symbolic.h
  double* d_schur = nullptr;      // two arenas (even / odd tree levels) of arena_doubles for the Schur complements in flight
  int64_t arena_doubles = 0;
  int64_t* d_soff = nullptr;      // per front: offset of its Schur complement inside its level's arena
  double* d_fvec = nullptr;       // per-front solve vectors in front order, offset 2*fnode_ptr[f]: right-hand side (owned rows)
  double *d_u0 = nullptr, *d_u1 = nullptr;   // updates pushed into a front's rows by its left / right child (forward sweep)
  double* d_xl = nullptr;         // complete local solution of every front (backward sweep)
  int32_t* d_npos = nullptr;      // [N] node -> front-order offset of its component 0: 2 fnode_ptr[owner] + dpn * local index, -1 = Dirichlet
  int32_t* d_prow = nullptr;      // per local node of a front: local node index in the PARENT front, -1 = none / padding
  double *d_wbuf = nullptr, *d_rbuf = nullptr;   // per-front panels m x NB of the level in flight, offset 2*(fnode_ptr[f] - fnode_ptr[level first])*NB;
                                                 // three thirds (block steps mod 3).  d_schur, d_wbuf, d_rbuf (alive during a factorisation
                                                 // only) share their part of the workspace with d_V, d_BV, d_V2, d_BV2 (alive during a Lanczos run only)
  double* d_dinv = nullptr;       // 2 x per-front NB x NB (inverse of the unit-lower pivot block of even / odd block steps)
  double* d_delta = nullptr;      // per-front D^-1 of the block LDL^T: (diagonal, off-diagonal of the node pair) per row, offset 2 * (2*fnode_ptr[f])
  double* d_fvec2 = nullptr;      // forward-sweep results of the owned rows (t = L11^-1 r; the backward sweep applies D^-1), front order
  int32_t* d_counters = nullptr;  // [0] pivot perturbations
  // ---- Lanczos workspace
  double *d_V = nullptr, *d_BV = nullptr, *d_V2 = nullptr, *d_BV2 = nullptr;   // n2 x (max_ncv+1), column major
  double *d_w = nullptr, *d_bw = nullptr, *d_t1 = nullptr, *d_t2 = nullptr;    // n2 (d_w, d_bw: n2 x BLOCK_P)
  double *d_hblk = nullptr, *d_G = nullptr, *d_Rinv = nullptr;                 // block Lanczos small matrices
  double *d_h = nullptr, *d_hacc = nullptr, *d_partial = nullptr, *d_scal = nullptr, *d_S = nullptr;
  double* d_Hcols = nullptr;      // (max_ncv+1) x (max_ncv+1) projected matrix columns
  uint8_t* d_coremask = nullptr;  // [N]
  double* d_post = nullptr;       // partial sums: post-processing in [0, post_doubles), residual check behind it
  size_t post_doubles = 0;
  size_t partial_doubles = 0;     // capacity of d_partial: the largest of its three users' needs (create_impl)
  double* h_pinned = nullptr;     // pinned staging, regions plfem::PIN_*
  size_t h_pinned_bytes = 0;      // size of that block (it returns to a process-wide cache)
  double* h_staging = nullptr;    // pinned staging block of the one upload of the host arrays (same cache)
  size_t h_staging_bytes = 0;
  double* h_slots = nullptr;      // pinned: new projected-matrix columns of the two block steps in flight
  char* slab = nullptr;           // the one device allocation every buffer above is carved from
  size_t slab_off = 0, slab_bytes = 0;
  bool own_slab = false;
  int64_t workspace_need = 0;
  // state
  bool assembled = false, factored = false;
  hipEvent_t ev_step[2] = {nullptr, nullptr};   // block Lanczos: completion of the two block steps in flight
  bool defer_sync = false;        // plfem_solve_modes: the Lanczos drivers leave their final stream synchronisation to it
  hipStream_t copy_stream = nullptr;   // plfem_solve_modes: side stream of the device-to-host copy of the mode vectors
  hipEvent_t ev_copy = nullptr;        // "mode vectors ready" (main stream -> copy stream)
  hipEvent_t ev_upload = nullptr;      // "front-level index arrays uploaded" (copy stream -> main stream)
  bool upload_pending = false;
  // live kernel timing (plfem_profile_*): event pairs around every tile-form forward-sweep launch
  bool prof_on = false;
  unsigned prof_toggle = 0;       // block solves alternate between timing whole sweeps and timing single launches
  int prof_n = 0, prof_max = 0;
  std::vector<hipEvent_t> prof_ev;   // taken from the process-wide pool at profile_begin, handed back at profile_end
  std::vector<int> prof_slot;        // PLFEM_PROF_* of every timed range
  std::vector<double> prof_rbytes;   // algorithmic bytes of every timed range
  // options (plfem_set_option)
  int refine_steps = 0;           // iterative-refinement passes inside every OP application of the Lanczos drivers
  // Test hooks: nothing in libplfem_hip.so sets these (no option, no export).  The add-on libplfem_testhooks.so
  // (api_debug.hip, plfem_debug_*) installs them on a context the tests hand it.
  void (*test_post_factor)(plfem_ctx*) = nullptr;   // called at the end of every plfem_factor
  double test_perturb = 0.0;      // plfem_debug_set_perturb: relative perturbation of the root front's D^-1
  int max_block_p = plfem::BLOCK_P;   // right-hand sides per sweep the LDS budget allows (BLOCK_P or 1)
  double sigma = 0.0;
  hipEvent_t ev[plfem::PH_COUNT][2] = {};   // device timing of the phases (phase_begin / phase_end)
  bool ev_used[plfem::PH_COUNT] = {};
  double* modes_dev = nullptr;    // where the last eigen-solve left its vectors (caller's buffer or the context's own)
  int modes_k = 0;
};

namespace {
// HIP_TRY for the kernel launches just made (hipGetLastError): the message names `what`
template <class Owner>
int check_launch(Owner* owner, const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return PLFEM_OK;
  owner->err = std::string(what) + ": " + hipGetErrorString(e);
  return PLFEM_EHIP;
}

// the front-level index arrays travel on the copy stream (flush_uploads): their first reader orders the context's stream
// behind them
int wait_for_upload(plfem_ctx* c) {
  if (!c->upload_pending) return PLFEM_OK;
  HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_upload, 0));
  c->upload_pending = false;
  return PLFEM_OK;
}

hipError_t phase_begin(plfem_ctx* c, plfem::Phase ph) { return hipEventRecord(c->ev[ph][0], c->stream); }
hipError_t phase_end(plfem_ctx* c, plfem::Phase ph) {
  const hipError_t e = hipEventRecord(c->ev[ph][1], c->stream);
  if (e == hipSuccess) c->ev_used[ph] = true;
  return e;
}
// device time of the phase's last run in microseconds (0 if it has not run); its events must have completed
double phase_us(const plfem_ctx* c, plfem::Phase ph) {
  float ms = 0;
  return (c->ev_used[ph] && hipEventElapsedTime(&ms, c->ev[ph][0], c->ev[ph][1]) == hipSuccess) ? ms * 1e3 : 0.0;
}
}  // namespace

namespace plfem {

// live timing (plfem_profile_*): a timed range = two HIP events on the context's stream around one or more launches
inline int prof_open(plfem_ctx* c, int slot, double bytes) {
  if (!c->prof_on || c->prof_n >= c->prof_max) return -1;
  while ((int)c->prof_ev.size() < 2 * (c->prof_n + 1)) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return -1;
    c->prof_ev.push_back(e);
  }
  const int id = c->prof_n++;
  c->prof_slot.push_back(slot);
  c->prof_rbytes.push_back(bytes);
  (void)hipEventRecord(c->prof_ev[2 * id], c->stream);
  return id;
}
inline void prof_close(plfem_ctx* c, int id) {
  if (id >= 0) (void)hipEventRecord(c->prof_ev[2 * id + 1], c->stream);
}

// A run-time value as a template argument: f(std::integral_constant<int, V>()) for the V of the list that equals v (the
// last one if none does).  A launch with a template-valued kernel is then written once, inside a generic lambda.
template <int V, int... Rest, class F>
inline void with_constant(int v, F&& f) {
  if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, V>());
  else if (v == V) f(std::integral_constant<int, V>());
  else with_constant<Rest...>(v, f);
}

// Sums V (a power of two <= 64) per-lane values over the 64 lanes with V - 1 + log2(64 / V) shuffles instead of
// 6 V: each butterfly step halves the values a lane still carries.  On return a[0] of lane l is the complete sum
// of value multi_reduce_index<V>(l); lanes 0 .. V-1 cover every value once.  Fixed order, so deterministic.
// DESC = false pairs lanes 1, 2, 4, .. apart (the sweeps' order).  DESC = true pairs them 32, 16, .. apart: every value
// is then summed in exactly the order of the plain six-step reduction `for (off = 32; off >= 1; off >>= 1) v += shfl_xor(v, off)`
// -- the same bits -- and value multi_reduce_index<V, true>(l) ends up in lane l (each value in 64 / V neighbouring lanes).
template <int V, bool DESC = false>
__device__ __forceinline__ int multi_reduce_index(int lane) {
  int idx = 0;
#pragma unroll
  for (int h = V / 2, s = 0; h >= 1; h >>= 1, ++s) idx += ((DESC ? lane >> (5 - s) : lane >> s) & 1) ? h : 0;
  return idx;
}

// (the butterfly steps are a compile-time recursion: as a loop over h = V/2, V/4, .. the V = 32 instance was not unrolled
// and its array went to scratch, and the sweeps' instances indexed theirs through chains of v_cndmask: DESIGN section 25)
template <int H, int BIT, bool DESC, int V>
__device__ __forceinline__ void multi_reduce_step(double (&a)[V], int lane) {
  if constexpr (H >= 1) {
    const bool up = (lane & BIT) != 0;
#pragma unroll
    for (int k = 0; k < H; ++k) {
      const double send = up ? a[k] : a[k + H];
      const double keep = up ? a[k + H] : a[k];
      a[k] = keep + __shfl_xor(send, BIT);
    }
    multi_reduce_step<H / 2, DESC ? BIT / 2 : 2 * BIT, DESC>(a, lane);
  }
}

template <int V, bool DESC = false>
__device__ __forceinline__ void multi_reduce(double (&a)[V], int lane) {
  multi_reduce_step<V / 2, DESC ? 32 : 1, DESC>(a, lane);
  if constexpr (DESC) {
#pragma unroll
    for (int off = 32 / V; off >= 1; off >>= 1) a[0] += __shfl_xor(a[0], off);
  } else {
#pragma unroll
    for (int off = V; off < 64; off <<= 1) a[0] += __shfl_xor(a[0], off);
  }
}

// Below, beside every launch function: the grid and scratch numbers it is shaped by (constants: plan.h).  Whoever else
// needs one -- create_impl for the buffer sizes, the test hooks for their bounds -- calls these.
inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
// columns of the basis buffers d_V, d_BV (and restart copies): max_ncv, then the residual column or block
inline int basis_cols(int max_ncv) { return max_ncv + 1 + BLOCK_P; }
// column capacity of the projected-matrix blocks d_h, d_hacc, d_hblk and of one panel dot (its partials in d_partial)
inline int proj_cols(int max_ncv) { return basis_cols(max_ncv) + 8; }

// An index profile as the C ABI takes it (plfem_set_index_profile, plfem_profile_grams): nullptr if the table is
// acceptable, otherwise what is wrong with it
inline const char* profile_table_error(const double* layers, int nlayer, double eps_bg) {
  if (nlayer < 0 || nlayer > MAX_LAYERS) return "nlayer must be in [0, 64]";
  if (nlayer > 0 && !layers) return "null layer table";
  if (!std::isfinite(eps_bg) || !(eps_bg > 0.0)) return "the background permittivity must be finite and positive";
  for (int l = 0; l < nlayer; ++l) {
    const double* p = layers + LAYER_DOUBLES * l;
    for (int j = 0; j < LAYER_DOUBLES; ++j)
      if (!std::isfinite(p[j])) return "every layer entry must be finite";
    if (p[2] < 0.0) return "r_in must be >= 0";
    if (!(p[3] > p[2])) return "r_out must be > r_in";
    if (!(p[4] > 0.0) || !(p[5] > 0.0)) return "permittivities must be positive";
    if (p[6] < 0.0) return "g must be >= 0";
  }
  return nullptr;
}

// A sampled map as the C ABI takes it (plfem_set_index_map, plfem_locator_set_index_map): nullptr if it is acceptable,
// otherwise what is wrong with it
inline const char* index_map_error(const double* eps, int nx, int ny, double x0, double y0, double dx, double dy) {
  if (nx < 2 || ny < 2 || nx > MAP_NMAX || ny > MAP_NMAX || (int64_t)nx * ny > MAP_SAMPLES)
    return "nx and ny must be in [2, 8192] with nx ny <= 2^24 (a null map with nx = ny = 0 clears)";
  if (!eps) return "null map";
  if (!std::isfinite(x0) || !std::isfinite(y0)) return "the origin must be finite";
  if (!std::isfinite(dx) || !std::isfinite(dy) || !(dx > 0.0) || !(dy > 0.0) || !std::isfinite(1.0 / dx) ||
      !std::isfinite(1.0 / dy))
    return "the steps must be finite and positive, with finite inverses";
  for (int64_t i = 0, n = (int64_t)nx * ny; i < n; ++i)
    if (!std::isfinite(eps[i]) || !(eps[i] > 0.0)) return "every permittivity must be finite and positive";
  return nullptr;
}

// What both entries do on a handle with `err`, `device`, `stream` and `map`.  A null map with nx = ny = 0 clears: the
// buffer is freed.  A rejected map leaves the handle as it was.  The copy goes behind whatever the handle's stream still
// runs on the old map and is waited for: the caller's array is free on return.
template <class Owner>
int set_index_map(Owner* o, const char* entry, const double* eps, int nx, int ny, double x0, double y0, double dx, double dy) {
  IndexMap& m = o->map;
  const bool clear = !eps && nx == 0 && ny == 0;
  if (!clear) {
    if (const char* bad = index_map_error(eps, nx, ny, x0, y0, dx, dy)) {
      o->err = std::string(entry) + ": " + bad;
      return PLFEM_EINVAL;
    }
  }
  if (clear && !m.d) return PLFEM_OK;                // (nothing to free: no device call)
  HIP_TRY(o, hipSetDevice(o->device));
  const size_t n = clear ? 0 : (size_t)nx * ny;
  if (clear || m.cap < n) {
    HIP_TRY(o, hipStreamSynchronize(o->stream));     // nothing in flight may still read the old buffer
    double* old = m.d;
    m = IndexMap();
    if (old) HIP_TRY(o, hipFree(old));
    if (clear) return PLFEM_OK;
    HIP_TRY(o, hipMalloc((void**)&m.d, sizeof(double) * (MAP_HEADER + n)));
    m.cap = n;
  }
  m.nx = 0;                                          // (no map while a copy can still fail)
  const IndexMapHeader head{x0, y0, 1.0 / dx, 1.0 / dy, nx, ny};
  HIP_TRY(o, hipMemcpyAsync(m.d, &head, sizeof(head), hipMemcpyHostToDevice, o->stream));
  HIP_TRY(o, hipMemcpyAsync(m.d + MAP_HEADER, eps, sizeof(double) * n, hipMemcpyHostToDevice, o->stream));
  HIP_TRY(o, hipStreamSynchronize(o->stream));
  m.x0 = head.x0; m.y0 = head.y0; m.inv_dx = head.inv_dx; m.inv_dy = head.inv_dy;
  m.nx = nx; m.ny = ny;
  return PLFEM_OK;
}
inline void free_index_map(IndexMap& m) {
  if (m.d) (void)hipFree(m.d);
  m = IndexMap();
}

// kernels_assembly.hip
void launch_element_matrices(plfem_ctx* c, int ncore, double eps_core, double eps_clad, double k0, double alpha_p);
void launch_element_matrices_scalar(plfem_ctx* c, int ncore, double eps_core, double eps_clad, double k0);
double launch_delta_eps_mass(plfem_ctx* c, int ncore, double eps_core, double eps_clad);   // MINV slot <- asm((eps - mean eps) u v)
void launch_csr_gather(plfem_ctx* c);
void launch_pattern_fill(plfem_ctx* c);   // colind / slot_row from the node -> element adjacency (once per context)
// y_q = A x_q (which = 0) or B x_q (which = 1) for P vectors ld apart.  Here and below P is 1 or BLOCK_P.
void launch_spmv(plfem_ctx* c, int which, int P, const double* x, double* y, int64_t ld);
// y_q = B x_q for BLOCK_P vectors, x as [node][component][q]; gram != nullptr: also the chunk partials of the Gram matrix
// x^T (B x), gram[(p P + q) nb + b] for workgroup b of nb (returned)
int launch_spmv_b_block_il(plfem_ctx* c, const double* x_interleaved, double* y, int64_t ld, double* gram = nullptr);
inline int spmv_workgroups(int N) { return ceil_div(N, SPMV_WG_ROWS); }
inline size_t gram_partial_doubles(int N) { return (size_t)BLOCK_P * BLOCK_P * spmv_workgroups(N); }
// out_host[i] = ||A v_i - lambda_i B v_i|| / ||A v_i||  (k vectors, row i of evecs; synchronises)
void launch_residuals(plfem_ctx* c, int k, const double* lam_host, const double* evecs, double* out_host);
// kernels_front.hip (factorisation), kernels_sweep.hip (solve sweeps)
void launch_factor(plfem_ctx* c, double sigma, int stop_level = -1, int stop_step = 0, int stop_stage = 0);
// P right-hand sides, columns ldx apart; x == nullptr: the result stays in front order in d_xl (the caller permutes it itself)
void launch_solve(plfem_ctx* c, int P, const double* rhs, double* x, int64_t ldx, bool rhs_in_front_order = false);
// LDS of a sweep workgroup for a front of order m: its P right-hand sides staged in planes of sweep_ldv(m) doubles
// (dynamic; even: the row forms read the planes as double2) and the static partial-sum tile of the backward tile form
// (8 waves x P x 64).  plfem_create decides P from it: past the device limit a launch fails as "invalid argument".
inline int sweep_ldv(int m) { return (m + 2) & ~1; }
inline size_t sweep_dynamic_lds(int P, int m) { return sizeof(double) * P * sweep_ldv(m); }
inline size_t sweep_lds(int P, int m) { return sweep_dynamic_lds(P, m) + sizeof(double) * 8 * P * 64; }
// y = K^-1 b, then `steps` passes y += K^-1 (b - K y) against the assembled K; scratch ta, tb, dy: P columns ld apart each
void solve_refined(plfem_ctx* c, int P, const double* b, double* y, int64_t ld, bool b_in_front_order, int steps, double* ta,
                   double* tb, double* dy);
// kernels_lanczos.hip
// panel products on P vectors (columns ldw apart); H matrices are column major with leading dimension ldh
// h = Pm^T W (ncols x P); hacc (optional) += the same coefficients
void launch_panel_dot(plfem_ctx* c, int P, const double* Pm, int ncols, const double* W, int64_t ldw, double* h, int ldh,
                      double* hacc = nullptr, int ldacc = 0);
inline int panel_chunks(int64_t n2) { return ceil_div(n2, PANEL_CHUNK); }
inline size_t panel_dot_partial_doubles(int64_t n2, int ncols) { return (size_t)panel_chunks(n2) * ncols * BLOCK_P; }
// W -= Pm H; w_interleaved (block only): see k_spmv_b_block_il
void launch_panel_axpy(plfem_ctx* c, int P, const double* Pm, int ncols, const double* H, int ldh, double* W, int64_t ldw,
                       double* w_interleaved = nullptr);
void launch_dot(plfem_ctx* c, const double* a, const double* b, double* out);                  // *out = a.b
void launch_scale_store(plfem_ctx* c, const double* w, const double* bw, const double* beta2, double* v, double* bv,
                        double* beta_out);  // v = w/sqrt(beta2), bv = bw/sqrt(beta2)
void launch_axpby(plfem_ctx* c, int64_t n, double a, const double* x, double b, const double* y, double* z);  // z = a x + b y
void launch_rotate(plfem_ctx* c, const double* V, int m, const double* Smat, int ldS, int p, double* out);  // out = V[:, :m] S
// first Gram-Schmidt pass of a block step over ncols <= FIRST_COLS columns in two launches: reads the sweeps' result d_xl (front
// order), writes W in global order (what k_permute_out would have done), h = BVm^T W -> Hout, W -= Vm h
void launch_first_pass_block(plfem_ctx* c, const double* BVm, const double* Vm, int ncols, double* W, int64_t ldw, double* Hout, int ldh);
inline int first_pass_segments(int64_t n2) { return ceil_div(n2, FIRST_ROWS); }
inline size_t first_pass_partial_doubles(int64_t n2) { return (size_t)FIRST_COLS * BLOCK_P * first_pass_segments(n2); }
// the Cholesky half alone, from nchunks Gram partials per entry already in d_partial (launch_spmv_b_block_il with gram)
void launch_chol_from_partials(plfem_ctx* c, int nchunks, double* Tblk, int ldT, double* Rinv);
void launch_chol_block(plfem_ctx* c, const double* G, int ldg, double* Tblk, int ldT, double* Rinv);
void launch_block_scale(plfem_ctx* c, const double* W, const double* BW, int64_t ldw, const double* Rinv, double* Vn,
                        double* BVn, int64_t ldv, const double* exp_src = nullptr, int exp_n = 0, double* exp_dst = nullptr,
                        int32_t* cnt_dst = nullptr, double* bv_front = nullptr);
void launch_start_field(plfem_ctx* c, int nvec, double* out);
void launch_post(plfem_ctx* c, int k, double* evecs, int ncore, double* out_host, double* frac_core, double* modes_int);
// the same in two halves (plfem_solve_modes: one stream synchronisation for everything behind the Lanczos run)
void post_enqueue(plfem_ctx* c, int k, double* evecs, int ncore, double* modes_int, const std::function<void(int, int)>* group_done);
void post_finish(plfem_ctx* c, int k, double* out_host, double* frac_core);
void resid_enqueue(plfem_ctx* c, int k, const double* lam_host, const double* evecs);
void resid_finish(plfem_ctx* c, int k, double* out_host);
// the sums of both: per mode one partial per workgroup of POST_ROWS rows, then the totals
inline int post_blocks(int N) { return ceil_div(N, POST_ROWS); }
inline size_t post_sum_doubles(int N, int modes) { return (size_t)POST_SUMS * modes * (post_blocks(N) + 1); }
inline size_t resid_sum_doubles(int N, int modes) { return (size_t)RESID_SUMS * modes * (post_blocks(N) + 1); }

}  // namespace plfem
