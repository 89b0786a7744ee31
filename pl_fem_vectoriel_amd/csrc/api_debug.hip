// Test hooks of the library (include/plfem.h, section guarded by PLFEM_TEST_HOOKS): libplfem_testhooks.so.
// NOT part of libplfem_hip.so -- the product library exports none of these symbols and has no switch that alters a
// result.  This add-on links against the product library (it calls its internal launch_* functions and works on
// contexts the product library created), so the tests that need a hook still run the product's own kernels.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#ifndef PLFEM_TEST_HOOKS
#define PLFEM_TEST_HOOKS 1
#endif
#include "device.h"

namespace {
// a slightly wrong factor: D^-1 of the root front scaled by 1 + test_perturb after every factorisation
void perturb_root_pivots(plfem_ctx* c) {
  if (c->test_perturb != 0.0)
    plfem::launch_axpby(c, (int64_t)2 * c->dpn * c->S->fs[0], 1.0 + c->test_perturb, c->d_delta, 0.0, c->d_delta,
                        c->d_delta);              // x = (1 + p) x + 0 x: D^-1 is finite
}
}  // namespace

extern "C" int plfem_debug_set_perturb(plfem_ctx* c, double value) try {
  if (!c) return PLFEM_EINVAL;
  c->test_perturb = value;
  c->test_post_factor = value != 0.0 ? perturb_root_pivots : nullptr;
  c->factored = false;              // takes effect at the next plfem_factor
  return PLFEM_OK;
} catch (...) { return host_failure(c); }

extern "C" int plfem_debug_factor_until(plfem_ctx* c, double sigma, int32_t level, int32_t step, int32_t stage) try {
  if (!c) return PLFEM_EINVAL;
  if (!c->assembled) { c->err = "debug factor before assemble"; return PLFEM_ESTATE; }
  TRY(wait_for_upload(c));              // (as plfem_factor)
  plfem::launch_factor(c, sigma, level, step, stage);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return check_launch(c, "debug factor");
} catch (...) { return host_failure(c); }

extern "C" int plfem_debug_copy(plfem_ctx* c, const char* name, int64_t offset, int64_t count, double* out_host) try {
  if (!c || !name || !out_host || offset < 0 || count < 0) return PLFEM_EINVAL;
  std::string n(name);
  const double* src = nullptr;
  if (n == "front") src = c->d_front;
  else if (n == "schur") src = c->d_schur;            // (arena of level l starts at (l & 1) * arena_doubles)
  else if (n == "fvec") src = c->d_fvec;
  else if (n == "wbuf") src = c->d_wbuf;
  else if (n == "rbuf") src = c->d_rbuf;
  else if (n == "dinv") src = c->d_dinv;
  else if (n == "delta") src = c->d_delta;
  else if (n == "fvec2") src = c->d_fvec2;
  else if (n == "xl") src = c->d_xl;
  else if (n == "elem") src = c->d_elem;
  else if (n == "V") src = c->d_V;                      // the Lanczos basis, B times it, the projected matrix (plfem.h)
  else if (n == "BV") src = c->d_BV;
  else if (n == "Hcols") src = c->d_Hcols;
  else if (n == "counters") {                             // the 4 int32 device counters, delivered as doubles
    if (offset + count > 4) return PLFEM_EINVAL;
    int32_t tmp[4];
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(tmp, c->d_counters, sizeof(tmp), hipMemcpyDeviceToHost));
    for (int64_t q = 0; q < count; ++q) out_host[q] = (double)tmp[offset + q];
    return PLFEM_OK;
  }
  else if (n == "colind" || n == "slot_row") {            // int32 index arrays, delivered as doubles
    if (offset + count > c->nnz) return PLFEM_EINVAL;
    std::vector<int32_t> tmp((size_t)count);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(tmp.data(), (n == "colind" ? c->d_colind : c->d_slot_row) + offset, sizeof(int32_t) * count, hipMemcpyDeviceToHost));
    for (int64_t q = 0; q < count; ++q) out_host[q] = (double)tmp[q];
    return PLFEM_OK;
  }
  else return PLFEM_EINVAL;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(out_host, src + offset, sizeof(double) * count, hipMemcpyDeviceToHost));
  return PLFEM_OK;
} catch (...) { return host_failure(c); }

// The write counterpart of plfem_debug_copy("elem"): the tests' own element matrices in place of the assembled ones, then
// the product's CSR gather, so that plfem_spmv and the refinement inside the solves see the pencil the factorisation sees.
extern "C" int plfem_debug_set_elements(plfem_ctx* c, const double* elem_host) try {
  if (!c || !elem_host) return PLFEM_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(wait_for_upload(c));              // (as plfem_factor: the gather reads the uploaded adjacency)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(c->d_elem, elem_host, sizeof(double) * (size_t)c->ne * plfem::ELEM_STRIDE, hipMemcpyHostToDevice));
  plfem::launch_csr_gather(c);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  TRY(check_launch(c, "debug set elements"));
  c->assembled = true;
  c->factored = false;
  return PLFEM_OK;
} catch (...) { return host_failure(c); }

// BLOCK_P right-hand sides (global order, columns ldx apart) through the block sweeps, then refine_steps passes of block
// iterative refinement against the assembled K = A - sigma B (the block SpMVs of the Lanczos driver's refined solve).
// The refinement's scratch is the first 3 BLOCK_P columns (ldx apart) of d_V2, as in the block Lanczos driver.
extern "C" int plfem_debug_solve_block(plfem_ctx* c, const double* rhs_dev, int64_t ldx, double* x_dev, int32_t refine_steps) try {
  constexpr int P = plfem::BLOCK_P;
  if (!c || !rhs_dev || !x_dev || refine_steps < 0) return PLFEM_EINVAL;
  if (!c->factored) { c->err = "debug block solve before plfem_factor"; return PLFEM_ESTATE; }
  if (c->max_block_p < P) { c->err = "debug block solve: the LDS budget of this tree allows one right-hand side per sweep"; return PLFEM_EINVAL; }
  if (ldx < c->n2) { c->err = "debug block solve: ldx < n2"; return PLFEM_EINVAL; }
  const int64_t scratch = (int64_t)c->n2 * plfem::basis_cols(c->max_ncv);
  if (refine_steps > 0 && 3 * P * ldx > scratch) { c->err = "debug block solve: ldx too large for the refinement scratch"; return PLFEM_EINVAL; }
  HIP_TRY(c, hipSetDevice(c->device));
  plfem::solve_refined(c, P, rhs_dev, x_dev, ldx, false, refine_steps, c->d_V2, c->d_V2 + (size_t)P * ldx,
                       c->d_V2 + (size_t)2 * P * ldx);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return check_launch(c, "debug block solve");
} catch (...) { return host_failure(c); }

// The launch plan the context's sweeps and factorisation run from, PLFEM_DEBUG_PLAN_FIELDS int64 per level (level 0 =
// root): fronts, forward / backward rows per workgroup (64: tile form), mixed forward launch, largest s2, largest m,
// forward / backward workgroups, block steps of the factorisation, right-hand sides per sweep the LDS budget allows.
extern "C" int plfem_debug_level_plan(plfem_ctx* c, int64_t* out, int64_t cap) try {
  if (!c || !out) return PLFEM_EINVAL;
  const plfem::LaunchPlan& plan = *c->plan;
  const int nl = (int)plan.levels.size();
  if (cap < (int64_t)PLFEM_DEBUG_PLAN_FIELDS * nl) { c->err = "debug level plan: cap too small"; return PLFEM_EINVAL; }
  for (int l = 0; l < nl; ++l) {
    const plfem::LevelInfo& li = plan.levels[l];
    const int next = l + 1 < nl ? plan.levels[l + 1].step0 : (int)plan.upd_n.size();
    const int64_t rec[PLFEM_DEBUG_PLAN_FIELDS] = {li.count, li.fwd_rows, li.bwd_rows, li.fwd_mixed ? 1 : 0, li.max_s2, li.max_m,
                                                  li.fwd_n, li.bwd_n, next - li.step0, c->max_block_p};
    std::copy(rec, rec + PLFEM_DEBUG_PLAN_FIELDS, out + (int64_t)PLFEM_DEBUG_PLAN_FIELDS * l);
  }
  return PLFEM_OK;
} catch (...) { return host_failure(c); }

// ---- the device kernels of the Lanczos drivers on caller device buffers (kernels_lanczos.hip, block SpMVs of
// kernels_assembly.hip); every hook runs the product's launch_* function on the context's stream and synchronises
namespace {
int lanczos_hook_done(plfem_ctx* c, const char* what) {
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return check_launch(c, what);
}
}  // namespace

extern "C" int plfem_debug_panel(plfem_ctx* c, int32_t form, int32_t ncols, const double* Pm, double* W, int64_t ldw, double* H,
                                 int32_t ldh, double* hacc, int32_t ldacc, double* wil) try {
  constexpr int P = plfem::BLOCK_P;
  if (!c || !H || !Pm || !W || form < PLFEM_DEBUG_PANEL_DOT || form > PLFEM_DEBUG_PANEL_AXPY_BLOCK) return PLFEM_EINVAL;
  if (ncols < 1 || ncols > c->max_ncv + P) { c->err = "debug panel: need 1 <= ncols <= max_ncv + BLOCK_P"; return PLFEM_EINVAL; }
  const bool block = form == PLFEM_DEBUG_PANEL_DOT_BLOCK || form == PLFEM_DEBUG_PANEL_AXPY_BLOCK;
  if (block && (ldw < c->n2 || ldh < ncols || (hacc && ldacc < ncols))) { c->err = "debug panel: leading dimension too small"; return PLFEM_EINVAL; }
  HIP_TRY(c, hipSetDevice(c->device));
  switch (form) {
    case PLFEM_DEBUG_PANEL_DOT: plfem::launch_panel_dot(c, 1, Pm, ncols, W, ldw, H, ldh, hacc, ldacc); break;
    case PLFEM_DEBUG_PANEL_AXPY: plfem::launch_panel_axpy(c, 1, Pm, ncols, H, ldh, W, ldw); break;
    case PLFEM_DEBUG_PANEL_DOT_BLOCK: plfem::launch_panel_dot(c, P, Pm, ncols, W, ldw, H, ldh, hacc, ldacc); break;
    default: plfem::launch_panel_axpy(c, P, Pm, ncols, H, ldh, W, ldw, wil); break;
  }
  return lanczos_hook_done(c, "debug panel");
} catch (...) { return host_failure(c); }

extern "C" int plfem_debug_scale_store(plfem_ctx* c, const double* w, const double* bw, const double* beta2, double* v, double* bv,
                                       double* beta_out) try {
  if (!c || !w || !bw || !beta2 || !v || !bv) return PLFEM_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  plfem::launch_scale_store(c, w, bw, beta2, v, bv, beta_out);
  return lanczos_hook_done(c, "debug scale store");
} catch (...) { return host_failure(c); }

extern "C" int plfem_debug_first_pass(plfem_ctx* c, const double* xl_front, const double* BVm, const double* Vm, int32_t ncols,
                                      double* W, int64_t ldw, double* Hout, int32_t ldh) try {
  if (!c || !xl_front || !BVm || !Vm || !W || !Hout) return PLFEM_EINVAL;
  if (ncols < 1 || ncols > plfem::FIRST_COLS || ldw < c->n2 || ldh < ncols) { c->err = "debug first pass: need 1 <= ncols <= FIRST_COLS, ldw >= n2, ldh >= ncols"; return PLFEM_EINVAL; }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(c->d_xl, xl_front, sizeof(double) * 2 * c->fnodes_total * plfem::BLOCK_P, hipMemcpyDeviceToDevice, c->stream));
  plfem::launch_first_pass_block(c, BVm, Vm, ncols, W, ldw, Hout, ldh);
  return lanczos_hook_done(c, "debug first pass");
} catch (...) { return host_failure(c); }

extern "C" int plfem_debug_spmv_block(plfem_ctx* c, int32_t form, const double* x, double* y, int64_t ld, double* gram_out,
                                      int32_t* nparts) try {
  constexpr int P = plfem::BLOCK_P;
  if (!c || !x || !y || form < PLFEM_DEBUG_SPMV_B_BLOCK || form > PLFEM_DEBUG_SPMV_A_BLOCK) return PLFEM_EINVAL;
  if (!c->assembled) { c->err = "debug block spmv before assemble"; return PLFEM_ESTATE; }
  if (ld < c->n2) { c->err = "debug block spmv: ld < n2"; return PLFEM_EINVAL; }
  HIP_TRY(c, hipSetDevice(c->device));
  int np = 0;
  switch (form) {
    case PLFEM_DEBUG_SPMV_B_BLOCK: plfem::launch_spmv(c, 1, P, x, y, ld); break;
    case PLFEM_DEBUG_SPMV_B_BLOCK_IL: plfem::launch_spmv_b_block_il(c, x, y, ld); break;
    case PLFEM_DEBUG_SPMV_B_BLOCK_IL_GRAM:
      np = plfem::launch_spmv_b_block_il(c, x, y, ld, c->d_partial);      // (where the Lanczos step leaves them for the CholQR)
      if (gram_out) HIP_TRY(c, hipMemcpyAsync(gram_out, c->d_partial, sizeof(double) * P * P * np, hipMemcpyDeviceToDevice, c->stream));
      break;
    default: plfem::launch_spmv(c, 0, P, x, y, ld); break;
  }
  if (nparts) *nparts = np;
  return lanczos_hook_done(c, "debug block spmv");
} catch (...) { return host_failure(c); }

extern "C" int plfem_debug_chol(plfem_ctx* c, const double* G, int32_t ldg, int32_t use_partials, int32_t nchunks, double* Tblk,
                                int32_t ldT, double* Rinv, int32_t* rank_flag) try {
  constexpr int P = plfem::BLOCK_P;
  if (!c || !Tblk || !Rinv || ldT < P) return PLFEM_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  if (use_partials) {
    if (nchunks < 1 || (size_t)P * P * nchunks > c->partial_doubles) { c->err = "debug chol: nchunks out of range"; return PLFEM_EINVAL; }
    if (G) HIP_TRY(c, hipMemcpyAsync(c->d_partial, G, sizeof(double) * P * P * nchunks, hipMemcpyDeviceToDevice, c->stream));
  } else if (!G || ldg < P) {
    return PLFEM_EINVAL;
  }
  HIP_TRY(c, hipMemsetAsync(c->d_counters + 2, 0, sizeof(int32_t), c->stream));
  if (use_partials) plfem::launch_chol_from_partials(c, nchunks, Tblk, ldT, Rinv);
  else plfem::launch_chol_block(c, G, ldg, Tblk, ldT, Rinv);
  int32_t flag = 0;
  HIP_TRY(c, hipMemcpyAsync(&flag, c->d_counters + 2, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemsetAsync(c->d_counters + 2, 0, sizeof(int32_t), c->stream));
  TRY(lanczos_hook_done(c, "debug chol"));
  if (rank_flag) *rank_flag = flag;
  return PLFEM_OK;
} catch (...) { return host_failure(c); }

extern "C" int plfem_debug_block_scale(plfem_ctx* c, const double* W, const double* BW, int64_t ldw, const double* Rinv, double* Vn,
                                       double* BVn, int64_t ldv, const double* exp_src, int32_t exp_n, double* exp_dst,
                                       int32_t* cnt_dst, int32_t want_front) try {
  if (!c || !W || !BW || !Rinv || !Vn || !BVn || exp_n < 0) return PLFEM_EINVAL;
  if (ldw < c->n2 || ldv < c->n2) { c->err = "debug block scale: leading dimension < n2"; return PLFEM_EINVAL; }
  if (exp_dst && (!exp_src || !cnt_dst)) { c->err = "debug block scale: an export needs exp_src and cnt_dst"; return PLFEM_EINVAL; }
  HIP_TRY(c, hipSetDevice(c->device));
  plfem::launch_block_scale(c, W, BW, ldw, Rinv, Vn, BVn, ldv, exp_src, exp_dst ? exp_n : 0, exp_dst, cnt_dst,
                            want_front ? c->d_fvec : nullptr);
  return lanczos_hook_done(c, "debug block scale");
} catch (...) { return host_failure(c); }

extern "C" int plfem_debug_rotate(plfem_ctx* c, const double* V, int32_t m, const double* S, int32_t ldS, int32_t p, double* out) try {
  if (!c || !V || !S || !out) return PLFEM_EINVAL;
  if (m < 1 || m > PLFEM_MAX_NCV + plfem::BLOCK_P || p < 1 || ldS < m) { c->err = "debug rotate: need 1 <= m <= PLFEM_MAX_NCV + BLOCK_P, p >= 1, ldS >= m"; return PLFEM_EINVAL; }
  HIP_TRY(c, hipSetDevice(c->device));
  plfem::launch_rotate(c, V, m, S, ldS, p, out);
  return lanczos_hook_done(c, "debug rotate");
} catch (...) { return host_failure(c); }

extern "C" int plfem_debug_start_field(plfem_ctx* c, int32_t nvec, double* out) try {
  if (!c || !out || nvec < 1 || nvec > plfem::BLOCK_P) return PLFEM_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  plfem::launch_start_field(c, nvec, out);
  return lanczos_hook_done(c, "debug start field");
} catch (...) { return host_failure(c); }
