// C-ABI of the device half of libplfem_hip.so: context, assembly, SpMV, factor/solve, the
// thick-restart Lanczos driver and post-processing (include/plfem.h).
#include <algorithm>
#include <atomic>
#include <memory>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <mutex>
#include <numeric>
#include <thread>
#include <vector>

#include "device.h"
#include "host_eig.h"
#include "p2_element.h"

using plfem::Symbolic;

namespace {
// Process-wide state: recycling pools of what is slow to create (hipHostMalloc / hipHostFree pin and unpin pages through
// the driver, a HIP event costs ~10 us, a stream ~50 us) and would otherwise be created by every context of a cold-solve
// loop.  Each pool is one object with its own mutex, created on first use and never destroyed (no exit-order hazard).
template <class T>
T& process_wide() {
  static T* t = new T();
  return *t;
}

// Idle HIP handles, one LIFO list per (device ordinal, kind): a handle belongs to the device that was current when it was
// created.  give() keeps at most `cap` handles in the list and destroys the rest; it never throws (no memory: destroyed).
template <class H, hipError_t (*Destroy)(H)>
struct Recycler {
  std::mutex m;
  std::vector<std::vector<H>> lists;   // [device * 4 + kind]
  std::vector<H>& list(int device, int kind) {
    const size_t i = (size_t)device * 4 + kind;
    if (lists.size() <= i) lists.resize(i + 1);
    return lists[i];
  }
  bool take(int device, int kind, H* out) {
    std::lock_guard<std::mutex> lk(m);
    auto& l = list(device, kind);
    if (l.empty()) return false;
    *out = l.back();
    l.pop_back();
    return true;
  }
  void give(int device, int kind, H h, size_t cap) noexcept {
    if (!h) return;
    try {
      std::lock_guard<std::mutex> lk(m);
      auto& l = list(device, kind);
      if (l.size() < cap) { l.push_back(h); return; }
    } catch (const std::exception&) {
    }
    (void)Destroy(h);
  }
  // every idle handle of the list moves to `mine` / every handle of `mine` moves back (plfem_profile_begin / _end: two
  // contexts profiling at once never share a vector -- the second one simply creates its own events)
  void take_all(int device, int kind, std::vector<H>& mine) {
    std::lock_guard<std::mutex> lk(m);
    auto& l = list(device, kind);
    mine.insert(mine.end(), l.begin(), l.end());
    l.clear();
  }
  void give_all(int device, int kind, std::vector<H>& mine) noexcept {
    for (H h : mine) give(device, kind, h, SIZE_MAX);
    mine.clear();
  }
};
// Events by kind: the dozen a context owns (phase timing pairs; block-step completion and copy hand-over, without
// timing), at most 256 idle per kind, and the timing events of plfem_profile_* (taken and given back whole).  Streams:
// the side streams of the mode-vector copy (plfem_solve_modes).
enum EventKind { EV_TIMING, EV_NO_TIMING, EV_PROFILE };
using EventPool = Recycler<hipEvent_t, hipEventDestroy>;
using StreamPool = Recycler<hipStream_t, hipStreamDestroy>;

hipError_t ctx_event_acquire(int device, EventKind kind, hipEvent_t* out) {
  if (process_wide<EventPool>().take(device, kind, out)) return hipSuccess;
  return kind == EV_TIMING ? hipEventCreate(out) : hipEventCreateWithFlags(out, hipEventDisableTiming);
}
void ctx_event_release(int device, EventKind kind, hipEvent_t e) { process_wide<EventPool>().give(device, kind, e, 256); }

hipError_t copy_stream_acquire(int device, hipStream_t* out) {
  if (process_wide<StreamPool>().take(device, 0, out)) return hipSuccess;
  return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}

// Pinned host blocks outlive their context in a small cache (at most 8 blocks), reused best-fit.
struct PinnedCache {
  struct Block { double* p; size_t bytes; };
  std::mutex m;
  std::vector<Block> blocks;
};

hipError_t pinned_acquire(size_t bytes, double** out, size_t* got) {
  {
    auto& pc = process_wide<PinnedCache>();
    std::lock_guard<std::mutex> lk(pc.m);
    auto& cache = pc.blocks;
    int best = -1;
    for (int i = 0; i < (int)cache.size(); ++i)
      if (cache[i].bytes >= bytes && (best < 0 || cache[i].bytes < cache[best].bytes)) best = i;
    if (best >= 0) {
      *out = cache[best].p;
      *got = cache[best].bytes;
      cache.erase(cache.begin() + best);
      return hipSuccess;
    }
  }
  *got = bytes;
  return hipHostMalloc((void**)out, bytes, hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable);
}

void pinned_release(double* p, size_t bytes) noexcept {
  try {
    auto& pc = process_wide<PinnedCache>();
    std::lock_guard<std::mutex> lk(pc.m);
    if (pc.blocks.size() < 8) { pc.blocks.push_back({p, bytes}); return; }
  } catch (const std::exception&) {
  }
  (void)hipHostFree(p);
}
}  // namespace

namespace {

// Every device buffer of a context is carved out of ONE slab (caller-provided, e.g. a torch tensor
// recycled by its caching allocator, or hipMalloc'ed once here).  Pass 0 (c->slab == nullptr) only
// measures; pass 1 places the buffers and uploads.
inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

template <class T>
int dalloc(plfem_ctx* c, T** dst, size_t count) {
  size_t bytes = align_up(std::max<size_t>(count, 1) * sizeof(T));
  if (c->slab) {
    if (c->slab_off + bytes > c->slab_bytes) { c->err = "workspace too small"; return PLFEM_EINVAL; }
    *dst = reinterpret_cast<T*>(c->slab + c->slab_off);
  }
  c->slab_off += bytes;
  return PLFEM_OK;
}

// Host arrays of a context go up in ONE copy from a pinned staging block: the uploads are placed first in the slab,
// upload() only records (slab offset, source, bytes), flush_uploads() fills the staging block (a few threads) and
// issues the copy.  22 separate copies from pageable memory were pinned and unpinned by the runtime one by one.
struct UploadItem { size_t off; const void* src; size_t bytes; };

template <class T, class A>
int upload(plfem_ctx* c, std::vector<UploadItem>& items, T** dst, const std::vector<T, A>& src) {
  const size_t off = c->slab_off;
  int rc = dalloc(c, dst, src.size());
  if (rc != PLFEM_OK) return rc;
  if (c->slab && !src.empty()) items.push_back({off, src.data(), src.size() * sizeof(T)});
  return PLFEM_OK;
}

// staging: pinned block of at least `span` bytes (the uploads occupy slab offsets [0, span)).  The block is filled and
// sent in a few pieces, so that the DMA of one piece runs while the host fills the next (filling 14 MB takes about as long
// as sending them: 0.28 + 0.25 ms in sequence at C1, round 3); the filling runs on a worker pool of the host analysis
// (parked threads from the process-wide cache: no thread creation here).
int flush_uploads(plfem_ctx* c, const std::vector<UploadItem>& items, size_t span, char* staging, size_t mesh_items) {
  size_t total = 0;
  for (const auto& it : items) total += it.bytes;
  const int nthreads = total > (4u << 20) ? 8 : 1;
  const int npieces = total > (2u << 20) ? 4 : 1;
  // pieces = runs of consecutive items (they are in slab order) of about total / npieces bytes
  // (the first piece = the mesh-level arrays, sent on the context's stream; the others follow on the copy stream)
  std::vector<size_t> first(1, 0);
  if (mesh_items > 0 && mesh_items < items.size()) first.push_back(mesh_items);
  {
    size_t acc = 0, rest = 0;
    for (size_t q = first.back(); q < items.size(); ++q) rest += items[q].bytes;
    const size_t q0 = first.back(), base = first.size();
    for (size_t q = q0; q < items.size(); ++q) {
      if ((int)first.size() < npieces && acc >= rest * (first.size() - base + 1) / (npieces - base + 1) && q > first.back()) first.push_back(q);
      acc += items[q].bytes;
    }
    first.push_back(items.size());
  }
  const bool split = c->copy_stream != nullptr && mesh_items > 0 && mesh_items < items.size();
  // the helpers run through the pieces on their own; the calling thread (rank 0) sends a piece as soon as every thread
  // has filled its share of it.  A share = a contiguous byte range of the piece (items are cut where a range ends).
  const size_t npc = first.size() - 1;
  std::unique_ptr<std::atomic<int>[]> done(new std::atomic<int>[npc]);
  for (size_t pc = 0; pc < npc; ++pc) done[pc].store(0, std::memory_order_relaxed);
  hipError_t herr = hipSuccess;
  plfem::host_parallel(nthreads, [&](int t, int nt) {
    for (size_t pc = 0; pc < npc; ++pc) {
      size_t bytes = 0;
      for (size_t q = first[pc]; q < first[pc + 1]; ++q) bytes += items[q].bytes;
      const size_t lo = bytes * t / nt, hi = bytes * (t + 1) / nt;      // this thread's byte range of the piece
      size_t pos = 0;
      for (size_t q = first[pc]; q < first[pc + 1] && pos < hi; ++q) {
        const size_t b0 = std::max(lo, pos), b1 = std::min(hi, pos + items[q].bytes);
        if (b0 < b1) std::memcpy(staging + items[q].off + (b0 - pos), (const char*)items[q].src + (b0 - pos), b1 - b0);
        pos += items[q].bytes;
      }
      done[pc].fetch_add(1, std::memory_order_release);
      if (t != 0) continue;
      for (int spins = 0; done[pc].load(std::memory_order_acquire) < nt; ++spins) plfem::cpu_relax(spins);
      const size_t q0 = first[pc], q1 = first[pc + 1];
      if (q0 == q1 || herr != hipSuccess) continue;
      const size_t plo = items[q0].off, phi = q1 < items.size() ? items[q1].off : span;
      herr = hipMemcpyAsync(c->slab + plo, staging + plo, phi - plo, hipMemcpyHostToDevice, (split && pc > 0) ? c->copy_stream : c->stream);
    }
  });
  if (herr == hipSuccess && split) {
    herr = hipEventRecord(c->ev_upload, c->copy_stream);
    c->upload_pending = true;              // (plfem_factor, the first reader of the front-level arrays, waits for it)
  }
  if (herr != hipSuccess) {
    c->err = std::string("hipMemcpyAsync (index upload): ") + hipGetErrorString(herr);
    return PLFEM_EHIP;
  }
  return PLFEM_OK;
}

void free_all(plfem_ctx* c) {
  if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);   // (the tail of the index upload reads the staging block)
  if (c->own_slab && c->slab) (void)hipFree(c->slab);
  plfem::free_index_map(c->map);
  if (c->h_pinned) pinned_release(c->h_pinned, c->h_pinned_bytes);
  if (c->h_staging) {
    (void)hipStreamSynchronize(c->stream);              // (the upload out of the block has long completed)
    pinned_release(c->h_staging, c->h_staging_bytes);
  }
  // (the stream has been synchronised by plfem_destroy: none of these events is pending)
  for (auto& pr : c->ev)
    for (auto& e : pr) ctx_event_release(c->device, EV_TIMING, e);
  for (auto& e : c->ev_step) ctx_event_release(c->device, EV_NO_TIMING, e);
  process_wide<EventPool>().give_all(c->device, EV_PROFILE, c->prof_ev);
  if (c->copy_stream) {
    (void)hipStreamSynchronize(c->copy_stream);
    process_wide<StreamPool>().give(c->device, 0, c->copy_stream, SIZE_MAX);
    c->copy_stream = nullptr;
  }
  ctx_event_release(c->device, EV_NO_TIMING, c->ev_copy);
  ctx_event_release(c->device, EV_NO_TIMING, c->ev_upload);
}

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// What place_buffers leaves for flush_uploads: the recorded host arrays, the slab bytes they span, how many of them are
// mesh-level
struct Placement {
  std::vector<UploadItem> items;
  size_t upload_span = 0, mesh_items = 0;
};

// One pass over every device buffer of the context, in slab order (see dalloc: measuring or placing)
int place_buffers(plfem_ctx* c, int max_ncv, Placement& pl) {
  const Symbolic& S = *c->S;
  const plfem::LaunchPlan& P = *c->plan;
  auto& items = pl.items;
  c->slab_off = 0;
  items.clear();
  // mesh-level arrays first: all that the CSR pattern kernel and the assembly read.  They go up on the context's stream,
  // the front-level arrays behind them on the copy stream, so that pattern and assembly run beside the rest of the upload
  TRY(upload(c, items, &c->d_edof, S.edof));
  c->d_tsorted = c->d_edof;          // rows 0-2 of the element DOF table ARE the column-sorted vertex table
  TRY(upload(c, items, &c->d_rowptr, S.rowptr));
  TRY(upload(c, items, &c->d_nptr, S.nptr));
  TRY(upload(c, items, &c->d_nadj, S.nadj));
  TRY(upload(c, items, &c->d_nloc, S.nloc));
  TRY(upload(c, items, &c->d_interior, S.interior));
  TRY(upload(c, items, &c->d_bmask, S.bmask));
  TRY(upload(c, items, &c->d_doflocs, S.doflocs));
  pl.mesh_items = items.size();
  TRY(upload(c, items, &c->d_blk, P.jobs));
  TRY(upload(c, items, reinterpret_cast<plfem::Tile**>(&c->d_tiles), P.tiles));   // (Tile has int2's layout)
  TRY(upload(c, items, &c->d_forder, P.forder));
  TRY(upload(c, items, &c->d_frec, P.frec));
  TRY(upload(c, items, &c->d_fs2, P.fs2));
  TRY(upload(c, items, &c->d_fm, P.fm));
  TRY(upload(c, items, &c->d_fnode_ptr, S.fnode_ptr));
  TRY(upload(c, items, &c->d_foff, S.foff));
  TRY(upload(c, items, &c->d_soff, S.soff));
  TRY(upload(c, items, &c->d_fnodes, S.fnodes));
  TRY(upload(c, items, &c->d_cinv0, S.cinv0));
  TRY(upload(c, items, &c->d_cinv1, S.cinv1));
  TRY(upload(c, items, &c->d_epos, S.epos));
  TRY(upload(c, items, &c->d_leaf_elem_ptr, S.leaf_elem_ptr));
  TRY(upload(c, items, &c->d_leaf_elems, S.leaf_elems));
  TRY(upload(c, items, &c->d_npos, S.npos));
  TRY(upload(c, items, &c->d_prow, S.prow));
  pl.upload_span = c->slab_off;
  TRY(dalloc(c, &c->d_colind, (size_t)c->nnz));      // filled on the device by launch_pattern_fill below
  TRY(dalloc(c, &c->d_slot_row, (size_t)c->nnz));
  TRY(dalloc(c, &c->d_cores, plfem::MAX_CORES * 3));
  TRY(dalloc(c, &c->d_elem, (size_t)S.ne * plfem::ELEM_STRIDE));
  for (auto& p : c->d_vals) TRY(dalloc(c, &p, (size_t)c->nnz));
  TRY(dalloc(c, &c->d_front, (size_t)S.foff[S.nfronts]));
  c->arena_doubles = (S.arena_doubles + 31) & ~(int64_t)31;
  const int64_t fnodes_total = c->fnodes_total = S.fnode_ptr[S.nfronts];
  TRY(dalloc(c, &c->d_fvec, (size_t)2 * fnodes_total * plfem::BLOCK_P));
  // What only the factorisation needs (Schur arenas, panels) and what only the Lanczos drivers need (the bases V, B V and
  // their restart copies) are never alive at the same time -- a context factorises, then iterates, on one stream -- and
  // share one region of the workspace.
  const size_t union_start = c->slab_off;
  TRY(dalloc(c, &c->d_schur, (size_t)2 * c->arena_doubles));
  // (panels of the largest tree level, one level at a time; three thirds: block steps kb mod 3)
  TRY(dalloc(c, &c->d_wbuf, (size_t)6 * P.level_nodes_max * plfem::NB));
  TRY(dalloc(c, &c->d_rbuf, (size_t)6 * P.level_nodes_max * plfem::NB));
  const size_t factor_end = c->slab_off;
  const size_t n2 = (size_t)c->n2, nc1 = (size_t)plfem::basis_cols(max_ncv), ncp = (size_t)plfem::proj_cols(max_ncv);
  c->slab_off = union_start;
  TRY(dalloc(c, &c->d_V, n2 * nc1));
  TRY(dalloc(c, &c->d_BV, n2 * nc1));
  TRY(dalloc(c, &c->d_V2, n2 * nc1));
  TRY(dalloc(c, &c->d_BV2, n2 * nc1));
  c->slab_off = std::max(c->slab_off, factor_end);
  TRY(dalloc(c, &c->d_dinv, (size_t)2 * S.nfronts * plfem::NB * plfem::NB));   // X of the pivot blocks, by block-step parity
  TRY(dalloc(c, &c->d_delta, (size_t)4 * fnodes_total));   // D^-1: (diagonal, off-diagonal) per front row
  TRY(dalloc(c, &c->d_fvec2, (size_t)2 * fnodes_total * plfem::BLOCK_P));
  TRY(dalloc(c, &c->d_u0, (size_t)2 * fnodes_total * plfem::BLOCK_P));
  TRY(dalloc(c, &c->d_u1, (size_t)2 * fnodes_total * plfem::BLOCK_P));
  TRY(dalloc(c, &c->d_xl, (size_t)2 * fnodes_total * plfem::BLOCK_P));
  TRY(dalloc(c, &c->d_counters, 4));
  TRY(dalloc(c, &c->d_w, n2 * plfem::BLOCK_P));
  TRY(dalloc(c, &c->d_bw, n2 * plfem::BLOCK_P));
  TRY(dalloc(c, &c->d_hblk, ncp * plfem::BLOCK_P));
  TRY(dalloc(c, &c->d_G, 64));
  TRY(dalloc(c, &c->d_Rinv, 64));
  TRY(dalloc(c, &c->d_t1, n2 * plfem::BLOCK_P));
  TRY(dalloc(c, &c->d_t2, n2 * plfem::BLOCK_P));
  TRY(dalloc(c, &c->d_h, ncp));
  TRY(dalloc(c, &c->d_hacc, ncp));
  // three users, one after the other on the context's stream: a panel dot, the Gram partials of the fused block B product,
  // the fused first pass
  c->partial_doubles = std::max({plfem::panel_dot_partial_doubles(c->n2, (int)ncp), plfem::gram_partial_doubles(S.N),
                                 plfem::first_pass_partial_doubles(c->n2)});
  TRY(dalloc(c, &c->d_partial, c->partial_doubles));
  TRY(dalloc(c, &c->d_scal, 16));
  TRY(dalloc(c, &c->d_S, nc1 * nc1));
  TRY(dalloc(c, &c->d_Hcols, (nc1 + 1) * (nc1 + 1)));
  TRY(dalloc(c, &c->d_coremask, (size_t)S.N));
  // two halves of post_doubles each: the post-processing, and the residual check in flight beside it
  c->post_doubles = std::max(plfem::post_sum_doubles(S.N, (int)nc1), plfem::resid_sum_doubles(S.N, (int)nc1)) + 16;
  TRY(dalloc(c, &c->d_post, 2 * c->post_doubles));
  TRY(dalloc(c, &c->d_layers, (size_t)plfem::MAX_LAYERS * plfem::LAYER_DOUBLES));   // (last: no other buffer moves)
  return PLFEM_OK;
}

int create_impl(plfem_ctx* c, const plfem_symbolic* sym, int device, void* stream, int max_ncv, void* workspace,
                int64_t workspace_bytes, bool size_only) {
  const Symbolic& S = sym->S;
  c->S = &S;
  c->device = device;
  c->stream = (hipStream_t)stream;   // NULL = the device's default (null) stream
  if (!size_only) {
    HIP_TRY(c, hipSetDevice(device));
    for (auto& pr : c->ev)
      for (auto& e : pr) HIP_TRY(c, ctx_event_acquire(device, EV_TIMING, &e));
    for (auto& e : c->ev_step) HIP_TRY(c, ctx_event_acquire(device, EV_NO_TIMING, &e));
    HIP_TRY(c, ctx_event_acquire(device, EV_NO_TIMING, &c->ev_upload));
    HIP_TRY(c, copy_stream_acquire(device, &c->copy_stream));
    HIP_TRY(c, phase_begin(c, plfem::PH_UPLOAD));
  }
  c->nv = S.nv; c->ne = S.ne; c->N = S.N; c->nnz = S.rowptr.empty() ? 0 : (int)S.rowptr[S.N]; c->nsolve = S.nsolve;
  c->L = S.L; c->nfronts = S.nfronts; c->dpn = S.dpn; c->sh = S.dpn - 1; c->n2 = S.dpn * (int64_t)S.N; c->max_ncv = max_ncv;
  // The launch plan (kernel forms by level, launch order, workgroup lists) depends on the mesh only: it is part of the
  // analysis (plan.cpp, built at the end of build_symbolic); every context on that analysis reads and uploads the same one.
  if (!S.plan.built) { c->err = "plfem_create: the analysis carries no launch plan"; return PLFEM_ESTATE; }
  c->plan = &S.plan;
  // The solve sweeps stage one front's right-hand sides in LDS (sweep_lds, device.h).  Beyond the device limit the launch
  // would fail as an opaque "invalid argument" much later, so decide here: P = BLOCK_P, else P = 1, else a clear error.
  if (!size_only) {
    int lim = 0;
    HIP_TRY(c, hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
    const int worst = c->plan->worst_m;
    if (plfem::sweep_lds(plfem::BLOCK_P, worst) <= (size_t)lim) c->max_block_p = plfem::BLOCK_P;
    else if (plfem::sweep_lds(1, worst) <= (size_t)lim) c->max_block_p = 1;
    else {
      c->err = "plfem_create: largest front has " + std::to_string(worst) + " DOFs; the solve sweeps stage 8 (m + 1) bytes of it in LDS, "
               "which exceeds this device's " + std::to_string(lim) + " bytes per workgroup (use a smaller leaf size / a coarser mesh)";
      return PLFEM_EINVAL;
    }
  }
  const bool ctx_trace = getenv("PLFEM_CTX_TRACE") != nullptr;
  const double tt1 = now_ms();
  Placement pl;
  TRY(place_buffers(c, max_ncv, pl));   // pass 0: measure
  const size_t need = c->slab_off;
  c->workspace_need = (int64_t)need;
  if (size_only) return PLFEM_OK;
  if (workspace) {
    if (workspace_bytes < (int64_t)need) { c->err = "plfem_create: workspace smaller than plfem_workspace_bytes"; return PLFEM_EINVAL; }
    if ((uintptr_t)workspace & 255) { c->err = "plfem_create: workspace must be 256-byte aligned"; return PLFEM_EINVAL; }
    c->slab = reinterpret_cast<char*>(workspace);
  } else {
    HIP_TRY(c, hipMalloc((void**)&c->slab, need));
    c->own_slab = true;
  }
  c->slab_bytes = need;
  const double tt2 = now_ms();
  TRY(place_buffers(c, max_ncv, pl));   // pass 1: place, then one staged upload
  double* staging = nullptr;
  size_t staging_bytes = 0;
  HIP_TRY(c, pinned_acquire(pl.upload_span, &staging, &staging_bytes));
  c->h_staging = staging;               // owned by the context from here on: released with it (free_all), so that
  c->h_staging_bytes = staging_bytes;   // creation does not have to wait for the copy
  TRY(flush_uploads(c, pl.items, pl.upload_span, reinterpret_cast<char*>(staging), pl.mesh_items));
  const double tt3 = now_ms();
  HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, 4 * sizeof(int32_t), c->stream));
  // the padding rows of the front-ordered right-hand side are never written and are multiplied by exact zeros of the
  // factors: they must be finite (the workspace may hold anything)
  HIP_TRY(c, hipMemsetAsync(c->d_fvec, 0, sizeof(double) * 2 * c->fnodes_total * plfem::BLOCK_P, c->stream));
  plfem::launch_pattern_fill(c);
  TRY(check_launch(c, "pattern fill"));
  {
    const size_t nc1p = (size_t)max_ncv + 2 + plfem::BLOCK_P;
    // the regions of device.h (plfem::PIN_*): the projected matrix (nc1p^2) last, then the two block-step slots
    HIP_TRY(c, pinned_acquire(sizeof(double) * (plfem::PIN_PROJ + nc1p * nc1p + 2 * nc1p * plfem::BLOCK_P), &c->h_pinned, &c->h_pinned_bytes));
    c->h_slots = c->h_pinned + plfem::PIN_PROJ + nc1p * nc1p;
  }
  HIP_TRY(c, phase_end(c, plfem::PH_UPLOAD));
  const double tt4 = now_ms();
  // no synchronisation: the upload and the pattern kernel run on while the caller prepares the assembly (every
  // later use of the context is ordered behind them on the stream)
  if (ctx_trace) fprintf(stderr, "[ctx] size pass %.3f  upload pass %.3f  pinned+launch %.3f  sync %.3f ms\n", tt2 - tt1, tt3 - tt2, tt4 - tt3, now_ms() - tt4);
  return PLFEM_OK;
}

int upload_cores(plfem_ctx* c, const double* cores_host, int ncore) {
  if (ncore < 0 || ncore > plfem::MAX_CORES || (ncore > 0 && !cores_host)) {
    c->err = "ncore must be in [0, 64]";
    return PLFEM_EINVAL;
  }
  if (ncore > 0) {
    std::memcpy(c->h_pinned + plfem::PIN_CORES, cores_host, sizeof(double) * 3 * ncore);
    HIP_TRY(c, hipMemcpyAsync(c->d_cores, c->h_pinned + plfem::PIN_CORES, sizeof(double) * 3 * ncore, hipMemcpyHostToDevice, c->stream));
  }
  return PLFEM_OK;
}

}  // namespace

extern "C" int plfem_create(const plfem_symbolic* sym, int32_t device, void* hip_stream, int32_t max_ncv,
                            void* workspace_dev, int64_t workspace_bytes, plfem_ctx** out, char* err,
                            int32_t errlen) try {
  if (!out) return PLFEM_EINVAL;
  *out = nullptr;
  if (!sym) return write_err(err, errlen, "plfem_create: null symbolic handle", PLFEM_EINVAL);
  if (max_ncv < 3 || max_ncv > PLFEM_MAX_NCV)
    return write_err(err, errlen, "plfem_create: max_ncv must be in [3, " + std::to_string(PLFEM_MAX_NCV) + "]", PLFEM_EINVAL);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return write_err(err, errlen, "plfem_create: no HIP device available (this library has no CPU fallback)", PLFEM_EHIP);
  if (device < 0 || device >= ndev) return write_err(err, errlen, "plfem_create: device index out of range", PLFEM_EINVAL);
  struct FreeCtx {
    void operator()(plfem_ctx* c) const { free_all(c); delete c; }
  };
  std::unique_ptr<plfem_ctx, FreeCtx> c(new plfem_ctx());
  const int rc = create_impl(c.get(), sym, device, hip_stream, max_ncv, workspace_dev, workspace_bytes, false);
  if (rc != PLFEM_OK) return write_err(err, errlen, c->err, rc);
  *out = c.release();
  return PLFEM_OK;
} catch (...) { return host_failure(err, errlen); }

extern "C" int plfem_workspace_bytes(const plfem_symbolic* sym, int32_t max_ncv, int64_t* bytes) try {
  if (!sym || !bytes || max_ncv < 3 || max_ncv > PLFEM_MAX_NCV) return PLFEM_EINVAL;
  plfem_ctx tmp;
  int rc = create_impl(&tmp, sym, 0, nullptr, max_ncv, nullptr, 0, true);
  *bytes = tmp.workspace_need;
  return rc;
} catch (...) { return host_failure(nullptr, 0); }

extern "C" void plfem_destroy(plfem_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  free_all(ctx);
  delete ctx;
}

extern "C" const char* plfem_last_error(const plfem_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

extern "C" int plfem_synchronize(plfem_ctx* ctx) try {
  if (!ctx) return PLFEM_EINVAL;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return PLFEM_OK;
} catch (...) { return host_failure(ctx); }

namespace {
// the two assembly calls: cores up, the element matrices (`element_matrices`, the one launch that differs), CSR gather
template <class ElementMatrices>
int assemble(plfem_ctx* c, const double* cores_host, int ncore, double eps_core, double eps_clad, const char* what,
             ElementMatrices element_matrices) {
  // (with an index profile set -- layers, a map or both -- eps_core and eps_clad are not read)
  const bool profile = c->nlayer > 0 || c->map.set();
  if (!profile && (!(eps_core > 0) || !(eps_clad > 0))) { c->err = "permittivities must be positive"; return PLFEM_EINVAL; }
  if (profile && !(c->eps_bg > 0)) {
    c->err = std::string(what) + ": an index map is set without a background permittivity (plfem_set_index_profile(ctx, NULL, 0, eps_bg))";
    return PLFEM_EINVAL;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(upload_cores(c, cores_host, ncore));
  HIP_TRY(c, phase_begin(c, plfem::PH_ASSEMBLE));
  element_matrices();
  plfem::launch_csr_gather(c);
  HIP_TRY(c, phase_end(c, plfem::PH_ASSEMBLE));
  TRY(check_launch(c, what));
  c->assembled = true;
  c->factored = false;
  return PLFEM_OK;
}
}  // namespace

extern "C" int plfem_set_index_profile(plfem_ctx* c, const double* layers_host, int32_t nlayer, double eps_bg) try {
  if (!c) return PLFEM_EINVAL;
  // no layers: back to the step model of the assembly calls' own arguments -- or, under an index map, to the map alone
  // over eps_bg, which is kept for that if it is one (anything else is not an error here: nothing else reads it)
  if (nlayer == 0) {
    c->nlayer = 0;
    c->eps_bg = (std::isfinite(eps_bg) && eps_bg > 0.0) ? eps_bg : 0.0;
    return PLFEM_OK;
  }
  if (const char* bad = plfem::profile_table_error(layers_host, nlayer, eps_bg)) {
    c->err = std::string("plfem_set_index_profile: ") + bad;
    return PLFEM_EINVAL;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t bytes = sizeof(double) * plfem::LAYER_DOUBLES * nlayer;
  double* pin = c->h_pinned + plfem::PIN_LAYERS;
  // whatever was queued before may still read the old table, and the pinned block must be free for the next call:
  // the copy goes behind that work on the context's stream and is waited for
  std::memcpy(pin, layers_host, bytes);
  HIP_TRY(c, hipMemcpyAsync(c->d_layers, pin, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->nlayer = nlayer;
  c->eps_bg = eps_bg;
  return PLFEM_OK;
} catch (...) { return host_failure(c); }

extern "C" int plfem_set_index_map(plfem_ctx* c, const double* eps_host, int32_t nx, int32_t ny, double x0, double y0,
                                   double dx, double dy) try {
  if (!c) return PLFEM_EINVAL;
  return plfem::set_index_map(c, "plfem_set_index_map", eps_host, nx, ny, x0, y0, dx, dy);
} catch (...) { return host_failure(c); }

extern "C" int plfem_assemble_hfield(plfem_ctx* c, const double* cores_host, int32_t ncore, double eps_core,
                                     double eps_clad, double k0, double alpha_p) try {
  if (!c) return PLFEM_EINVAL;
  if (c->dpn != 2) { c->err = "plfem_assemble_hfield: the analysis of this context has one unknown per node (use plfem_assemble_scalar)"; return PLFEM_EINVAL; }
  return assemble(c, cores_host, ncore, eps_core, eps_clad, "assemble",
                  [&] { plfem::launch_element_matrices(c, ncore, eps_core, eps_clad, k0, alpha_p); });
} catch (...) { return host_failure(c); }

extern "C" int plfem_assemble_scalar(plfem_ctx* c, const double* cores_host, int32_t ncore, double eps_core,
                                     double eps_clad, double k0) try {
  if (!c) return PLFEM_EINVAL;
  if (c->dpn != 1) { c->err = "plfem_assemble_scalar: the analysis of this context has two unknowns per node (plfem_symbolic_create_ex(..., 1, 0, ...))"; return PLFEM_EINVAL; }
  return assemble(c, cores_host, ncore, eps_core, eps_clad, "assemble scalar",
                  [&] { plfem::launch_element_matrices_scalar(c, ncore, eps_core, eps_clad, k0); });
} catch (...) { return host_failure(c); }

// CMT coupling integrals: raw[i + j n] = E_i^T M_deps F_j, norms
extern "C" int plfem_cmt_coupling(plfem_ctx* c, int32_t n, const double* fields_i_dev, const double* fields_j_dev,
                                  const double* cores_host, int32_t ncore, double eps_core, double eps_clad,
                                  double* raw_host, double* pi_host, double* pj_host, double* eps_mean_host) try {
  if (!c || !fields_i_dev || !fields_j_dev || !raw_host || !pi_host || !pj_host || n < 1) return PLFEM_EINVAL;
  if (c->dpn != 1) { c->err = "plfem_cmt_coupling: needs a context with one unknown per node (scalar fields)"; return PLFEM_EINVAL; }
  if (n > c->max_ncv) { c->err = "plfem_cmt_coupling: more fields than the context's max_ncv"; return PLFEM_EINVAL; }
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(upload_cores(c, cores_host, ncore));
  // From here on the MINV slot holds M_deps, not the mass matrix of the eigenproblem: whatever way this function is left,
  // the context must ask for a new assembly before the next factorisation / solve / residual check.
  struct Invalidate {
    plfem_ctx* c;
    ~Invalidate() { c->assembled = false; c->factored = false; }
  } invalidate{c};
  const double mean = plfem::launch_delta_eps_mass(c, ncore, eps_core, eps_clad);
  c->assembled = true;                        // (launch_spmv below reads the MINV slot)
  const int64_t N = c->n2;
  const int ld = n;
  double* Hd = c->d_Hcols;                    // [n + 2][n]: columns of the raw matrix, then the two norm vectors
  for (int j = 0; j < n; ++j) {
    plfem::launch_spmv(c, 1, 1, fields_j_dev + (size_t)j * N, c->d_w, N);                     // y = M_deps F_j
    plfem::launch_panel_dot(c, 1, fields_i_dev, n, c->d_w, N, Hd + (size_t)j * ld, ld);           // column j: E_i^T y
  }
  for (int i = 0; i < n; ++i) {
    plfem::launch_dot(c, fields_i_dev + (size_t)i * N, fields_i_dev + (size_t)i * N, Hd + (size_t)n * ld + i);
    plfem::launch_dot(c, fields_j_dev + (size_t)i * N, fields_j_dev + (size_t)i * N, Hd + (size_t)(n + 1) * ld + i);
  }
  TRY(check_launch(c, "cmt coupling"));
  double* hs = c->h_pinned + plfem::PIN_PROJ;
  HIP_TRY(c, hipMemcpyAsync(hs, Hd, sizeof(double) * (size_t)(n + 2) * ld, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i) raw_host[i + (size_t)j * n] = hs[(size_t)j * ld + i];
  for (int i = 0; i < n; ++i) { pi_host[i] = hs[(size_t)n * ld + i]; pj_host[i] = hs[(size_t)(n + 1) * ld + i]; }
  if (eps_mean_host) *eps_mean_host = mean;
  return PLFEM_OK;
} catch (...) { return host_failure(c); }

extern "C" int plfem_block_values_dev(plfem_ctx* c, int32_t block, const double** values_dev) try {
  if (!c || !values_dev || block < 0 || block >= PLFEM_BLK_COUNT) return PLFEM_EINVAL;
  *values_dev = c->d_vals[block];
  return PLFEM_OK;
} catch (...) { return host_failure(c); }

extern "C" int plfem_block_values_host(plfem_ctx* c, int32_t block, double* values_host) try {
  if (!c || !values_host || block < 0 || block >= PLFEM_BLK_COUNT) return PLFEM_EINVAL;
  if (!c->assembled) { c->err = "plfem_block_values_host before plfem_assemble_hfield"; return PLFEM_ESTATE; }
  HIP_TRY(c, hipMemcpyAsync(values_host, c->d_vals[block], sizeof(double) * c->nnz, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PLFEM_OK;
} catch (...) { return host_failure(c); }

extern "C" int plfem_spmv(plfem_ctx* c, int32_t which, const double* x_dev, double* y_dev) try {
  if (!c || !x_dev || !y_dev || (which != 0 && which != 1)) return PLFEM_EINVAL;
  if (!c->assembled) { c->err = "plfem_spmv before plfem_assemble_hfield"; return PLFEM_ESTATE; }
  HIP_TRY(c, hipSetDevice(c->device));
  plfem::launch_spmv(c, which, 1, x_dev, y_dev, c->n2);
  return check_launch(c, "spmv");
} catch (...) { return host_failure(c); }

extern "C" int plfem_factor(plfem_ctx* c, double sigma) try {
  if (!c) return PLFEM_EINVAL;
  if (!c->assembled) { c->err = "plfem_factor before plfem_assemble_hfield"; return PLFEM_ESTATE; }
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(wait_for_upload(c));
  HIP_TRY(c, phase_begin(c, plfem::PH_FACTOR));
  HIP_TRY(c, hipMemsetAsync(c->d_fvec, 0, sizeof(double) * 2 * c->fnodes_total * plfem::BLOCK_P, c->stream));   // (see plfem_create)
  plfem::launch_factor(c, sigma);
  if (c->test_post_factor) c->test_post_factor(c);   // null unless the test-hook add-on library installed one (api_debug.hip)
  HIP_TRY(c, phase_end(c, plfem::PH_FACTOR));
  TRY(check_launch(c, "factor"));
  c->sigma = sigma;
  c->factored = true;
  return PLFEM_OK;
} catch (...) { return host_failure(c); }

extern "C" int plfem_solve(plfem_ctx* c, const double* rhs_dev, double* x_dev, int32_t refine_steps) try {
  if (!c || !rhs_dev || !x_dev || refine_steps < 0) return PLFEM_EINVAL;
  if (!c->factored) { c->err = "plfem_solve before plfem_factor"; return PLFEM_ESTATE; }
  HIP_TRY(c, hipSetDevice(c->device));
  // scratch: d_t1 / d_t2, not d_V2 -- after plfem_solve_modes that holds the vectors plfem_modes_dev hands out
  plfem::solve_refined(c, 1, rhs_dev, x_dev, c->n2, false, refine_steps, c->d_t1, c->d_t2, c->d_t2);
  return check_launch(c, "solve");
} catch (...) { return host_failure(c); }

// ------------------------------------------------------------------------------------------------
// thick-restart Lanczos, shift-invert, B inner product, shared by the block driver (P = BLOCK_P) and the single-vector
// one (P = 1).  A driver builds the basis (m columns, then the residual block) and fills the columns of T (upper triangle
// authoritative, ld = m + P; R_m = T[mm:mm+P, mm-P:mm] upper triangular, beta_m for P = 1); this is the rest.
// ------------------------------------------------------------------------------------------------
namespace {
struct ThickRestart {
  plfem_ctx* c;
  int P, k, ld;
  double tol;
  double* hH;                     // pinned staging of the rotation matrices (and the single-vector driver's d_Hcols mirror)
  std::vector<double> T, Tm, theta, Svec;
  std::vector<int> order;         // Ritz pairs by decreasing |theta|
  int nconv = 0, restarts = 0;
  double max_rel_res = 0.0;

  ThickRestart(plfem_ctx* c_, int P_, int k_, int m, double tol_)
      : c(c_), P(P_), k(k_), ld(m + P_), tol(tol_), hH(c_->h_pinned + plfem::PIN_PROJ), T((size_t)ld * ld, 0.0) {}

  void fill_tm(int mm) {
    Tm.assign((size_t)mm * mm, 0.0);     // symmetric mm x mm projected matrix from the upper triangle
    for (int j = 0; j < mm; ++j)
      for (int i = 0; i <= j; ++i) {
        const double v = T[(size_t)j * ld + i];
        Tm[(size_t)j * mm + i] = v;
        Tm[(size_t)i * mm + j] = v;
      }
  }
  // order the Ritz pairs (theta) and count the converged wanted ones.  Residual of pair `id`: || R_m s[mm-P:mm] ||;
  // last(id, b) = component mm - P + b of its eigenvector
  template <class Last>
  void count_converged(int mm, Last last) {
    order.resize(mm);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return std::fabs(theta[a]) > std::fabs(theta[b]); });
    nconv = 0;
    max_rel_res = 0.0;
    for (int q = 0; q < std::min(k, mm); ++q) {
      const int id = order[q];
      double res;
      if (P == 1) {
        res = std::fabs(T[(size_t)(mm - 1) * ld + mm] * last(id, 0));
      } else {
        double r2 = 0.0;
        for (int a = 0; a < P; ++a) {
          double v = 0.0;
          for (int b = a; b < P; ++b) v += T[(size_t)(mm - P + b) * ld + (mm + a)] * last(id, b);
          r2 += v * v;
        }
        res = std::sqrt(r2);
      }
      const double rel = res / std::max(std::fabs(theta[id]), 3.7e-11);
      max_rel_res = std::max(max_rel_res, rel);
      if (rel <= tol) ++nconv;
    }
  }
  void count_from_svec(int mm) { count_converged(mm, [&](int id, int b) { return Svec[(size_t)id * mm + (mm - P + b)]; }); }
  // dense Ritz decomposition of the first mm columns
  void ritz(int mm) {
    fill_tm(mm);
    plfem::sym_eig(mm, Tm, Svec, theta);
    count_from_svec(mm);
  }

  // thick restart of mm columns: keep the k wanted pairs plus some of the next ones (ARPACK: kev + min(nconv, np/2)),
  // followed by the residual block; pk = the columns kept.  The room left for two more blocks never costs a wanted pair:
  // at least min(k, mm - P) columns stay (ncv = k + 1 on the single-vector driver would otherwise keep k - 1 columns at
  // every restart and never converge; the block driver's dispatch has m >= k + 3 P, so its pk is unchanged)
  int restart(int mm, int& pk) {
    const int64_t n = c->n2;
    hipStream_t st = c->stream;
    pk = k + std::min(nconv, (mm - k) / 2);
    pk = std::max(pk, k + (mm - k) / 4);
    pk = std::min(pk, mm - 2 * P);
    pk = std::max(pk, std::min(k, mm - P));
    for (int q = 0; q < pk; ++q) std::memcpy(hH + (size_t)q * mm, &Svec[(size_t)order[q] * mm], sizeof(double) * mm);
    HIP_TRY(c, hipMemcpyAsync(c->d_S, hH, sizeof(double) * mm * pk, hipMemcpyHostToDevice, st));
    plfem::launch_rotate(c, c->d_V, mm, c->d_S, mm, pk, c->d_V2);
    plfem::launch_rotate(c, c->d_BV, mm, c->d_S, mm, pk, c->d_BV2);
    TRY(check_launch(c, "restart rotation"));
    HIP_TRY(c, hipMemcpyAsync(c->d_V2 + (size_t)pk * n, c->d_V + (size_t)mm * n, sizeof(double) * n * P, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_BV2 + (size_t)pk * n, c->d_BV + (size_t)mm * n, sizeof(double) * n * P, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipStreamSynchronize(st));   // (hH is reused by the next cycle)
    std::swap(c->d_V, c->d_V2);
    std::swap(c->d_BV, c->d_BV2);
    std::fill(T.begin(), T.end(), 0.0);
    for (int q = 0; q < pk; ++q) T[(size_t)q * ld + q] = theta[order[q]];
    HIP_TRY(c, hipMemsetAsync(c->d_Hcols, 0, sizeof(double) * ld * ld, st));
    ++restarts;
    return PLFEM_OK;
  }

  // the wanted Ritz pairs of mm columns, ascending lambda = sigma + 1/theta: values to evals_host, vectors rotated into
  // evecs_dev (nullptr: the context's own buffer, see lanczos_run); then the stats and the verdict
  int finish(int mm, double sigma, double* evals_host, double* evecs_dev, double* stats_host, int nop, int nblock) {
    hipStream_t st = c->stream;
    std::vector<int> want(order.begin(), order.begin() + k);
    std::vector<double> lam(mm);
    for (int i = 0; i < mm; ++i) lam[i] = sigma + 1.0 / theta[i];
    std::sort(want.begin(), want.end(), [&](int a, int b) { return lam[a] < lam[b]; });
    // Converged pairs are purified as ARPACK purifies them in shift-invert mode: x + V[:, mm:mm+P] (R_m s[mm-P:mm]) / theta
    // = OP x / theta, one step of inverse iteration at the cost of P more rows of the rotation.  The correction is of the
    // size of tol and B-orthogonal to the basis; it damps the components of x far from sigma, which the stopping test on OP
    // barely sees and which dominate the residual A x - lambda B x of the pencil (about 100 times smaller afterwards).
    // An unconverged call returns the plain Ritz vectors; so does an exhausted Krylov space (a zero on the diagonal of R_m),
    // whose residual block is no vector.
    bool purify = nconv >= k;
    for (int a = 0; a < P; ++a) purify = purify && T[(size_t)(mm - P + a) * ld + (mm + a)] > 0.0;
    const int rows = purify ? mm + P : mm;
    for (int q = 0; q < k; ++q) {
      const int id = want[q];
      evals_host[q] = lam[id];
      double* s = hH + (size_t)q * rows;
      std::memcpy(s, &Svec[(size_t)id * mm], sizeof(double) * mm);
      for (int a = 0; a < rows - mm; ++a) {
        double v = 0.0;
        for (int b = a; b < P; ++b) v += T[(size_t)(mm - P + b) * ld + (mm + a)] * Svec[(size_t)id * mm + (mm - P + b)];
        s[mm + a] = v / theta[id];
      }
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_S, hH, sizeof(double) * rows * k, hipMemcpyHostToDevice, st));
    if (!evecs_dev) evecs_dev = c->d_V2;            // (idle since the last restart, if any)
    c->modes_dev = evecs_dev;
    c->modes_k = k;
    plfem::launch_rotate(c, c->d_V, rows, c->d_S, rows, k, evecs_dev);
    HIP_TRY(c, phase_end(c, plfem::PH_LANCZOS));
    TRY(check_launch(c, "ritz rotation"));
    if (!c->defer_sync) HIP_TRY(c, hipStreamSynchronize(st));   // (plfem_solve_modes: its one synchronisation comes later)
    if (stats_host) {
      const double s[5] = {(double)nconv, (double)nop, (double)restarts, max_rel_res, (double)nblock};
      std::copy(s, s + 5, stats_host);
    }
    if (nconv < k) { c->err = "Lanczos: no convergence within maxiter restarts"; return PLFEM_ENOCONV; }
    return PLFEM_OK;
  }
};
}  // namespace

// ------------------------------------------------------------------------------------------------
// block thick-restart Lanczos (BLOCK_P vectors per step): every pass over the factors of the
// shift-invert operator serves BLOCK_P right-hand sides.
// ------------------------------------------------------------------------------------------------
static int lanczos_block(plfem_ctx* c, int k, int ncv, double tol, int maxiter, double sigma, double* evals_host,
                         double* evecs_dev, double* stats_host) {
  constexpr int P = plfem::BLOCK_P;
  const int64_t n = c->n2;
  hipStream_t st = c->stream;
  HIP_TRY(c, phase_begin(c, plfem::PH_LANCZOS));
  int m = ((ncv + P - 1) / P) * P;                                 // basis columns before the residual block
  if (m > c->max_ncv) m = (c->max_ncv / P) * P;
  ThickRestart R(c, P, k, m, tol);
  const int ld = R.ld;
  int nop = 0, nblock = 0;
  {
    plfem::launch_start_field(c, P, c->d_V2);       // fixed pseudo-random interior block, generated on the device
    plfem::launch_spmv(c, 1, P, c->d_V2, c->d_bw, n);
    plfem::launch_solve(c, P, c->d_bw, c->d_w, n);    // (start block: any vector will do, no refinement)
    nop += P; ++nblock;
    plfem::launch_spmv(c, 1, P, c->d_w, c->d_bw, n);
    plfem::launch_panel_dot(c, P, c->d_w, P, c->d_bw, n, c->d_G, P);
    plfem::launch_chol_block(c, c->d_G, P, c->d_hblk, P, c->d_Rinv);      // R itself is not needed for the start block
    plfem::launch_block_scale(c, c->d_w, c->d_bw, n, c->d_Rinv, c->d_V, c->d_BV, n, nullptr, 0, nullptr, nullptr, c->d_fvec);
  }
  HIP_TRY(c, hipMemsetAsync(c->d_Hcols, 0, sizeof(double) * ld * ld, st));
  int c0 = 0, mm = 0;
  // One block step = one pass over the factors for P vectors + CGS2 + CholQR, all asynchronous.  The
  // P new columns of the projected matrix and the rank flag follow it into a pinned slot, then an event.
  int32_t* hcnt = reinterpret_cast<int32_t*>(c->h_pinned + plfem::PIN_COUNTERS);
  double* slots_dev = nullptr;                   // device view of the pinned slots and counters
  int32_t* hcnt_dev = nullptr;
  HIP_TRY(c, hipHostGetDevicePointer((void**)&slots_dev, c->h_slots, 0));
  HIP_TRY(c, hipHostGetDevicePointer((void**)&hcnt_dev, hcnt, 0));
  // Orthogonalisation: in exact arithmetic OP V_j only has components along V_j and V_{j-1}, so the first
  // Gram-Schmidt pass runs over those two blocks (where the cancellation is) and the second over the whole basis
  // (full reorthogonalisation of what rounding left, no cancellation any more).  The first step after a thick
  // restart couples with every kept Ritz vector: both passes full.
  int cycle_start = -1;                          // first column of the current cycle when it follows a restart
  int il_ready = 0;                              // basis column whose B V block d_fvec holds in front order (k_block_scale)
  auto launch_step = [&](int c0_, int slot) -> int {
    const int nc = c0_ + P;
    const int lo = (c0_ == cycle_start) ? 0 : std::max(0, nc - 2 * P);
    double* Hblk = c->d_Hcols + (size_t)c0_ * ld;                             // T[0:nc, c0:c0+P] (zero before the step)
    if (c->refine_steps == 0 && nc - lo <= plfem::FIRST_COLS) {
      // W = OP V_j left in front order by the sweeps; the first pass permutes it on the way (two launches instead of four)
      plfem::launch_solve(c, P, c->d_BV + (size_t)c0_ * n, nullptr, n, il_ready == c0_);
      plfem::launch_first_pass_block(c, c->d_BV + (size_t)lo * n, c->d_V + (size_t)lo * n, nc - lo, c->d_w, n, Hblk + lo, ld);
    } else {
      // W = OP V_j; scratch: the first 3 P columns of d_V2 (the restart double buffer, idle between restarts)
      plfem::solve_refined(c, P, c->d_BV + (size_t)c0_ * n, c->d_w, n, il_ready == c0_, c->refine_steps, c->d_V2,
                           c->d_V2 + (size_t)P * n, c->d_V2 + (size_t)2 * P * n);
      plfem::launch_panel_dot(c, P, c->d_BV + (size_t)lo * n, nc - lo, c->d_w, n, Hblk + lo, ld);
      plfem::launch_panel_axpy(c, P, c->d_V + (size_t)lo * n, nc - lo, Hblk + lo, ld, c->d_w, n);
    }
    plfem::launch_panel_dot(c, P, c->d_BV, nc, c->d_w, n, c->d_hblk, ld, Hblk, ld);  // second pass, T += h2
    // (the second pass also leaves the block interleaved in d_t1 -- idle in this driver -- for the SpMV's gathers)
    plfem::launch_panel_axpy(c, P, c->d_V, nc, c->d_hblk, ld, c->d_w, n, c->d_t1);
    {
      const int pid = plfem::prof_open(c, PLFEM_PROF_SPMV_B, 12.0 * c->nnz + 4.0 * (c->N + 1) + 2.0 * 8.0 * P * (double)n);
      // (the B product also leaves the chunk partials of the Gram matrix W^T B W: no panel-dot launch for the CholQR)
      const int nparts = plfem::launch_spmv_b_block_il(c, c->d_t1, c->d_bw, n, c->d_partial);
      plfem::prof_close(c, pid);
      plfem::launch_chol_from_partials(c, nparts, Hblk + nc, ld, c->d_Rinv);          // W^T B W = R^T R, R -> T[nc:nc+P, c0:c0+P]
    }
    // the last kernel of the step also stores the new columns and the counters into the pinned slot (no copies)
    plfem::launch_block_scale(c, c->d_w, c->d_bw, n, c->d_Rinv, c->d_V + (size_t)nc * n, c->d_BV + (size_t)nc * n, n,
                              Hblk, ld * P, slots_dev + (size_t)slot * ld * P, hcnt_dev + 4 * slot, c->d_fvec);
    il_ready = nc;
    int rc = check_launch(c, "block lanczos step");
    if (rc != PLFEM_OK) return rc;
    HIP_TRY(c, hipEventRecord(c->ev_step[slot], st));
    return PLFEM_OK;
  };
  // wait for the step in `slot` and copy its columns [c0_, c0_ + P) into the host copy of T
  auto absorb_step = [&](int c0_, int slot) -> int {
    HIP_TRY(c, hipEventSynchronize(c->ev_step[slot]));
    if (hcnt[4 * slot + 2] != 0) { c->err = "block Lanczos: rank-deficient block (Krylov space exhausted)"; return PLFEM_ESINGULAR; }
    const double* src = c->h_slots + (size_t)slot * ld * P;
    for (int j = 0; j < P; ++j)
      for (int i = 0; i < ld; ++i) {
        const double v = src[(size_t)j * ld + i];
        if (!std::isfinite(v)) { c->err = "block Lanczos breakdown: non-finite projected matrix"; return PLFEM_ESINGULAR; }
        R.T[(size_t)(c0_ + j) * ld + i] = v;
      }
    return PLFEM_OK;
  };
  std::vector<double> Ylast;
  // convergence test only: Ritz values + last block of every Ritz vector (no eigenvector matrix)
  auto quick_check = [&](int mm_) {
    R.fill_tm(mm_);
    plfem::sym_eig_last_rows(mm_, P, R.Tm, Ylast, R.theta);
    R.count_converged(mm_, [&](int id, int b) { return Ylast[(size_t)id * P + b]; });
  };
  // Ritz decomposition (theta, Svec, order) for the final rotation, or (need_all) for a restart.  Before the first
  // restart the projected matrix is block tridiagonal (half bandwidth P; what full reorthogonalisation leaves outside
  // the band is rounding) and the final rotation only needs the k wanted vectors: band path of host_eig.h, Svec
  // then holds the rows of order[0 .. k) only.
  auto full_check = [&](int mm_, bool need_all) {
    if (R.restarts > 0 || need_all) {
      R.ritz(mm_);
      return;
    }
    R.fill_tm(mm_);
    plfem::sym_band_eigenvalues(mm_, P, R.Tm.data(), mm_, R.theta);
    std::vector<int> ids(mm_);
    std::iota(ids.begin(), ids.end(), 0);
    std::sort(ids.begin(), ids.end(), [&](int a, int b) { return std::fabs(R.theta[a]) > std::fabs(R.theta[b]); });
    ids.resize(std::min(k, mm_));
    R.Svec.resize((size_t)mm_ * mm_);
    plfem::sym_band_eigenvectors(mm_, P, R.Tm.data(), mm_, R.theta, ids, R.Svec.data(), mm_);
    R.count_from_svec(mm_);
  };
  // Pipeline: while the GPU runs block step j + 1, the host tests convergence on the projected matrix of
  // step j; the extra step in flight when the test succeeds is simply not used.  The largest residual of the
  // wanted pairs decays geometrically (x 0.15-0.25 per block step), so when the last two tests predict that the
  // pending step converges, step j + 1 is held back until its test is in: a correct prediction saves the wasted
  // step, a wrong one idles the GPU for one host test.
  double res_prev = 0.0, res_last = 0.0;         // largest relative residual at the last two tests (0 = none yet)
  while (true) {
    int pend_c0 = -1, pend_slot = 0, slot = 0;
    bool converged = false, inflight = false, force_launch = false, have_full = false;
    mm = c0;
    while (true) {
      const bool predicted = !force_launch && pend_c0 >= 0 && res_prev > 0.0 && res_last > 0.0 &&
                             res_last * (res_last / res_prev) <= tol;
      force_launch = false;
      int new_c0 = -1, new_slot = 0;
      if (c0 + P <= m && !predicted) {
        TRY(launch_step(c0, slot));
        nop += P; ++nblock;
        new_c0 = c0; new_slot = slot;
        c0 += P; slot ^= 1;
      }
      if (pend_c0 >= 0) {
        TRY(absorb_step(pend_c0, pend_slot));
        mm = pend_c0 + P;
        if (mm >= k + P && (new_c0 >= 0 || predicted)) {     // (the last step of a cycle gets the full test below)
          // a held step is expected to converge: go straight to the full decomposition the rotation needs
          if (predicted) { full_check(mm, false); have_full = true; } else { quick_check(mm); have_full = false; }
          res_prev = res_last;
          res_last = R.max_rel_res;
          if (getenv("PLFEM_LANCZOS_TRACE"))
            fprintf(stderr, "[lanczos] cols %d nconv %d max_rel_res %.3e%s\n", mm, R.nconv, R.max_rel_res, predicted ? " (held)" : "");
          if (R.nconv >= k) { converged = true; inflight = new_c0 >= 0; break; }
        }
        if (predicted) {                            // not converged after all: resume with the step that was held
          pend_c0 = -1;
          force_launch = true;
          if (c0 + P <= m) continue;
          break;
        }
      }
      pend_c0 = new_c0; pend_slot = new_slot;
      if (pend_c0 < 0) break;                       // basis full and every step absorbed
    }
    if (converged) {
      if (!have_full) full_check(mm, false);
      if (R.nconv < k) {                            // the two eigensolvers disagree at the threshold: resume
        converged = false;
        if (inflight) { TRY(absorb_step(c0 - P, slot ^ 1)); }
        res_prev = res_last = 0.0;
        if (c0 + P <= m) continue;
        mm = c0;
        full_check(mm, true);
      }
    } else {
      mm = c0;
      full_check(mm, true);
    }
    res_prev = res_last = 0.0;                      // a restart changes the decay
    if (R.nconv >= k || R.restarts >= maxiter) break;
    int pk = 0;
    TRY(R.restart(mm, pk));
    c0 = pk;
    cycle_start = pk;
    il_ready = -1;
  }
  return R.finish(mm, sigma, evals_host, evecs_dev, stats_host, nop, nblock);
}

// evecs_dev == nullptr: the vectors go into the context's own buffer (the idle restart double buffer d_V2; see
// plfem_solve_modes / plfem_modes_dev)
// The single-vector driver does not resolve eigenvalues closer together than its tolerance: a one-vector Krylov space holds
// one direction of such a cluster, so the call can converge on a set that misses copies and holds pairs further from sigma
// in their place (ARPACK shares this limit).  The block driver finds up to BLOCK_P copies.
static int lanczos_run(plfem_ctx* c, int32_t k, int32_t ncv, double tol, int32_t maxiter,
                       double sigma, double* evals_host, double* evecs_dev, double* stats_host) {
  if (!c || !evals_host) return PLFEM_EINVAL;
  if (!c->factored || c->sigma != sigma) { c->err = "plfem_lanczos_shift_invert: call plfem_factor(sigma) first"; return PLFEM_ESTATE; }
  const int64_t n = c->n2;
  if (k < 1 || ncv <= k || ncv > c->max_ncv || ncv > c->dpn * c->nsolve) { c->err = "need 1 <= k < ncv <= max_ncv"; return PLFEM_EINVAL; }
  if (tol <= 0) tol = 2.2e-16;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemsetAsync(c->d_counters + 2, 0, sizeof(int32_t), c->stream));
  // large problems: block Lanczos (BLOCK_P right-hand sides per pass over the factors); tiny ones
  // (Krylov space of dimension ~n) keep the single-vector recurrence
  {
    const char* env = std::getenv("PLFEM_LANCZOS_BLOCK");
    const bool allow = !(env && env[0] == '0');
    int mblk = ((ncv + plfem::BLOCK_P - 1) / plfem::BLOCK_P) * plfem::BLOCK_P;
    if (mblk > c->max_ncv) mblk = (c->max_ncv / plfem::BLOCK_P) * plfem::BLOCK_P;   // round down instead
    if (allow && c->max_block_p >= plfem::BLOCK_P && k >= plfem::BLOCK_P && mblk >= k + 3 * plfem::BLOCK_P &&
        c->dpn * (int64_t)c->nsolve >= 16 * (int64_t)(mblk + plfem::BLOCK_P))
      return lanczos_block(c, k, ncv, tol, maxiter, sigma, evals_host, evecs_dev, stats_host);
  }
  hipStream_t st = c->stream;
  HIP_TRY(c, phase_begin(c, plfem::PH_LANCZOS));
  const int m = ncv;
  ThickRestart R(c, 1, k, m, tol);
  const int ld = R.ld;
  double* hH = R.hH;                              // pinned mirror of d_Hcols
  int nop = 0;

  // start vector: fixed pseudo-random interior field pushed through OP once (as ARPACK does for mode 3)
  {
    plfem::launch_start_field(c, 1, c->d_t1);
    plfem::launch_spmv(c, 1, 1, c->d_t1, c->d_bw, n);
    plfem::launch_solve(c, 1, c->d_bw, c->d_w, n);
    ++nop;
    plfem::launch_spmv(c, 1, 1, c->d_w, c->d_bw, n);
    plfem::launch_dot(c, c->d_w, c->d_bw, c->d_scal);
    plfem::launch_scale_store(c, c->d_w, c->d_bw, c->d_scal, c->d_V, c->d_BV, nullptr);
  }
  HIP_TRY(c, hipMemsetAsync(c->d_Hcols, 0, sizeof(double) * ld * ld, st));

  int j0 = 0;        // first Lanczos column to compute in this cycle
  while (true) {
    for (int j = j0; j < m; ++j) {
      double* Vj1 = c->d_V + (size_t)(j + 1) * n;
      double* BVj1 = c->d_BV + (size_t)(j + 1) * n;
      plfem::solve_refined(c, 1, c->d_BV + (size_t)j * n, c->d_w, n, false, c->refine_steps, c->d_t1, c->d_t2,
                           c->d_t2);                                      // w = OP v_j = K^-1 B v_j
      ++nop;
      double* hcol = c->d_Hcols + (size_t)j * ld;
      plfem::launch_panel_dot(c, 1, c->d_BV, j + 1, c->d_w, n, hcol, ld);                 // h = V^T B w
      plfem::launch_panel_axpy(c, 1, c->d_V, j + 1, hcol, ld, c->d_w, n);
      plfem::launch_panel_dot(c, 1, c->d_BV, j + 1, c->d_w, n, c->d_h, ld, hcol, ld);     // CGS2 second pass, T += h2
      plfem::launch_panel_axpy(c, 1, c->d_V, j + 1, c->d_h, ld, c->d_w, n);
      plfem::launch_spmv(c, 1, 1, c->d_w, c->d_bw, n);
      plfem::launch_dot(c, c->d_w, c->d_bw, c->d_scal);
      plfem::launch_scale_store(c, c->d_w, c->d_bw, c->d_scal, Vj1, BVj1, hcol + (j + 1));
    }
    TRY(check_launch(c, "lanczos step"));
    HIP_TRY(c, hipMemcpyAsync(hH, c->d_Hcols, sizeof(double) * ld * ld, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    for (int j = j0; j < m; ++j)
      for (int i = 0; i <= j + 1 && i < ld; ++i) R.T[(size_t)j * ld + i] = hH[(size_t)j * ld + i];
    const double beta_m = R.T[(size_t)(m - 1) * ld + m];
    if (!std::isfinite(beta_m)) { c->err = "Lanczos breakdown: non-finite residual norm (is sigma an eigenvalue?)"; return PLFEM_ESINGULAR; }
    R.ritz(m);
    if (R.nconv >= k || R.restarts >= maxiter) break;
    TRY(R.restart(m, j0));
  }
  return R.finish(m, sigma, evals_host, evecs_dev, stats_host, nop, 0);
}

extern "C" int plfem_lanczos_shift_invert(plfem_ctx* c, int32_t k, int32_t ncv, double tol, int32_t maxiter,
                                          double sigma, double* evals_host, double* evecs_dev, double* stats_host) try {
  if (!c || !evals_host || !evecs_dev) return PLFEM_EINVAL;
  return lanczos_run(c, k, ncv, tol, maxiter, sigma, evals_host, evecs_dev, stats_host);
} catch (...) { return host_failure(c); }

extern "C" int plfem_postprocess(plfem_ctx* c, int32_t k, double* evecs_dev, const double* cores_host, int32_t ncore,
                                 double* out_host, double* frac_core_host, double* modes_int_dev) try {
  if (!c || !evecs_dev || !out_host || k < 1 || k > c->max_ncv) return PLFEM_EINVAL;
  if (!c->assembled) { c->err = "plfem_postprocess before plfem_assemble_hfield"; return PLFEM_ESTATE; }
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(upload_cores(c, cores_host, ncore));
  HIP_TRY(c, phase_begin(c, plfem::PH_POST));
  plfem::launch_post(c, k, evecs_dev, ncore, out_host, frac_core_host, modes_int_dev);
  HIP_TRY(c, phase_end(c, plfem::PH_POST));
  TRY(check_launch(c, "postprocess"));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PLFEM_OK;
} catch (...) { return host_failure(c); }

// ------------------------------------------------------------------------------------------------
// One call for the whole numeric solve (include/plfem.h): assembly, factorisation, eigen-solve, post-processing, the
// a-posteriori check (with its refined second pass) and the copy of the interior mode vectors to the host, enqueued back
// to back.  Behind the Lanczos run (which synchronises with its own step events) the host waits ONCE.
// ------------------------------------------------------------------------------------------------
extern "C" int plfem_solve_modes(plfem_ctx* c, const double* cores_host, int32_t ncore, double eps_core, double eps_clad,
                                 double k0, double alpha_p, double sigma, int32_t k, int32_t ncv, double tol,
                                 int32_t maxiter, double residual_tol, double tol_refined, double* evals_host,
                                 double* post_host, double* frac_core_host, double* resid_host, double* modes_int_host,
                                 double* stats_host) try {
  if (!c || !evals_host || !post_host || !resid_host) return PLFEM_EINVAL;
  if (k < 1 || k > c->max_ncv) { c->err = "plfem_solve_modes: need 1 <= k <= max_ncv"; return PLFEM_EINVAL; }
  const double th0 = now_ms();
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->copy_stream) HIP_TRY(c, copy_stream_acquire(c->device, &c->copy_stream));
  if (!c->ev_copy) HIP_TRY(c, ctx_event_acquire(c->device, EV_NO_TIMING, &c->ev_copy));
  // Whatever way the call is left: the Lanczos drivers leave their final synchronisation to this call, the mode copies
  // queued on the copy stream land before the caller may release modes_int_host (the explicit synchronisations below
  // clear copy_pending, so that the success path makes no extra call), and the trace events go back.
  struct Defer {
    plfem_ctx* c;
    int saved_refine;
    bool copy_pending = false;
    hipEvent_t tr_ev[3] = {nullptr, nullptr, nullptr};
    ~Defer() {
      if (copy_pending) (void)hipStreamSynchronize(c->copy_stream);
      for (hipEvent_t e : tr_ev) if (e) (void)hipEventDestroy(e);
      c->defer_sync = false;
      c->refine_steps = saved_refine;
    }
  } defer{c, c->refine_steps};
  c->defer_sync = true;
  // PLFEM_CALL_TRACE=1 (tuning aid): where the wall time of this call goes beyond its device phases -- host timestamps of the
  // enqueue points, the stream's backlog at entry (work of plfem_create still queued) and the tail of the mode copy
  static const bool call_trace = getenv("PLFEM_CALL_TRACE") != nullptr;
  auto& tr_ev = defer.tr_ev;
  double th_asm = 0, th_fac = 0, th_lan = 0, th_enq = 0, th_sync = 0;
  if (call_trace) {
    for (auto& e : tr_ev) (void)hipEventCreate(&e);
    (void)hipEventRecord(tr_ev[0], c->stream);
  }
  if (c->dpn == 2) TRY(plfem_assemble_hfield(c, cores_host, ncore, eps_core, eps_clad, k0, alpha_p));
  else TRY(plfem_assemble_scalar(c, cores_host, ncore, eps_core, eps_clad, k0));
  th_asm = now_ms();
  TRY(plfem_factor(c, sigma));
  th_fac = now_ms();
  double st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double first_res = 0.0, res = 0.0;
  int perturbed = 0, refined = 0;
  double n_opinv = 0, n_block = 0, restarts = 0;
  // the one writer of stats_host: entries [lo, hi) (PLFEM_SOLVE_*) as they stand at the exit
  auto put_stats = [&](int lo, int hi) {
    if (!stats_host) return;
    double v[PLFEM_SOLVE_STATS] = {st[0], n_opinv, restarts, st[3], n_block, first_res, res, (double)refined, (double)perturbed};
    if (hi > PLFEM_SOLVE_T_ASSEMBLE_US) {
      for (int ph = 0; ph < plfem::PH_COUNT; ++ph) v[PLFEM_SOLVE_T_ASSEMBLE_US + ph] = phase_us(c, (plfem::Phase)ph);
      v[PLFEM_SOLVE_T_CALL_US] = (now_ms() - th0) * 1e3;
    }
    for (int q = lo; q < hi; ++q) stats_host[q] = v[q];
  };
  for (int pass = 0; pass < 2; ++pass) {
    // second pass: refinement inside the operator (repairs an inaccurate factor) AND a tighter Ritz tolerance (repairs a
    // first pass that merely stopped too early: a residual above the bound with no perturbed pivot)
    c->refine_steps = pass == 0 ? defer.saved_refine : std::max(1, defer.saved_refine + 1);
    const double tol_p = pass == 0 ? tol : std::min(tol, tol_refined);
    const int rc = lanczos_run(c, k, ncv, tol_p, maxiter, sigma, evals_host, nullptr, st);
    n_opinv += st[1]; n_block += st[4]; restarts += st[2];
    if (rc != PLFEM_OK) {
      (void)hipStreamSynchronize(c->stream);       // (PLFEM_ENOCONV: evals_host / plfem_modes_dev hold the current Ritz pairs)
      put_stats(0, PLFEM_SOLVE_RESIDUAL_FIRST);
      return rc;
    }
    th_lan = now_ms();
    double* modes = c->modes_dev;
    double* modes_int = c->d_BV2 != modes ? c->d_BV2 : c->d_BV;   // (a restart swaps the double buffers: take the idle one)
    HIP_TRY(c, phase_begin(c, plfem::PH_POST));
    // The copy of the mode vectors (~30 MB at C1: 0.58 ms on the host link, the longest item behind the Lanczos run) leaves
    // on its own stream, group of modes by group of modes as their post-processing completes, while the later groups and
    // the check below occupy this stream.
    hipError_t copy_err = hipSuccess;
    const size_t row_bytes = sizeof(double) * (size_t)c->dpn * c->nsolve;
    const std::function<void(int, int)> send_group = [&](int g0, int kg) {
      if (copy_err != hipSuccess) return;
      defer.copy_pending = true;
      copy_err = hipEventRecord(c->ev_copy, c->stream);
      if (copy_err == hipSuccess) copy_err = hipStreamWaitEvent(c->copy_stream, c->ev_copy, 0);
      if (copy_err == hipSuccess)
        copy_err = hipMemcpyAsync(reinterpret_cast<char*>(modes_int_host) + g0 * row_bytes, reinterpret_cast<char*>(modes_int) + g0 * row_bytes,
                                  kg * row_bytes, hipMemcpyDeviceToHost, c->copy_stream);
    };
    plfem::post_enqueue(c, k, modes, ncore, modes_int_host ? modes_int : nullptr, modes_int_host ? &send_group : nullptr);
    HIP_TRY(c, phase_end(c, plfem::PH_POST));
    HIP_TRY(c, copy_err);
    HIP_TRY(c, phase_begin(c, plfem::PH_RESIDUAL));
    plfem::resid_enqueue(c, k, evals_host, modes);
    HIP_TRY(c, phase_end(c, plfem::PH_RESIDUAL));
    TRY(check_launch(c, "post-processing + residual check"));
    if (call_trace) {
      (void)hipEventRecord(tr_ev[1], c->stream);
      (void)hipEventRecord(tr_ev[2], c->copy_stream);
    }
    th_enq = now_ms();
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // THE synchronisation of the call
    th_sync = now_ms();
    plfem::post_finish(c, k, post_host, frac_core_host);
    plfem::resid_finish(c, k, resid_host);
    perturbed = reinterpret_cast<const int32_t*>(c->h_pinned + plfem::PIN_COUNTERS)[0];
    res = 0.0;
    for (int i = 0; i < k; ++i) res = (resid_host[i] > res || !(resid_host[i] == resid_host[i])) ? resid_host[i] : res;
    if (pass == 0) first_res = res;
    if (res <= residual_tol && perturbed == 0) break;
    if (modes_int_host) HIP_TRY(c, hipStreamSynchronize(c->copy_stream));   // (the vectors on their way: let them land, then redo)
    defer.copy_pending = false;
    if (pass == 1) {
      if (res <= residual_tol) break;              // (perturbed pivots, repaired by the refinement)
      char msg[512];
      std::snprintf(msg, sizeof(msg), "eigen-residual %.2e after the refined re-run (first pass %.2e, bound %.0e); %s", res, first_res,
                    residual_tol, perturbed > 0 ? "vanishing pivots were perturbed: the shift-invert factorisation is inaccurate on this mesh"
                                                : "no pivot was perturbed: the eigenpairs did not converge tightly enough");
      c->err = msg;
      put_stats(PLFEM_SOLVE_RESIDUAL_FIRST, PLFEM_SOLVE_T_ASSEMBLE_US);
      return PLFEM_ERESIDUAL;
    }
    refined = 1;
  }
  if (modes_int_host) HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
  defer.copy_pending = false;
  if (call_trace) {
    const double th_end = now_ms();
    float backlog = 0, total = 0, copy_tail = 0;
    (void)hipEventElapsedTime(&backlog, tr_ev[0], c->ev[plfem::PH_ASSEMBLE][0]);      // entry -> first assembly kernel may start
    (void)hipEventElapsedTime(&total, tr_ev[0], tr_ev[1]);
    (void)hipEventElapsedTime(&copy_tail, tr_ev[1], tr_ev[2]);        // end of the residual check -> end of the mode copy
    fprintf(stderr, "[call] host: assemble enqueued +%.3f, factor +%.3f, lanczos returned +%.3f, post + check enqueued +%.3f, stream done +%.3f, "
                    "copy done +%.3f ms | device: entry -> assembly %.3f (backlog of plfem_create + launch), entry -> end of check %.3f, "
                    "check -> copy end %.3f ms\n",
            th_asm - th0, th_fac - th0, th_lan - th0, th_enq - th0, th_sync - th0, th_end - th0, backlog, total, copy_tail);
  }
  put_stats(0, PLFEM_SOLVE_STATS);
  return PLFEM_OK;
} catch (...) { return host_failure(c); }

extern "C" int plfem_modes_dev(plfem_ctx* c, const double** evecs_dev, int32_t* k) try {
  if (!c || !evecs_dev) return PLFEM_EINVAL;
  if (!c->modes_dev) { c->err = "plfem_modes_dev: no eigen-solve has run on this context"; return PLFEM_ESTATE; }
  *evecs_dev = c->modes_dev;
  if (k) *k = c->modes_k;
  return PLFEM_OK;
} catch (...) { return host_failure(c); }

extern "C" int plfem_timings(plfem_ctx* c, double* out_host) try {
  if (!c || !out_host) return PLFEM_EINVAL;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  int32_t cnt[4] = {0, 0, 0, 0};
  HIP_TRY(c, hipMemcpy(cnt, c->d_counters, sizeof(cnt), hipMemcpyDeviceToHost));
  // slots 0-4: assemble, factor, lanczos, post, upload (us); 5: pivot perturbations; 6: residual check (us); 7: 0
  for (int ph = plfem::PH_ASSEMBLE; ph <= plfem::PH_UPLOAD; ++ph) out_host[ph] = phase_us(c, (plfem::Phase)ph);
  out_host[5] = cnt[0];
  out_host[6] = phase_us(c, plfem::PH_RESIDUAL);
  out_host[7] = 0.0;
  return PLFEM_OK;
} catch (...) { return host_failure(c); }

// ---- live kernel timing for bench.py's roofline object -------------------------------------------
extern "C" int plfem_profile_begin(plfem_ctx* c, int32_t max_ranges) try {
  if (!c || max_ranges < 1) return PLFEM_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  c->prof_max = max_ranges;                          // event pairs are created on demand at the launch site
  if (c->prof_ev.empty()) process_wide<EventPool>().take_all(c->device, EV_PROFILE, c->prof_ev);
  c->prof_n = 0;
  c->prof_toggle = 0;
  c->prof_slot.clear();
  c->prof_rbytes.clear();
  c->prof_on = true;
  return PLFEM_OK;
} catch (...) { return host_failure(c); }

extern "C" int plfem_profile_end(plfem_ctx* c, double* out_host) try {
  if (!c || !out_host) return PLFEM_EINVAL;
  c->prof_on = false;
  for (int q = 0; q < 3 * PLFEM_PROF_COUNT; ++q) out_host[q] = 0.0;
  hipError_t e = hipSetDevice(c->device);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  for (int q = 0; q < c->prof_n && e == hipSuccess; ++q) {
    float ms = 0;
    e = hipEventElapsedTime(&ms, c->prof_ev[2 * q], c->prof_ev[2 * q + 1]);
    double* o = out_host + 3 * c->prof_slot[q];
    o[0] += 1.0;
    o[1] += ms * 1e3;
    o[2] += c->prof_rbytes[q];
  }
  process_wide<EventPool>().give_all(c->device, EV_PROFILE, c->prof_ev);   // (on the error path too)
  if (e != hipSuccess) {
    c->err = std::string("plfem_profile_end: ") + hipGetErrorString(e);
    return PLFEM_EHIP;
  }
  return PLFEM_OK;
} catch (...) { return host_failure(c); }

// ---- a-posteriori residuals, options ---------------------------------------------------------------
extern "C" int plfem_residuals(plfem_ctx* c, int32_t k, const double* evals_host, const double* evecs_dev, double* out_host) try {
  if (!c || !evals_host || !evecs_dev || !out_host || k < 1 || k > c->max_ncv) return PLFEM_EINVAL;
  if (!c->assembled) { c->err = "plfem_residuals before plfem_assemble_hfield"; return PLFEM_ESTATE; }
  HIP_TRY(c, hipSetDevice(c->device));
  plfem::launch_residuals(c, k, evals_host, evecs_dev, out_host);
  return check_launch(c, "residuals");
} catch (...) { return host_failure(c); }

extern "C" int plfem_set_option(plfem_ctx* c, const char* name, double value) try {
  if (!c || !name) return PLFEM_EINVAL;
  const std::string n(name);
  if (n == "refine_steps") {
    if (value < 0 || value > 8) { c->err = "refine_steps must be in [0, 8]"; return PLFEM_EINVAL; }
    c->refine_steps = (int)value;
  } else {
    c->err = "plfem_set_option: unknown option '" + n + "'";
    return PLFEM_EINVAL;
  }
  return PLFEM_OK;
} catch (...) { return host_failure(c); }
