// C-ABI of libspecpride_hip.so (include/specpride.h): argument checks,
// workspace carving and kernel launches.  One translation unit (the kernel
// sources are included) so the whole engine is a single gfx950 code object.
//
// Every entry point only enqueues work, on the caller's stream and (bin-mean,
// gap-average, medoid: SideFork) on the device's side stream, forked from the
// caller's and joined back to it: no workspace allocation, no synchronisation
// (hipGraph-capturable).  The global state is the error text (thread-local), the
// opt-in profile accumulators (g_prof, under g_prof_mu) and one side stream
// with three events per device (g_side, under g_side_mu, created on first use).
//
// Layout of this file: shared helpers, then per method its workspace layout (one
// carve_* function serves the size query and the launch) and its launch chain,
// all in one anonymous namespace; the extern "C" entry points follow.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/specpride.h"

// Earlier rounds' A/B switches were folded into the source at their kept settings
// (round 6), and the diagnostic variants whose results were wrong by design were
// deleted: git history and profiles/r0*_ab_* keep the record.  A build that still asks
// for one of them fails here instead of silently producing something else.
#if defined(SPX_DG_NOMZ) || defined(SPX_DG_NOBAR) || defined(SPX_DG_P3LANE) || defined(SPX_DG_NOMIRROR) || \
    defined(SPX_GR_DIAG) || defined(SPX_QF_DIAG) || defined(SPX_BR_FOLD) || defined(SPX_BF_RING) ||       \
    defined(SPX_BF_REVERSE)
#error "diagnostic / rejected variants are not part of libspecpride_hip (see git history)"
#endif
#if defined(SPX_GA_FLAT4) || defined(SPX_GA_FLAT6) || defined(SPX_GA_HASH) || defined(SPX_GA_HASH2) ||     \
    defined(SPX_GA_HASH3) || defined(SPX_GA_NOFILT) || defined(SPX_GA_TPERM) || defined(SPX_GA_GBATCH) ||  \
    defined(SPX_GA_HYBRID) || defined(SPX_GA_P3INT) || defined(SPX_GA_BSKIP) || defined(SPX_GA_P2B) ||     \
    defined(SPX_GA_EARLY) || defined(SPX_GA_DEFERBIG) || defined(SPX_MD_MFMA) || defined(SPX_MD_P5L) ||    \
    defined(SPX_MD_RECIP) || defined(SPX_MD_R32) || defined(SPX_MD_MBC) || defined(SPX_MD_L1RUNS) ||       \
    defined(SPX_MD_SWZ) || defined(SPX_MD_P6W) || defined(SPX_MD_P1B) || defined(SPX_MD_FILL_LDS) ||       \
    defined(SPX_MD_FILL_FLAT) || defined(SPX_MD_LEAF_W) || defined(SPX_MD_LEAF_B) || defined(SPX_GR_FP4) ||\
    defined(SPX_GR_TR) || defined(SPX_WALK_R)
#error "this A/B switch was folded into the source at its kept setting in round 6 (see git history)"
#endif
#include "best_score.hip"
#include "bin_mean.hip"
#include "bin_mean_seg.hip"
#include "bin_mean_q.hip"

#include "bin_mean_split.hip"
#include "bin_mean_wide.hip"
#include "binned_cosine.hip"
#include "by_fraction.hip"
#include "cosine_medoid.hip"
#include "gap_average.hip"
#include "medoid.hip"
#include "mgf_format.hip"
#include "mgf_parse.hip"
#include "mgf_splice.hpp"
#include "fused.hip"
#include "transfer.hip"
#include "wire.hip"

#ifndef SPX_MD_GRIDY
#define SPX_MD_GRIDY 128u  // deferred clusters the large path's grid-stride passes take at a time (32: configs[3] medoid 3.02 ms, 128: 2.92, 512: 2.92)
#endif
#ifndef SPX_GR_GRID
#define SPX_GR_GRID 8192  // medoid_gram_reg_kernel workgroups (4 waves each, grid-stride over the flat tile list;
                          // 2048: 3.20 ms configs[3] medoid, 8192: 3.05-3.11, 16384: 3.06-3.08)
#endif

namespace {

// ---------------------------------------------------------------- shared helpers
thread_local char g_err[256] = "";

int fail(int code, const char* msg) {
  std::snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    std::snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return SPX_EHIP;
  }
  return SPX_SUCCESS;
}

// one kernel launch on stream s and its error check (`name` goes into the error text);
// SPX_LAUNCH(kernel, grid, block, s, args...) names the kernel it launches
template <class... Params, class... Args>
int launch(const char* name, void (*kernel)(Params...), dim3 grid, dim3 block, hipStream_t s, Args&&... args) {
  hipLaunchKernelGGL(kernel, grid, block, 0, s, std::forward<Args>(args)...);
  return check_launch(name);
}
#define SPX_LAUNCH(kernel, ...) launch(#kernel, spx::kernel, __VA_ARGS__)

spx::CsrView view(const spx_csr* c) {
  return spx::CsrView{c->n_clusters, c->n_spectra, c->n_peaks, c->cluster_off, c->spec_off,
                      c->mz,         c->inten,     c->prec_mz, c->charge,      c->rt};
}

bool csr_ok(const spx_csr* c) {
  return c && c->n_clusters >= 0 && c->n_spectra >= 0 && c->n_peaks >= 0 && c->cluster_off && c->spec_off &&
         (c->n_peaks == 0 || (c->mz && c->inten)) && (c->n_spectra == 0 || (c->prec_mz && c->charge));
}

size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

// carving helper: takes `count` T (256-aligned) from the workspace.  On a null base it only
// measures: every size query carves the layout its launch carves.
struct Carver {
  char* base;
  size_t used;
  template <class T>
  T* take(size_t count) {
    T* p = reinterpret_cast<T*>(base + used);
    used += align256(count * sizeof(T));
    return p;
  }
};

// ------------------------------------------- per-kernel launch timing (opt-in)
// bench.py's rooflines need the dominant kernel's own duration, not the entry
// point's (which also launches its leftover chain).  When enabled
// (spx_profile_enable), the launches below are bracketed by HIP events on the
// caller's stream; spx_profile_read syncs on them and sums.  Off by default: the
// launch path then records nothing and never synchronises.
enum ProfSlot { kProfBinMeanReg, kProfMedoidReg, kProfMedoidGram, kProfGapLds, kProfGapWide, kProfBinMeanMedoid,
                kProfN };
constexpr const char* kProfNames[kProfN] = {"bin_mean_reg_kernel",     "medoid_reg_kernel",
                                            "medoid_gram_kernel",      "gap_average_lds_kernel",
                                            "gap_average_wide_kernel", "bin_mean_medoid_kernel"};
struct ProfAcc {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  std::vector<int64_t> calls;  // per pending pair: the call it belongs to
  double ms = 0.0;
  int64_t launches = 0, last_call = -1;
};
std::atomic<int64_t> g_prof_calls{0};
std::atomic<bool> g_prof_on{false};
std::mutex g_prof_mu;
ProfAcc g_prof[kProfN];

int prof_index(const char* name) {
  for (int i = 0; i < kProfN; ++i)
    if (std::strcmp(kProfNames[i], name) == 0) return i;
  return -1;
}
// events of one launch: begin() before it, end() after it (no-ops when off)
struct ProfScope {
  int idx = -1;
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t s = nullptr;
  int64_t call = -1;
  // `call` >= 0: scopes of one call sharing it count as ONE launch (spx_medoid's two large
  // paths, one per stream: the Gram time of the call is their sum)
  ProfScope(ProfSlot i, hipStream_t st, int64_t call_id = -1) : s(st), call(call_id) {
    if (!g_prof_on.load(std::memory_order_relaxed)) return;
    if (call < 0) call = g_prof_calls.fetch_add(1);
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    if (hipEventRecord(a, s) != hipSuccess) return;
    idx = i;
  }
  void end() {
    if (idx < 0) return;
    if (hipEventRecord(b, s) == hipSuccess) {
      std::lock_guard<std::mutex> lock(g_prof_mu);
      g_prof[idx].pending.emplace_back(a, b);
      g_prof[idx].calls.push_back(call);
    }
    idx = -1;
  }
};

// launch() inside `prof` (opened by the caller, on the same stream, as the first argument)
template <class... Params, class... Args>
int launch_timed(ProfScope prof, const char* name, void (*kernel)(Params...), dim3 grid, dim3 block, hipStream_t s,
                 Args&&... args) {
  hipLaunchKernelGGL(kernel, grid, block, 0, s, std::forward<Args>(args)...);
  prof.end();
  return check_launch(name);
}
#define SPX_LAUNCH_TIMED(prof, kernel, ...) launch_timed(prof, #kernel, spx::kernel, __VA_ARGS__)

// ------------------------------------------------------------ the side stream
// A second stream per device, for a call's work that can run BESIDE the kernels on the
// caller's stream (gap-average's giant pipeline next to its LDS and wide kernels).  The
// call forks it from the caller's stream with an event and joins it back before returning,
// so to the caller the call is one stream's worth of ordered work (hipGraph capture
// included).  The mutex covers one call's fork ... join enqueue, so the shared events pair up.
struct SideStream {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, mid = nullptr, join = nullptr;
};
std::mutex g_side_mu;
SideStream g_side[64];

// the current device's side stream (created on first use), or nullptr on a HIP error;
// call with g_side_mu held
SideStream* side_stream() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  SideStream& S = g_side[dev];
  if (!S.s) {
    // (a high-priority stream measured the same: profiles/r06_ga_intake.txt)
    if (hipStreamCreateWithFlags(&S.s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&S.fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&S.mid, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&S.join, hipEventDisableTiming) != hipSuccess)
      return nullptr;
  }
  return &S;
}

// One call's use of the side stream.  begin(s) takes the lock (held until the object dies:
// until the entry point returns) and forks the side stream from the caller's stream s; what
// the call then enqueues on stream() runs beside s.  mark_mid() / mark_join() record where
// the side stream stands, wait_mid(s) / wait_join(s) make s wait for that point.  A call that
// never begins touches neither the lock nor the stream.  Every step returns an SPX code;
// `who` (the entry point) goes into the error text.
class SideFork {
 public:
  explicit SideFork(const char* who) : who_(who), lock_(g_side_mu, std::defer_lock) {}
  int begin(hipStream_t s) {
    lock_.lock();
    side_ = side_stream();
    if (!side_) return err("side stream");
    return ok(hipEventRecord(side_->fork, s) == hipSuccess &&
                  hipStreamWaitEvent(side_->s, side_->fork, 0) == hipSuccess,
              "fork");
  }
  // everything below needs a begin() that returned SPX_SUCCESS: callers guard both with one flag
  hipStream_t stream() const { return side_->s; }
  int mark_mid() { return ok(hipEventRecord(side_->mid, side_->s) == hipSuccess, "mid event"); }
  int wait_mid(hipStream_t s) { return ok(hipStreamWaitEvent(s, side_->mid, 0) == hipSuccess, "mid wait"); }
  int mark_join() { return ok(hipEventRecord(side_->join, side_->s) == hipSuccess, "join event"); }
  int wait_join(hipStream_t s) { return ok(hipStreamWaitEvent(s, side_->join, 0) == hipSuccess, "join wait"); }

 private:
  int ok(bool done, const char* step) { return done ? (int)SPX_SUCCESS : err(step); }
  int err(const char* step) {
    char what[96];
    std::snprintf(what, sizeof(what), "%s %s", who_, step);
    if (int rc = check_launch(what)) return rc;
    return fail(SPX_EHIP, what);  // (a device past g_side: HIP itself reported nothing)
  }
  const char* who_;
  std::unique_lock<std::mutex> lock_;
  SideStream* side_ = nullptr;
};

// ------------------------------------------------------------ fallback grids
constexpr int kFallbackBlocks = 64;

int64_t fallback_grid(int64_t C) { return std::max<int64_t>(1, std::min<int64_t>(C, kFallbackBlocks)); }

// Grid of a global-scratch fallback kernel whose workgroups each own a slice of
// `slice_bytes`: as many as a 1 GiB scratch budget allows (>= 64, <= 4,096, <= C),
// so a batch whose clusters all defer (long spectra, many distinct bins) still
// fills the device.  Workspace sizing and the launch use the same value.
int64_t fallback_grid_sized(int64_t C, int64_t slice_bytes) {
  constexpr int64_t kBudget = int64_t(1) << 30;
  int64_t g = slice_bytes > 0 ? kBudget / slice_bytes : kFallbackBlocks;
  g = std::max<int64_t>(kFallbackBlocks, std::min<int64_t>(g, 4096));
  return std::max<int64_t>(1, std::min<int64_t>(C, g));
}

unsigned wire_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192)); }

// ------------------------------------------------------------------ bin-mean
int32_t bin_words(const spx_bin_params* p) {
  const double nb = std::trunc((p->maximum - p->minimum) / p->binsize) + 1.0;  // binning.py:172
  return (int32_t)((nb + 63.0) / 64.0);
}

int64_t bin_mean_fallback_grid(int64_t C, const spx_bin_params* params, int64_t dcap) {
  return fallback_grid_sized(C, spx::bin_mean_slice_bytes(bin_words(params), dcap));
}

// range records of the split path: every range holds >= SP_CAPW occupied bins
// except each cluster's last, so C + P / SP_CAPW bounds them (capped; clusters past
// the cap take the global kernel)
// SPX_SPLIT_RANGE_CAP (environment, tests only) lowers the cap so the overflow
// path -- clusters handed to the global kernel -- runs on small batches
int32_t split_range_cap(const spx_csr* csr) {
  int64_t r = csr->n_clusters + csr->n_peaks / spx::SP_CAPW + 1;
  if (const char* e = std::getenv("SPX_SPLIT_RANGE_CAP")) {
    const long v = std::strtol(e, nullptr, 10);
    if (v > 0) r = std::min<int64_t>(r, v);
  }
  return (int32_t)std::max<int64_t>(1, std::min<int64_t>(r, int64_t(1) << 20));
}

// Arena of the segmented fold (bin_mean_seg.hip): a cluster needs its bitmap and
// prefix (12 B per bin word), (blocks x slots) tables and 16 B per contribution;
// clusters that do not fit take the bin-range split path.  Bounded by the batch
// (64 B per peak) and by a fixed cap.
// SPX_SEG_ARENA (environment, tests only) caps it, so clusters overflow to the
// split path on small batches.
int64_t seg_arena_bytes(const spx_csr* csr, const spx_bin_params* params) {
  constexpr int64_t kCap = int64_t(2) << 30;
  const int64_t per_cluster = align256((size_t)bin_words(params) * 12) + 4096;
  int64_t b = 64 * csr->n_peaks + per_cluster * std::min<int64_t>(csr->n_clusters, 4096) + (int64_t(1) << 20);
  if (const char* e = std::getenv("SPX_SEG_ARENA")) {
    const long long v = std::strtoll(e, nullptr, 10);
    if (v >= 0) b = std::min<int64_t>(b, v);
  }
  return std::min(b, kCap);
}

// SPX_KEPT_FOLD=0 (environment, tests only) sends every cluster the wide kernel
// defers past the kept-bin fold, to the segmented fold
int kept_fold_enabled() {
  const char* e = std::getenv("SPX_KEPT_FOLD");
  return !(e && e[0] == '0');
}

// slots of BinMeanWs::counters (zeroed by the call's opening memset)
enum BmCounter {
  kBmcDeferred = 0,       // clusters past the wide kernel: the main chain's kept-bin fold list
  kBmcUnused = 1,         // the fused head's cluster queue (bin_mean_medoid_kernel); unused otherwise
  kBmcSplitClusters = 2,  // planned split clusters
  kBmcSplitRanges = 3,
  kBmcGlobal = 4,         // the global kernel's list
  kBmcSegTasks = 5,       // segmented-fold block tasks
  kBmcSegTiles = 6,       // its slot tiles
  kBmcSplitList = 7,      // the split path's list (clusters the segmented fold's arena could not hold)
  kBmcSegIn = 8,          // the segmented fold's list (what the kept-bin folds pass on)
  kBmcFoldTasks = 9,      // the main chain's kept-bin fold: block tasks,
  kBmcFoldTiles = 10,     // count tiles,
  kBmcFoldUnits = 11,     // fold units: long-chain,
  kBmcFoldUnitsOther = 12,  // and the others (the kernels read n_units[0..1])
  kBmcInDeferred = 16,    // the intake's kept-bin fold: its list,
  kBmcInTasks = 17,       // tasks,
  kBmcInTiles = 18,       // tiles,
  kBmcInUnits = 19,       // and units (two again)
  kBmcInUnitsOther = 20,
  kBmcSlots = 32
};
static_assert(kBmcFoldUnitsOther == kBmcFoldUnits + 1 && kBmcInUnitsOther == kBmcInUnits + 1, "n_units[0..1]");

// What one kept-bin fold (bin_mean_q.hip) works on: a list of clusters, a record each, and
// its task / tile / unit lists with their counters.
struct KeptFoldWs {
  int32_t *list, *n_list;
  spx::QMeta* meta;
  int32_t *task_cl, *tile_cl, *unit_cl;
  int32_t task_cap, tile_cap, unit_cap;
  int32_t *n_tasks, *n_tiles, *n_units;
};

struct BinMeanWs {
  int32_t *counters, *glist, *split_list, *task_cl, *tile_cl, *seg_in;
  size_t zeroed;  // bytes from `counters` the opening memset clears: the counters, bump and rest.counts
  // the main chain's kept-bin fold (what the wide kernel defers) and the intake's (clusters
  // past the wide kernel by size, on the side stream; empty when no cluster can be one)
  KeptFoldWs fold, fold_in;
  spx::StripedList rest;  // the register kernel's leftovers (striped appends)
  unsigned long long* bump;
  spx::SplitCluster* scl;
  spx::SplitRange* ranges;
  spx::SegMeta* meta;
  char *arena, *scratch;
  int64_t arena_bytes, n_task_cap, n_tile_cap;
  int32_t range_cap;
};

// A batch whose largest cluster has more than BM_NMAX spectra may hold clusters the
// intake takes (bin_mean_past_wide's other tests -- 2^28 peaks, a bin space past BM_WMAX
// words -- the chain after the wide kernel keeps, as before).
bool bin_mean_intake_possible(const spx_batch_info* info) {
  return info->max_cluster_spectra > spx::BM_NMAX;
}

// a kept-bin fold's records and lists (its cluster list is carved by the caller)
void carve_kept_fold(Carver& w, KeptFoldWs& K, size_t clusters, int32_t task_cap, int32_t tile_cap, int32_t unit_cap) {
  K.meta = w.take<spx::QMeta>(clusters);
  K.task_cap = task_cap;
  K.task_cl = w.take<int32_t>((size_t)task_cap);
  K.tile_cap = tile_cap;
  K.tile_cl = w.take<int32_t>((size_t)tile_cap);
  K.unit_cap = unit_cap;
  K.unit_cl = w.take<int32_t>((size_t)unit_cap);
}

// The workspace layout (the size query and the launch use the same carving).
BinMeanWs carve_bin_mean(Carver& w, const spx_csr* csr, const spx_bin_params* params, const spx_batch_info* info) {
  const size_t C = (size_t)std::max<int64_t>(csr->n_clusters, 1);
  const size_t begin = w.used;
  BinMeanWs W;
  W.counters = w.take<int32_t>(kBmcSlots);
  W.bump = w.take<unsigned long long>(1);
  // right after the counters and the bump pointer: one memset clears all three
  W.rest.counts = w.take<int32_t>((size_t)spx::kListStripes * spx::kListLine);
  W.zeroed = w.used - begin;
  W.rest.cap = spx::striped_cap((int64_t)C);
  W.rest.items = w.take<int32_t>((size_t)W.rest.cap * spx::kListStripes);
  W.fold.list = w.take<int32_t>(C);
  W.glist = w.take<int32_t>(C);
  W.split_list = w.take<int32_t>(C);
  W.scl = w.take<spx::SplitCluster>(C);
  W.range_cap = split_range_cap(csr);
  W.ranges = w.take<spx::SplitRange>((size_t)W.range_cap);
  W.meta = w.take<spx::SegMeta>(C);
  // the kept-bin fold: clusters the wide kernel defers have > 128 spectra or
  // > 4,096 peaks; tasks are blocks of >= 1 spectrum, units kept bins (each
  // holding >= 33 contributions: the quorum of n > 128, or one of 4,096+ peaks'
  // Q_KCAP-capped share)
  W.seg_in = w.take<int32_t>(C);
  const int64_t q_bound = std::min<int64_t>(csr->n_clusters, csr->n_spectra / 129 + csr->n_peaks / 4097 + 2);
  const int32_t task_cap = (int32_t)std::min<int64_t>(csr->n_spectra + 1, INT32_MAX);
  const int32_t tile_cap = (int32_t)std::min<int64_t>(q_bound * (spx::BM_WMAX / spx::Q_TILEW) + 1, INT32_MAX);
  const int32_t unit_cap = (int32_t)std::min<int64_t>(csr->n_peaks / 32 + q_bound + 1, INT32_MAX);
  carve_kept_fold(w, W.fold, C, task_cap, tile_cap, unit_cap);
  W.n_task_cap = csr->n_spectra / spx::SG_SB + csr->n_clusters + 1;
  W.task_cl = w.take<int32_t>((size_t)W.n_task_cap);
  W.n_tile_cap = csr->n_peaks / spx::SG_TILE + csr->n_clusters + 1;
  W.tile_cl = w.take<int32_t>((size_t)W.n_tile_cap);
  W.arena_bytes = seg_arena_bytes(csr, params);
  W.arena = w.take<char>((size_t)W.arena_bytes);
  const bool in = bin_mean_intake_possible(info);
  W.fold_in.list = w.take<int32_t>(in ? C : 1);
  carve_kept_fold(w, W.fold_in, in ? C : 1, in ? task_cap : 1, in ? tile_cap : 1, in ? unit_cap : 2);
  W.scratch = w.base + w.used;
  W.fold.n_list = W.counters + kBmcDeferred;
  W.fold.n_tasks = W.counters + kBmcFoldTasks;
  W.fold.n_tiles = W.counters + kBmcFoldTiles;
  W.fold.n_units = W.counters + kBmcFoldUnits;
  W.fold_in.n_list = W.counters + kBmcInDeferred;
  W.fold_in.n_tasks = W.counters + kBmcInTasks;
  W.fold_in.n_tiles = W.counters + kBmcInTiles;
  W.fold_in.n_units = W.counters + kBmcInUnits;
  return W;
}

// The launch that replaces the register kernel's (spx_bin_mean_medoid: the fused
// kernel), given the call's views; nullptr = bin_mean_reg_kernel itself.
struct BinMeanHead {
  // `queue`: a counter of the workspace that the opening memset zeroes (kBmcUnused)
  int (*launch)(void* ctx, const spx::CsrView& V, const spx::BinMeanParams& P, const spx::PeaksOut& O,
                double* prec_out, int32_t* charge_out, int32_t* status, const spx::StripedList& rest, int32_t* queue,
                hipStream_t s);
  void* ctx;
};

// argument and workspace checks of spx_bin_mean (also run up front by the fused entry point)
int bin_mean_validate(const spx_csr* csr, const spx_bin_params* params, const spx_batch_info* info,
                      const spx_peaks_out* out, const double* prec_out, const int32_t* charge_out,
                      const int32_t* status, const void* workspace, size_t workspace_bytes) {
  if (!csr_ok(csr) || !params || !info || !out || !out->count || !prec_out || !charge_out || !status)
    return fail(SPX_EINVAL, "spx_bin_mean: null argument");
  if (!(params->binsize > 0) || !(params->maximum > params->minimum))
    return fail(SPX_EINVAL, "spx_bin_mean: need binsize > 0 and maximum > minimum");
  if (csr->n_peaks && (!out->mz || !out->inten)) return fail(SPX_EINVAL, "spx_bin_mean: null output arrays");
  const size_t need = spx_bin_mean_workspace_size(csr, params, info);
  if (!workspace || workspace_bytes < need) return fail(SPX_ENOSPACE, "spx_bin_mean: workspace too small");
  return SPX_SUCCESS;
}

// What one bin_mean_impl call launches.  kBmAll/kBmFront/kBmChain are spx_bin_mean_stage's
// stages 0/1/2; kBmHead (the memset and the head kernel only) and kBmTail (everything after
// the head, on the same workspace) split spx_bin_mean_medoid_stage's pass.
enum BmStage { kBmAll = 0, kBmFront = 1, kBmChain = 2, kBmHead = 3, kBmTail = 4 };

// what one kept_fold call launches: all of it, the set-up kernel only, or the rest
enum FoldPart { kFoldAll, kFoldSetup, kFoldRest };

int bin_mean_impl(const spx_csr* csr, const spx_bin_params* params, const spx_batch_info* info,
                  spx_peaks_out* out, double* prec_out, int32_t* charge_out, int32_t* status, void* workspace,
                  size_t workspace_bytes, void* stream, int stage, const BinMeanHead* head) {
  if (stage < kBmAll || stage > kBmTail) return fail(SPX_EINVAL, "bin_mean_impl: stage must be 0..4 (BmStage)");
  if (int rc = bin_mean_validate(csr, params, info, out, prec_out, charge_out, status, workspace, workspace_bytes))
    return rc;
  const int64_t C = csr->n_clusters;
  if (C == 0) return SPX_SUCCESS;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Carver w{static_cast<char*>(workspace), 0};
  const BinMeanWs W = carve_bin_mean(w, csr, params, info);
  auto cnt = [&](BmCounter slot) { return W.counters + slot; };

  spx::BinMeanParams P;
  P.minimum = params->minimum;
  P.maximum = params->maximum;
  P.binsize = params->binsize;
  P.inv_binsize = 1.0 / params->binsize;
  P.apply_quorum = params->apply_peak_quorum ? 1 : 0;
  P.n_words = bin_words(params);
  spx::PeaksOut O{out->mz, out->inten, out->count};
  const spx::CsrView V = view(csr);
  const int64_t dcap = std::max<int64_t>(1, info->max_cluster_peaks);

  const dim3 gcl((unsigned)std::max<int64_t>(1, std::min<int64_t>(C, 2048)));
  const dim3 bsg(spx::SG_BLOCK), bbm(spx::BM_BLOCK);
  // the kept-bin fold (bin_mean_q.hip) over one list of clusters, on stream q
  auto kept_fold = [&](const KeptFoldWs& K, hipStream_t q, FoldPart part) -> int {
    const dim3 gqt((unsigned)std::max(1, std::min(K.task_cap, 8192)));
    if (part != kFoldRest) {
      if (int rc = SPX_LAUNCH(bin_mean_q_setup_kernel, gcl, bsg, q, V, P, O, prec_out, charge_out, status, K.list,
                              K.n_list, K.meta, W.arena, W.bump, W.arena_bytes, K.task_cl, K.n_tasks, K.task_cap,
                              K.tile_cl, K.n_tiles, K.tile_cap, kept_fold_enabled()))
        return rc;
      if (part == kFoldSetup) return SPX_SUCCESS;
    }
    int rc = SPX_LAUNCH(bin_mean_q_tally_kernel, gqt, bsg, q, V, P, K.meta, W.arena, K.task_cl, K.n_tasks, K.task_cap);
    if (!rc) rc = SPX_LAUNCH(bin_mean_q_count_kernel, dim3((unsigned)std::max(1, std::min(K.tile_cap, 8192))), bsg, q,
                             K.meta, W.arena, K.tile_cl, K.n_tiles, K.tile_cap);
    if (!rc) rc = SPX_LAUNCH(bin_mean_q_plan_kernel, gcl, bsg, q, K.n_list, K.meta, W.arena, W.bump, W.arena_bytes,
                             K.unit_cl, K.n_units, K.unit_cap);
    if (!rc) rc = SPX_LAUNCH(bin_mean_q_place_kernel, gqt, bsg, q, V, P, K.meta, W.arena, K.task_cl, K.n_tasks,
                             K.task_cap);
    if (!rc) rc = SPX_LAUNCH(bin_mean_q_fold_kernel, dim3((unsigned)std::max(1, std::min(K.unit_cap, 2048))),
                             dim3(spx::QF_BLOCK), q, K.meta, W.arena, K.unit_cl, K.n_units, K.unit_cap);
    if (!rc) rc = SPX_LAUNCH(bin_mean_q_emit_kernel, gcl, bsg, q, V, O, prec_out, charge_out, status, K.n_list, K.meta,
                             W.arena, W.seg_in, cnt(kBmcSegIn), W.glist, cnt(kBmcGlobal));
    return rc;
  };
  // The intake (spx_bin_mean's whole chain only, with the quorum): the clusters past the wide
  // kernel by size go to a list of their own at once, and their kept-bin fold runs on the
  // side stream while the register and wide kernels take the rest on `s`; the wide kernel
  // leaves them alone, its own leftovers take a second kept-bin fold on `s`, and the chain
  // after it (segmented fold, split path, global kernel) waits for both.
  const bool intake = stage == kBmAll && !head && P.apply_quorum && kept_fold_enabled() &&
                      bin_mean_intake_possible(info);
  SideFork side("spx_bin_mean");
  auto global_pass = [&]() {
    return SPX_LAUNCH(bin_mean_global_kernel, dim3((unsigned)bin_mean_fallback_grid(C, params, dcap)), bbm, s, V, P, O,
                      prec_out, charge_out, status, W.glist, cnt(kBmcGlobal), W.scratch,
                      spx::bin_mean_slice_bytes(P.n_words, dcap), (int)std::min<int64_t>(dcap, INT32_MAX));
  };
  // stage 0/1: the counters, the bump pointer and the striped list's counters after them
  // (W.zeroed), then the register path, whose leftovers (longer spectra, more spectra,
  // unsorted, > 1,536 bins) all go to the wide kernel
  if (stage == kBmAll || stage == kBmFront || stage == kBmHead) {
    if (hipMemsetAsync(W.counters, 0, W.zeroed, s) != hipSuccess) return check_launch("spx_bin_mean memset");
    if (intake) {
      if (int rc = side.begin(s)) return rc;
      if (int rc = SPX_LAUNCH(bin_mean_intake_kernel, dim3((unsigned)std::min<int64_t>((C + 255) / 256, 1024)),
                              dim3(256), side.stream(), V, P, W.fold_in.list, W.fold_in.n_list))
        return rc;
      // the kept-bin fold's set-up (a few long latency chains: the big clusters' offsets,
      // charges and window) alone on the GPU, before the register kernel fills it
      if (int rc = kept_fold(W.fold_in, side.stream(), kFoldSetup)) return rc;
      if (int rc = side.mark_mid()) return rc;
      if (int rc = side.wait_mid(s)) return rc;
    }
    if (head) {
      if (int rc = head->launch(head->ctx, V, P, O, prec_out, charge_out, status, W.rest, cnt(kBmcUnused), s))
        return rc;
    } else {
      if (int rc = SPX_LAUNCH_TIMED(ProfScope(kProfBinMeanReg, s), bin_mean_reg_kernel, dim3((unsigned)C), bbm, s, V, P,
                                    O, prec_out, charge_out, status, W.rest))
        return rc;
    }
    if (intake) {  // (after the register kernel's launch: the side stream's launches would delay it)
      if (int rc = kept_fold(W.fold_in, side.stream(), kFoldRest)) return rc;
      if (int rc = side.mark_join()) return rc;
    }
  }
  if (stage == kBmHead) return SPX_SUCCESS;  // the head's leftovers stay on W.rest for kBmTail
  if (stage != kBmChain) {
    if (int rc = SPX_LAUNCH(bin_mean_wide_kernel, gcl, dim3(spx::BW_BLOCK), s, V, P, O, prec_out, charge_out, status,
                            W.rest, W.fold.list, W.fold.n_list, W.glist, cnt(kBmcGlobal), intake ? 1 : 0))
      return rc;
  }
  if (stage == kBmFront) return global_pass();  // clusters past the wide kernel keep status SPX_UNRESOLVED
  if (stage == kBmChain) {
    // the global kernel's list was consumed by stage 1: the chain's own start at 0
    if (hipMemsetAsync(cnt(kBmcGlobal), 0, sizeof(int32_t), s) != hipSuccess)
      return check_launch("spx_bin_mean memset");
  }
  // kept-bin fold of the clusters past the wide kernel (the quorum applies)
  if (int rc = kept_fold(W.fold, s, kFoldAll)) return rc;
  // the segmented fold reads what both kept-bin folds passed on
  if (intake)
    if (int rc = side.wait_join(s)) return rc;
  // segmented fold of what the kept-bin fold passes on (no quorum, no room)
  const dim3 gtask((unsigned)std::max<int64_t>(1, std::min<int64_t>(W.n_task_cap, 8192)));
  const dim3 gtile((unsigned)std::max<int64_t>(1, std::min<int64_t>(W.n_tile_cap, 8192)));
  int rc = SPX_LAUNCH(bin_mean_seg_setup_kernel, gcl, bsg, s, V, P, O, prec_out, charge_out, status, W.seg_in,
                      cnt(kBmcSegIn), W.meta, W.arena, W.bump, W.arena_bytes, W.task_cl, cnt(kBmcSegTasks));
  if (!rc) rc = SPX_LAUNCH(bin_mean_seg_occupy_kernel, gtask, bsg, s, V, P, W.meta, W.arena, W.task_cl,
                           cnt(kBmcSegTasks));
  if (!rc) rc = SPX_LAUNCH(bin_mean_seg_prefix_kernel, gcl, bsg, s, V, P, O, prec_out, charge_out, status,
                           cnt(kBmcSegIn), W.meta, W.arena, W.bump, W.arena_bytes, W.tile_cl, cnt(kBmcSegTiles));
  if (!rc) rc = SPX_LAUNCH(bin_mean_seg_mask_kernel, gtask, bsg, s, V, P, W.meta, W.arena, W.task_cl,
                           cnt(kBmcSegTasks));
  if (!rc) rc = SPX_LAUNCH(bin_mean_seg_count_kernel, gtile, bsg, s, W.meta, W.arena, W.tile_cl, cnt(kBmcSegTiles));
  if (!rc) rc = SPX_LAUNCH(bin_mean_seg_scan_kernel, gcl, bsg, s, cnt(kBmcSegIn), W.meta, W.arena);
  if (!rc) rc = SPX_LAUNCH(bin_mean_seg_place_kernel, gtask, bsg, s, V, P, W.meta, W.arena, W.task_cl,
                           cnt(kBmcSegTasks));
  if (!rc) rc = SPX_LAUNCH(bin_mean_seg_fold_kernel, gtile, bsg, s, P, W.meta, W.arena, W.tile_cl, cnt(kBmcSegTiles));
  if (!rc) rc = SPX_LAUNCH(bin_mean_seg_emit_kernel, gcl, bsg, s, V, O, prec_out, charge_out, status, cnt(kBmcSegIn),
                           W.meta, W.arena, W.split_list, cnt(kBmcSplitList), W.glist, cnt(kBmcGlobal));
  // bin-range split path for what the arena could not hold, then the global kernel
  if (!rc) rc = SPX_LAUNCH(bin_mean_split_plan_kernel, gcl, bbm, s, V, P, O, prec_out, charge_out, status, W.split_list,
                           cnt(kBmcSplitList), W.scl, cnt(kBmcSplitClusters), W.ranges, cnt(kBmcSplitRanges),
                           W.range_cap, W.glist, cnt(kBmcGlobal));
  if (!rc) rc = SPX_LAUNCH(bin_mean_split_fold_kernel, dim3(4096), bbm, s, V, P, O, W.scl, W.ranges,
                           cnt(kBmcSplitRanges), W.range_cap);
  if (!rc) rc = SPX_LAUNCH(bin_mean_split_emit_kernel, gcl, bbm, s, V, P, O, prec_out, charge_out, status, W.scl,
                           cnt(kBmcSplitClusters), W.ranges, W.glist, cnt(kBmcGlobal));
  return rc ? rc : global_pass();
}

// -------------------------------------------------------------- gap-average
// Bitmap words of the gap-average global slice: the batch's m/z span in
// half-accuracy buckets.  A non-finite or absurd span (a caller's bad info) is
// clamped: clusters past the slice report SPX_UNRESOLVED, they are never read
// out of bounds.
int gap_wcap(const spx_gap_params* p, const spx_batch_info* info) {
  double span = (info && info->max_mz_span > 0) ? info->max_mz_span : 5000.0;
  if (!std::isfinite(span)) span = 5000.0;
  const double w = std::ceil((span / (p->mz_accuracy * 0.5) + 3.0) / 64.0);
  return (int)std::min(w, (double)(1 << 24));
}

// The giant pipeline's arena (gap_average.hip, GA_GIANT_N): none when no cluster can
// be a giant, else room for the giants the batch can hold, within a 1 GiB budget
// (a giant it cannot take stays in the global kernel).
int64_t gap_giant_arena(const spx_csr* csr, const spx_gap_params* params, const spx_batch_info* info) {
  const int64_t maxp = info->max_cluster_peaks;
  if (maxp <= spx::GA_GIANT_N) return 0;
  const int wcap = gap_wcap(params, info);
  const int64_t dg = std::min<int64_t>(maxp, (int64_t)wcap * 64);
  const int64_t per = spx::gap_slice_bytes(wcap, (int)std::min<int64_t>(dg, INT32_MAX));
  const int64_t giants = std::min<int64_t>(spx::GA_GMAX, csr->n_peaks / (spx::GA_GIANT_N + 1));
  return std::min<int64_t>(int64_t(1) << 30, per * std::max<int64_t>(giants, 1));
}

// Pass 5's partial records (gap_giant_tiles_kernel<5>, gap_giant_reduce_kernel): a
// per-(giant, tile) offset for every tile a batch's giants can have, and an arena of at
// most 256 MiB for the records (a tile whose records do not fit flushes by atomics).
int64_t gap_giant_tile_slots(const spx_csr* csr, const spx_batch_info* info, int64_t tile) {
  if (info->max_cluster_peaks <= spx::GA_GIANT_N) return 0;
  return csr->n_peaks / tile + spx::GA_GMAX + 1;
}
int64_t gap_partials_cap(const spx_csr* csr, const spx_batch_info* info) {
  if (info->max_cluster_peaks <= spx::GA_GIANT_N) return 0;
  return std::min<int64_t>(int64_t(256) << 20, csr->n_peaks * 6 + (int64_t(1) << 20));
}

int64_t gap_fallback_grid(int64_t C, const spx_gap_params* params, const spx_batch_info* info) {
  const int64_t dcap = std::max<int64_t>(1, info->max_cluster_peaks);
  return fallback_grid_sized(C, spx::gap_slice_bytes(gap_wcap(params, info), (int)std::min<int64_t>(dcap, INT32_MAX)));
}

// What one run of the giant pipeline works on: a table of giants and its count, the arena
// of pass 5's partial records with its bump pointer, and the per-(giant, tile) offsets.
struct GiantTable {
  spx::GapGiant* giants;
  int32_t* n_giant;
  char* part;
  unsigned long long* part_used;
  long long* tile_off;
  int64_t tile;  // peaks per tile
};

struct GapWs {
  int32_t *n_def, *unresolved;
  size_t zeroed;  // bytes from `n_def` the opening memset clears: the counters, both giant tables, wide.counts
  unsigned long long* arena_used;
  // the global kernel's giants (data-dependent, few: GA_TILE_LATE) and the intake's (GA_TILE)
  GiantTable late, in;
  spx::StripedList wide;  // the LDS kernel's leftovers for the wide kernel
  int32_t* def;           // the wide kernel's leftovers for the global kernel
  uint8_t* owned;         // the intake's second tier, per cluster
  char *arena, *scratch;  // the giants' slices (both tables); the global kernel's
  int64_t arena_bytes, part_cap;
};

// The workspace layout (the size query and the launch use the same carving).
GapWs carve_gap(Carver& w, const spx_csr* csr, const spx_gap_params* params, const spx_batch_info* info) {
  const size_t C = (size_t)std::max<int64_t>(csr->n_clusters, 1);
  const size_t begin = w.used;
  GapWs W;
  W.n_def = w.take<int32_t>(1);
  W.unresolved = w.take<int32_t>(1);
  W.late.n_giant = w.take<int32_t>(1);
  W.arena_used = w.take<unsigned long long>(1);
  W.late.part_used = w.take<unsigned long long>(1);
  W.in.n_giant = w.take<int32_t>(1);
  W.in.part_used = w.take<unsigned long long>(1);
  W.late.giants = w.take<spx::GapGiant>(spx::GA_GMAX);
  W.in.giants = w.take<spx::GapGiant>(spx::GA_GMAX);
  W.wide.counts = w.take<int32_t>((size_t)spx::kListStripes * spx::kListLine);
  W.zeroed = w.used - begin;
  W.wide.cap = spx::striped_cap((int64_t)C);
  W.def = w.take<int32_t>(C);
  W.wide.items = w.take<int32_t>((size_t)W.wide.cap * spx::kListStripes);
  W.arena_bytes = gap_giant_arena(csr, params, info);
  W.arena = w.take<char>((size_t)W.arena_bytes);
  // pass 5's partial records and the per-(giant, tile) offsets (none when no giant is possible)
  W.part_cap = gap_partials_cap(csr, info);
  W.late.tile = spx::GA_TILE_LATE;
  W.late.tile_off = w.take<long long>((size_t)std::max<int64_t>(gap_giant_tile_slots(csr, info, W.late.tile), 1));
  W.late.part = w.take<char>((size_t)std::max<int64_t>(W.part_cap, 1));
  W.owned = w.take<uint8_t>(C);
  W.in.tile = spx::GA_TILE;
  W.in.tile_off = w.take<long long>((size_t)std::max<int64_t>(gap_giant_tile_slots(csr, info, W.in.tile), 1));
  W.in.part = w.take<char>((size_t)std::max<int64_t>(W.part_cap, 1));
  W.scratch = w.base + w.used;
  return W;
}

// ------------------------------------------------------------------- MGF emit
// spx_format_peaks: the segments' offsets among the peaks covered, and the two passes'
// per-workgroup sums
struct FormatWs {
  int64_t *voff, *seg_part, *text_part;
};
FormatWs carve_format(Carver& w, int64_t n_segments) {
  FormatWs W;
  W.voff = w.take<int64_t>((size_t)n_segments + 1);
  W.seg_part = w.take<int64_t>(spx::kFmtSegGrid);
  W.text_part = w.take<int64_t>(spx::kFmtPeakGrid);
  return W;
}

// ------------------------------------------------------------------- medoid
// Arena bytes of one deferred cluster of n spectra and p peaks (K <= p columns).
size_t medoid_cluster_bytes(int64_t n, int64_t p) {
  const int64_t K = std::max<int64_t>(p, 1);  // occupied bins <= peaks
  const int64_t KW = ((K + 63) / 64 + 7) / 8 * 8;
  const int64_t T = (n + spx::MD_GT - 1) / spx::MD_GT;
  const int64_t B1 = std::min<int64_t>(K, 64 * (int64_t)spx::MD_L1WORDS);
  const int64_t L = spx::md_max_leaves(n);
  return (size_t)(spx::md_l1_bytes() + spx::md_align(B1 * 12 + 8) +
                  2 * spx::md_align(T * spx::MD_GT * KW * 8) +
                  spx::md_align(n * n * 4) + spx::md_align((2 * L + 1) * 4) + spx::md_align(2 * (2 * L) * n * 8) +
                  spx::md_align(n * 8));
}

// past the small-cluster kernels by size alone (the register kernel, then the wide one)
bool medoid_large_by_size(int64_t n, int64_t p) { return n > spx::MD_NMAX || p > spx::MW_PMAX; }

// the large path's per-cluster prefix arrays (LargePathWs::base), C + 1 entries each
enum MdBase {
  kMdTileBase,
  kMdUnitBase,
  kMdChunkBase,
  kMdXposeBase,
  kMdPeakBase,
  kMdBases,
  kMdRowBase = kMdPeakBase  // reused: the peak passes are done with it when medoid_scan_kernel fills it
};

// What one run of the large path works on: a list of deferred clusters and its count, a
// record each, and the prefix arrays.
struct LargePathWs {
  int32_t *def, *n_def;
  spx::MedoidMeta* meta;
  int64_t* base[kMdBases];
};

// The fixed part of the workspace (the arena is what follows it).
struct MedoidWs {
  size_t zeroed;  // bytes from `late.n_def` the opening memset clears: both counts, bump and wide.counts
  unsigned long long* bump;
  spx::StripedList wide;  // the register kernel's leftovers for the wide kernel (striped appends)
  LargePathWs late, in;   // the wide kernel's deferrals; the intake's (clusters large by size)
};

// a large path's records and prefix arrays (its list and count are carved by the caller)
void carve_large_path(Carver& w, LargePathWs& L, size_t C) {
  L.meta = w.take<spx::MedoidMeta>(C);
  for (auto& b : L.base) b = w.take<int64_t>(C + 1);
}

// The workspace layout (the size query and the launch use the same carving).
MedoidWs carve_medoid(Carver& w, int64_t n_clusters) {
  const size_t C = (size_t)std::max<int64_t>(n_clusters, 1);
  const size_t begin = w.used;
  MedoidWs W;
  W.late.n_def = w.take<int32_t>(1);
  W.in.n_def = W.late.n_def + 1;  // in the same 256 B
  W.bump = w.take<unsigned long long>(1);
  W.wide.counts = w.take<int32_t>((size_t)spx::kListStripes * spx::kListLine);
  W.zeroed = w.used - begin;
  W.wide.cap = spx::striped_cap((int64_t)C);
  W.late.def = w.take<int32_t>(C);
  W.wide.items = w.take<int32_t>((size_t)W.wide.cap * spx::kListStripes);
  carve_large_path(w, W.late, C);
  W.in.def = w.take<int32_t>(C);
  carve_large_path(w, W.in, C);
  return W;
}

// What the fused kernel needs of a medoid call prepared by kMdPrepare.
struct MedoidHead {
  spx::StripedList wide;
  spx::MedoidParams P;
};

// argument checks of spx_medoid (also run up front by the fused entry point)
int medoid_validate(const spx_csr* csr, const spx_medoid_params* params, const int64_t* rep,
                    const void* workspace) {
  if (!csr_ok(csr) || !params || !rep) return fail(SPX_EINVAL, "spx_medoid: null argument");
  if (!(params->tolerance > 0)) return fail(SPX_EINVAL, "spx_medoid: tolerance must be > 0");
  if (csr->n_clusters > 0 && !workspace) return fail(SPX_ENOSPACE, "spx_medoid: no workspace");
  return SPX_SUCCESS;
}

// What one medoid_impl call does.  kMdAll: the whole call; kMdPrepare: checks, workspace
// carving and the memset only (the caller launches the head kernel: spx_bin_mean_medoid);
// kMdTail: everything after the register kernel (the wide kernel and the large path), on
// the same workspace.
enum MdPart { kMdAll = 0, kMdPrepare = 1, kMdTail = 2 };

int medoid_impl(const spx_csr* csr, const spx_medoid_params* params, int64_t* rep, double* totals, void* workspace,
                size_t workspace_bytes, void* stream, MdPart part, MedoidHead* head) {
  if (int rc = medoid_validate(csr, params, rep, workspace)) return rc;
  const int64_t C = csr->n_clusters;
  if (C == 0) return SPX_SUCCESS;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Carver w{static_cast<char*>(workspace), 0};
  const MedoidWs W = carve_medoid(w, C);
  if (w.used >= workspace_bytes) return fail(SPX_ENOSPACE, "spx_medoid: workspace too small");
  char* arena = w.base + w.used;
  const int64_t arena_bytes = (int64_t)(workspace_bytes - w.used);
  spx::MedoidParams P{params->tolerance, 1.0 / params->tolerance};
  const spx::CsrView V = view(csr);
  const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>(C, 1024));
  // grid-stride passes: 32 deferred clusters at a time x 64 blocks fills the chip,
  // and an empty deferred list (the common case) costs a small launch
  const dim3 grid2(spx::MD_GRIDX, std::min<unsigned>(g, SPX_MD_GRIDY)), blk(spx::MD_BLOCK);

  if (part != kMdTail) {
    if (hipMemsetAsync(W.late.n_def, 0, W.zeroed, s) != hipSuccess) return check_launch("spx_medoid memset");
  }
  if (part == kMdPrepare) {
    head->wide = W.wide;
    head->P = P;
    return SPX_SUCCESS;
  }
  // The large path over one list of deferred clusters, on stream q.
  const int64_t prof_call = g_prof_calls.fetch_add(1);  // both large paths' Gram time: one launch of the call
  auto large_path = [&](const LargePathWs& L, hipStream_t q) -> int {
    int64_t* const* base = L.base;
    int rc = SPX_LAUNCH(medoid_units_kernel, dim3(1), blk, q, V, L.meta, L.n_def, base[kMdPeakBase]);
    // the peak passes: a flat grid over MD_PU-peak units of every deferred cluster
    const dim3 gridu(2048);
    if (!rc) rc = SPX_LAUNCH(medoid_range_kernel, gridu, blk, q, V, P, L.n_def, L.meta, base[kMdPeakBase], arena,
                             W.bump, arena_bytes);
    if (!rc) rc = SPX_LAUNCH(medoid_l1_kernel, gridu, blk, q, V, P, L.n_def, L.meta, base[kMdPeakBase], arena);
    if (!rc) rc = SPX_LAUNCH(medoid_plan1_kernel, dim3(g), blk, q, L.n_def, L.meta, arena, W.bump, arena_bytes, rep);
    if (!rc) rc = SPX_LAUNCH(medoid_l2_kernel, gridu, blk, q, V, P, L.n_def, L.meta, base[kMdPeakBase], arena);
    if (!rc) rc = SPX_LAUNCH(medoid_plan2_kernel, dim3(g), blk, q, L.n_def, L.meta, arena, W.bump, arena_bytes, rep);
    if (!rc) rc = SPX_LAUNCH(medoid_scan_kernel, dim3(1), blk, q, L.meta, L.n_def, base[kMdTileBase], base[kMdUnitBase],
                             base[kMdChunkBase], base[kMdXposeBase], base[kMdRowBase]);
    if (!rc) rc = SPX_LAUNCH(medoid_fill_kernel, grid2, blk, q, V, P, L.meta, L.n_def, base[kMdRowBase], arena);
    if (!rc) rc = SPX_LAUNCH(medoid_transpose_kernel, dim3(4096), blk, q, L.meta, L.n_def, base[kMdXposeBase], arena);
    if (!rc) rc = SPX_LAUNCH_TIMED(ProfScope(kProfMedoidGram, q, prof_call), medoid_gram_reg_kernel, dim3(SPX_GR_GRID),
                                   blk, q, L.meta, L.n_def, base[kMdTileBase], arena);
    if (!rc) rc = SPX_LAUNCH(medoid_leaves_kernel, dim3(4096), blk, q, V, L.meta, L.n_def, base[kMdUnitBase], arena);
    if (!rc) rc = SPX_LAUNCH(medoid_combine_kernel, dim3(1024), blk, q, L.meta, L.n_def, base[kMdChunkBase], arena,
                             totals);
    if (!rc) rc = SPX_LAUNCH(medoid_argmin_kernel, dim3(g), blk, q, L.meta, L.n_def, arena, rep);
    return rc;
  };
  // The intake (spx_medoid's whole call with the large path): the clusters large by size
  // are deferred up front and their large path runs on the side stream while the register
  // and wide kernels take the others on `s`; the register kernel leaves them alone, the wide
  // kernel's own deferrals take a second large path on `s`, which then waits for the first.
  const bool intake = part == kMdAll && params->large_path;
  SideFork side("spx_medoid");
  if (intake)
    if (int rc = side.begin(s)) return rc;
  if (part == kMdAll) {
    if (int rc = SPX_LAUNCH_TIMED(ProfScope(kProfMedoidReg, s), medoid_reg_kernel, dim3((unsigned)C), blk, s, V, P, rep,
                                  totals, W.wide, intake ? 1 : 0))
      return rc;
  }
  if (intake) {  // (after the register kernel's launch: the side stream's launches would delay it)
    if (int rc = SPX_LAUNCH(medoid_intake_kernel, dim3((unsigned)std::min<int64_t>((C + 255) / 256, 1024)), dim3(256),
                            side.stream(), V, rep, W.in.def, W.in.n_def, W.in.meta))
      return rc;
    if (int rc = large_path(W.in, side.stream())) return rc;
    if (int rc = side.mark_join()) return rc;
  }
  if (int rc = SPX_LAUNCH(medoid_wide_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(C, 1024))),
                          dim3(spx::MW_BLOCK), s, V, P, rep, totals, W.wide, W.late.def, W.late.n_def, W.late.meta))
    return rc;
  if (!params->large_path) return SPX_SUCCESS;  // deferred clusters keep rep = SPX_REP_DEFERRED
  if (int rc = large_path(W.late, s)) return rc;
  if (intake) return side.wait_join(s);
  return SPX_SUCCESS;
}

struct FusedCtx {
  const MedoidHead* md;
  int64_t* rep;
  double* totals;
  int64_t C;
  const int32_t* bm_counts;  // set by the launch: the bin-mean hand-off list's stripe counters
};

// The fused kernel is persistent: its grid is the workgroups the device holds at once (CUs x
// workgroups per CU from the occupancy query, asked once per device), at most C.  Its
// workgroups never wait on one another, so any grid >= 1 gives the same results.
// SPX_FU_GRID (environment, tests only) caps it, so one workgroup walks many clusters of a
// small batch (1: the whole batch, in order).
int64_t fused_grid(int64_t C) {
  static std::mutex mu;
  static int64_t slots[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return -1;
  int64_t g = 0;
  {
    std::lock_guard<std::mutex> lock(mu);
    int64_t& cached = slots[dev < 64 ? dev : 63];
    if (dev >= 64 || cached == 0) {
      int cus = 0, per_cu = 0;
      if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
          hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, spx::bin_mean_medoid_kernel, spx::BM_BLOCK, 0) !=
              hipSuccess ||
          cus < 1 || per_cu < 1)
        return -1;
      cached = (int64_t)cus * per_cu;
    }
    g = cached;
  }
  if (const char* e = std::getenv("SPX_FU_GRID")) {
    const long long v = std::strtoll(e, nullptr, 10);
    if (v > 0) g = std::min<int64_t>(g, v);
  }
  return std::max<int64_t>(1, std::min(g, C));
}

int fused_head(void* ctx, const spx::CsrView& V, const spx::BinMeanParams& P, const spx::PeaksOut& O, double* prec_out,
               int32_t* charge_out, int32_t* status, const spx::StripedList& rest, int32_t* queue, hipStream_t s) {
  FusedCtx& F = *static_cast<FusedCtx*>(ctx);
  F.bm_counts = rest.counts;
  const int64_t grid = fused_grid(F.C);
  if (grid < 1) {
    if (int rc = check_launch("spx_bin_mean_medoid occupancy query")) return rc;
    return fail(SPX_EHIP, "spx_bin_mean_medoid: occupancy query failed");
  }
  // the queue head is 32-bit and every workgroup claims once past the end
  if (F.C > (int64_t)INT32_MAX - grid) return fail(SPX_EINVAL, "spx_bin_mean_medoid: too many clusters");
  const spx::FusedArgs A{V,        P,     O,        prec_out,   charge_out, status, rest, F.md->P,
                         F.rep,    F.totals, F.md->wide, reinterpret_cast<uint32_t*>(queue)};
  return SPX_LAUNCH_TIMED(ProfScope(kProfBinMeanMedoid, s), bin_mean_medoid_kernel, dim3((unsigned)grid),
                          dim3(spx::BM_BLOCK), s, A);
}

// ------------------------------------------------------------ binned cosine
struct CosineWs {
  int32_t *n_def, *def;  // clusters deferred to the global kernel, and their count
  char* scratch;         // the global kernel's slices (only when max_rep_peaks > CS_RCAP)
};

CosineWs carve_cosine(Carver& w, int64_t n_clusters) {
  CosineWs W;
  W.n_def = w.take<int32_t>(1);
  W.def = w.take<int32_t>((size_t)std::max<int64_t>(n_clusters, 1));
  W.scratch = w.base + w.used;
  return W;
}

// ------------------------------------------------------------ cosine medoid
spx::CosMedWs carve_cosine_medoid(Carver& w, int64_t n_clusters, int64_t n_spectra, int64_t n_peaks) {
  const size_t P = (size_t)std::max<int64_t>(n_peaks, 1), S = (size_t)std::max<int64_t>(n_spectra, 1);
  spx::CosMedWs W;
  W.rb = w.take<int32_t>(P);
  W.rA = w.take<double>(P);
  W.rE = w.take<double>(P);
  W.rA2 = w.take<double>(P);
  W.nr = w.take<int32_t>(S);
  W.L = w.take<int32_t>(S);
  W.nE = w.take<int32_t>(S);
  W.flag = w.take<int32_t>(S);
  W.tot2 = w.take<double>(S);
  W.score = w.take<double>(S);
  W.n_def = w.take<int32_t>(1);
  W.def = w.take<int32_t>((size_t)std::max<int64_t>(n_clusters, 1));
  return W;
}

// np.arange(-s/2, stop, s): e0 = start, e1 = start + s, e_i = start + i * (e1 - e0)
// (numpy DOUBLE_fill); scipy's on-edge rounding keeps int(-log10(min edge gap)) + 6 decimals
spx::CosParams cosine_params(double mz_space) {
  spx::CosParams P;
  P.s = mz_space;
  P.start = -mz_space / 2.0;
  P.e1 = P.start + P.s;
  P.d = P.e1 - P.start;
  P.inv_d = 1.0 / P.d;
  const int dec = (int)(-std::log10(std::min(P.d, P.s))) + 6;
  P.p10 = std::pow(10.0, (double)dec);
  return P;
}

// runs the LDS image of cosine_medoid_pairs_kernel holds for this batch
int cosine_medoid_rcap(const spx_batch_info* info) {
  const int64_t r = std::max<int64_t>(64, std::min<int64_t>(info->max_cluster_peaks, spx::CM_LDS_RUNS));
  return (int)((r + 63) & ~int64_t(63));
}

}  // namespace

extern "C" {

int spx_abi_version(void) { return SPX_ABI_VERSION; }

#ifdef SPX_STAMPS
// diagnostic builds only: where the phase stamps go (nullptr: off)
int spx_debug_stamps(void* dev_ptr) {
  return hipMemcpyToSymbol(HIP_SYMBOL(spx::g_spx_stamps), &dev_ptr, sizeof(dev_ptr)) == hipSuccess ? 0 : SPX_EHIP;
}
#endif
const char* spx_last_error(void) { return g_err; }

int spx_profile_enable(int on) {
  std::lock_guard<std::mutex> lock(g_prof_mu);
  for (auto& p : g_prof) {
    for (auto& ab : p.pending) {
      (void)hipEventSynchronize(ab.second);
      (void)hipEventDestroy(ab.first);
      (void)hipEventDestroy(ab.second);
    }
    p = ProfAcc{};
  }
  g_prof_on.store(on != 0);
  return SPX_SUCCESS;
}

int spx_profile_read(const char* kernel, double* total_ms, int64_t* launches) {
  const int i = kernel ? prof_index(kernel) : -1;
  if (i < 0 || !total_ms || !launches) return fail(SPX_EINVAL, "spx_profile_read: unknown kernel or null output");
  std::lock_guard<std::mutex> lock(g_prof_mu);
  ProfAcc& p = g_prof[i];
  for (size_t k = 0; k < p.pending.size(); ++k) {
    auto& ab = p.pending[k];
    float ms = 0.0f;
    if (hipEventSynchronize(ab.second) == hipSuccess && hipEventElapsedTime(&ms, ab.first, ab.second) == hipSuccess) {
      p.ms += ms;
      if (p.calls[k] != p.last_call) ++p.launches;  // a call's scopes are recorded back to back
      p.last_call = p.calls[k];
    }
    (void)hipEventDestroy(ab.first);
    (void)hipEventDestroy(ab.second);
  }
  p.pending.clear();
  p.calls.clear();
  *total_ms = p.ms;
  *launches = p.launches;
  return SPX_SUCCESS;
}

int spx_medoid_gram_operand_bits(void) { return 4; }  // FP4 e2m1 (the i8 form is in git history, round 3)

// ------------------------------------------------------------------ bin-mean
size_t spx_bin_mean_workspace_size(const spx_csr* csr, const spx_bin_params* params, const spx_batch_info* info) {
  if (!csr || !params || !info) return 0;
  const int64_t C = csr->n_clusters;
  const int64_t dcap = std::max<int64_t>(1, info->max_cluster_peaks);
  Carver w{nullptr, 0};
  carve_bin_mean(w, csr, params, info);
  return w.used + (size_t)bin_mean_fallback_grid(C, params, dcap) * (size_t)spx::bin_mean_slice_bytes(bin_words(params), dcap);
}

int spx_bin_mean_stage(const spx_csr* csr, const spx_bin_params* params, const spx_batch_info* info,
                       spx_peaks_out* out, double* prec_out, int32_t* charge_out, int32_t* status, void* workspace,
                       size_t workspace_bytes, void* stream, int stage) {
  if (stage < 0 || stage > 2) return fail(SPX_EINVAL, "spx_bin_mean_stage: stage must be 0, 1 or 2");
  return bin_mean_impl(csr, params, info, out, prec_out, charge_out, status, workspace, workspace_bytes, stream, stage,
                       nullptr);
}

int spx_bin_mean(const spx_csr* csr, const spx_bin_params* params, const spx_batch_info* info, spx_peaks_out* out,
                 double* prec_out, int32_t* charge_out, int32_t* status, void* workspace, size_t workspace_bytes,
                 void* stream) {
  return spx_bin_mean_stage(csr, params, info, out, prec_out, charge_out, status, workspace, workspace_bytes, stream,
                            0);
}

// -------------------------------------------------------------- gap-average
size_t spx_gap_average_workspace_size(const spx_csr* csr, const spx_gap_params* params, const spx_batch_info* info) {
  if (!csr || !params || !info) return 0;
  const int64_t dcap = std::max<int64_t>(1, info->max_cluster_peaks);
  Carver w{nullptr, 0};
  carve_gap(w, csr, params, info);
  return w.used + (size_t)gap_fallback_grid(csr->n_clusters, params, info) *
                      (size_t)spx::gap_slice_bytes(gap_wcap(params, info), (int)std::min<int64_t>(dcap, INT32_MAX));
}

int spx_gap_average(const spx_csr* csr, const spx_gap_params* params, const spx_batch_info* info, spx_peaks_out* out,
                    double* pepmass_out, int32_t* charge_out, double* rt_out, int32_t* status, void* workspace,
                    size_t workspace_bytes, void* stream) {
  if (!csr_ok(csr) || !params || !info || !out || !out->count || !pepmass_out || !charge_out || !rt_out || !status)
    return fail(SPX_EINVAL, "spx_gap_average: null argument");
  if (csr->n_spectra && !csr->rt) return fail(SPX_EINVAL, "spx_gap_average: rt array required");
  if (!(params->mz_accuracy > 0)) return fail(SPX_EINVAL, "spx_gap_average: mz_accuracy must be > 0");
  if (csr->n_peaks && (!out->mz || !out->inten)) return fail(SPX_EINVAL, "spx_gap_average: null output arrays");
  const size_t need = spx_gap_average_workspace_size(csr, params, info);
  if (!workspace || workspace_bytes < need) return fail(SPX_ENOSPACE, "spx_gap_average: workspace too small");
  const int64_t C = csr->n_clusters;
  if (C == 0) return SPX_SUCCESS;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Carver w{static_cast<char*>(workspace), 0};
  const GapWs W = carve_gap(w, csr, params, info);
  spx::GapParams P;
  P.mz_accuracy = params->mz_accuracy;
  P.dyn_range = params->dyn_range;
  P.min_fraction = params->min_fraction;
  P.proton = params->proton;
  P.pepmass_mode = params->pepmass_mode;
  P.rt_mode = params->rt_mode;
  P.bucket_w = params->mz_accuracy;
  P.inv_bucket_w = 1.0 / params->mz_accuracy;
  spx::PeaksOut O{out->mz, out->inten, out->count};
  const spx::CsrView V = view(csr);
  const int wcap = gap_wcap(params, info);
  const int dcap = (int)std::min<int64_t>(std::max<int64_t>(1, info->max_cluster_peaks), INT32_MAX);

  spx::GapParams P2 = P;  // half-width buckets: no gap can hide inside one
  P2.bucket_w = params->mz_accuracy * 0.5;
  P2.inv_bucket_w = 1.0 / P2.bucket_w;
  const int gmax = spx::GA_GMAX;
  const dim3 tiles(spx::GA_GIANT_GRID), per(gmax), blk(spx::GA_BLOCK);
  // the giant clusters' pipeline over one giant table, on stream `q`
  auto giant_pipeline = [&](const GiantTable& T, hipStream_t q) -> int {
    const spx::GiantArgs A{V, P2, T.giants, T.n_giant, gmax, W.arena, wcap, O.mz, O.inten, O.count,
                           T.part, (long long)W.part_cap, T.part_used, T.tile_off, T.tile};
    int rc = SPX_LAUNCH(gap_giant_tiles_kernel<1>, tiles, blk, q, A);
    if (!rc) rc = SPX_LAUNCH(gap_giant_tiles_kernel<2>, tiles, blk, q, A);
    if (!rc) rc = SPX_LAUNCH(gap_giant_step_kernel<0>, per, blk, q, A, O, pepmass_out, charge_out, rt_out, status,
                             W.unresolved);
    if (!rc) rc = SPX_LAUNCH(gap_giant_tiles_kernel<3>, tiles, blk, q, A);
    if (!rc) rc = SPX_LAUNCH(gap_giant_reduce_kernel<3>, tiles, blk, q, A);
    if (!rc) rc = SPX_LAUNCH(gap_giant_groups_kernel<0>, tiles, blk, q, A);
    if (!rc) rc = SPX_LAUNCH(gap_giant_groups_kernel<1>, per, blk, q, A);
    if (!rc) rc = SPX_LAUNCH(gap_giant_groups_kernel<2>, tiles, blk, q, A);
    if (!rc) rc = SPX_LAUNCH(gap_giant_groups_kernel<3>, tiles, blk, q, A);
    if (!rc) rc = SPX_LAUNCH(gap_giant_tiles_kernel<5>, tiles, blk, q, A);
    if (!rc) rc = SPX_LAUNCH(gap_giant_reduce_kernel<5>, tiles, blk, q, A);
    if (!rc) rc = SPX_LAUNCH(gap_giant_groups_kernel<4>, tiles, blk, q, A);
    if (!rc) rc = SPX_LAUNCH(gap_giant_groups_kernel<5>, tiles, blk, q, A);
    if (!rc) rc = SPX_LAUNCH(gap_giant_groups_kernel<6>, per, blk, q, A);
    if (!rc) rc = SPX_LAUNCH(gap_giant_groups_kernel<7>, tiles, blk, q, A);
    if (!rc) rc = SPX_LAUNCH(gap_giant_step_kernel<6>, per, blk, q, A, O, pepmass_out, charge_out, rt_out, status,
                             W.unresolved);
    return rc;
  };

  // the counters, the giants' records and the striped list's counters
  if (hipMemsetAsync(W.n_def, 0, W.zeroed, s) != hipSuccess) return check_launch("spx_gap_average memset");
  // Clusters past SPX_GA_WMAXN peaks (the skewed law's giants) are known by size alone:
  // with any in the batch, the intake registers them and their pipeline runs on the side
  // stream while the LDS and wide kernels take the rest on the caller's (own_n tells those
  // two to leave such clusters alone).  The global kernel waits for the intake (its list
  // takes what the intake's table could not) and hands ITS giants (data-dependent: more
  // than 16,384 peaks and deferred by the wide kernel) to the second table's pipeline.
  const bool intake = W.arena_bytes > 0 && info->max_cluster_peaks > spx::GA_OWN_N;
  const int64_t own_n = intake ? spx::GA_OWN_N : 0;
  const int64_t own_lo = intake ? spx::GA_OWN_LO : 0;
  static_assert(spx::GA_OWN_N > spx::GA_GIANT_N && (spx::GA_OWN_LO == 0 || spx::GA_OWN_LO > spx::GA_GIANT_N),
                "the intake takes giants only");
  SideFork side("spx_gap_average");
  if (intake)
    if (int rc = side.begin(s)) return rc;
  // the LDS kernel first: the side stream's 17 launches would otherwise delay its start
  if (int rc = SPX_LAUNCH_TIMED(ProfScope(kProfGapLds, s), gap_average_lds_kernel, dim3((unsigned)C), blk, s, V, P, O,
                                pepmass_out, charge_out, rt_out, status, W.wide, own_n, own_lo))
    return rc;
  if (intake) {
    if (hipMemsetAsync(W.owned, 0, (size_t)C, side.stream()) != hipSuccess)
      return check_launch("spx_gap_average memset");
    const dim3 gin((unsigned)std::min<int64_t>((C + 255) / 256, 1024));
    if (int rc = SPX_LAUNCH(gap_giant_intake_kernel<0>, gin, dim3(256), side.stream(), V, own_n, own_lo, W.in.giants,
                            W.in.n_giant, gmax, W.arena_used, (long long)W.arena_bytes, wcap, W.def, W.n_def, W.owned))
      return rc;
    if (own_lo > 0)
      if (int rc = SPX_LAUNCH(gap_giant_intake_kernel<1>, gin, dim3(256), side.stream(), V, own_n, own_lo, W.in.giants,
                              W.in.n_giant, gmax, W.arena_used, (long long)W.arena_bytes, wcap, W.def, W.n_def,
                              W.owned))
        return rc;
    if (int rc = side.mark_mid()) return rc;
    if (int rc = giant_pipeline(W.in, side.stream())) return rc;
    if (int rc = side.mark_join()) return rc;
    // the wide kernel reads `owned` and appends to the global kernel's list after the intake
    if (int rc = side.wait_mid(s)) return rc;
  }
  if (int rc = SPX_LAUNCH_TIMED(ProfScope(kProfGapWide, s), gap_average_wide_kernel,
                                dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(C, 256))), blk, s, V, P, O,
                                pepmass_out, charge_out, rt_out, status, W.wide, W.def, W.n_def, own_n,
                                intake ? W.owned : nullptr))
    return rc;
  if (int rc = SPX_LAUNCH(gap_average_global_kernel, dim3((unsigned)gap_fallback_grid(C, params, info)), blk, s, V, P2,
                          O, pepmass_out, charge_out, rt_out, status, W.def, W.n_def, W.scratch,
                          spx::gap_slice_bytes(wcap, dcap), wcap, dcap, W.unresolved, W.late.giants, W.late.n_giant,
                          gmax, W.arena_used, (long long)W.arena_bytes))
    return rc;
  if (W.arena_bytes > 0) {  // (arena_bytes == 0: no cluster of this batch can be a giant)
    if (int rc = giant_pipeline(W.late, s)) return rc;
  }
  if (intake) return side.wait_join(s);
  return SPX_SUCCESS;
}

// ------------------------------------------------------------------- medoid
size_t spx_medoid_workspace_size(const int64_t* hco, const int64_t* hso, int64_t C, const int64_t* extra,
                                 int64_t n_extra) {
  if (C < 0 || (C > 0 && (!hco || !hso)) || n_extra < 0 || (n_extra > 0 && !extra)) return 0;
  Carver w{nullptr, 0};
  carve_medoid(w, C);
  const size_t fixed = w.used;
  size_t arena = 0, margin = 0;
  // small clusters with more peaks than the wide kernel has bin words for: the only
  // ones a run can defer into the arena (their arena bytes)
  std::vector<size_t> risk;
  for (int64_t c = 0; c < C; ++c) {
    const int64_t n = hco[c + 1] - hco[c];
    const int64_t p = hso[hco[c + 1]] - hso[hco[c]];
    const size_t bytes = medoid_cluster_bytes(n, p);
    if (medoid_large_by_size(n, p)) arena += bytes;
    else if (n > 1) {
      margin = std::max(margin, bytes);
      if (p > 64 * (int64_t)spx::MW_KWMAX) risk.push_back(bytes);
    }
  }
  for (int64_t k = 0; k < n_extra; ++k) {
    const int64_t c = extra[k];
    if (c < 0 || c >= C) return 0;
    arena += medoid_cluster_bytes(hco[c + 1] - hco[c], hso[hco[c + 1]] - hso[hco[c]]);
  }
  // Room for run-time deferrals on top: the arena bytes of the 256 largest at-risk
  // clusters (all of them when fewer) PLUS 8 slots of the largest small cluster -- the
  // fixed headroom is for clusters deferred for another reason (an m/z past the
  // register kernel's bin range), which the at-risk list does not predict.  A call that
  // still runs out reports SPX_REP_ARENA for the rest, and a re-run with those clusters
  // in `extra` has room for every one.
  const size_t slots = std::min<size_t>(risk.size(), 256);
  if (slots < risk.size())
    std::nth_element(risk.begin(), risk.begin() + (ptrdiff_t)slots, risk.end(), std::greater<size_t>());
  size_t reserve = 0;
  for (size_t k = 0; k < slots; ++k) reserve += risk[k];
  reserve += 8 * margin;
  return fixed + arena + reserve + (size_t(1) << 20);
}

int spx_medoid_needs_large_path(const int64_t* hco, const int64_t* hso, int64_t C) {
  for (int64_t c = 0; c < C; ++c)
    if (medoid_large_by_size(hco[c + 1] - hco[c], hso[hco[c + 1]] - hso[hco[c]])) return 1;
  return 0;
}

int spx_medoid(const spx_csr* csr, const spx_medoid_params* params, int64_t* rep, double* totals, void* workspace,
               size_t workspace_bytes, void* stream) {
  return medoid_impl(csr, params, rep, totals, workspace, workspace_bytes, stream, kMdAll, nullptr);
}

int spx_bin_mean_medoid_stage(const spx_csr* csr, const spx_bin_params* bin_params, const spx_batch_info* info,
                              spx_peaks_out* out, double* prec_out, int32_t* charge_out, int32_t* status,
                              void* bin_workspace, size_t bin_workspace_bytes, const spx_medoid_params* medoid_params,
                              int64_t* rep, double* totals, void* medoid_workspace, size_t medoid_workspace_bytes,
                              void* stream, int stage, int32_t* handoff) {
  if (!csr_ok(csr)) return fail(SPX_EINVAL, "spx_bin_mean_medoid: null argument");
  if (stage < 0 || stage > 2) return fail(SPX_EINVAL, "spx_bin_mean_medoid_stage: stage must be 0, 1 or 2");
  // both methods' checks before anything is enqueued (and before the empty-batch return)
  if (int rc = bin_mean_validate(csr, bin_params, info, out, prec_out, charge_out, status, bin_workspace,
                                 bin_workspace_bytes))
    return rc;
  if (int rc = medoid_validate(csr, medoid_params, rep, medoid_workspace)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (csr->n_clusters == 0) {
    if (stage == 1 && handoff && hipMemsetAsync(handoff, 0, 2 * sizeof(int32_t), s) != hipSuccess)
      return check_launch("spx_bin_mean_medoid_stage memset");
    return SPX_SUCCESS;
  }
  if (stage == 2) {  // both leftover chains, on the workspaces stage 1 left
    if (int rc = bin_mean_impl(csr, bin_params, info, out, prec_out, charge_out, status, bin_workspace,
                               bin_workspace_bytes, stream, kBmTail, nullptr))
      return rc;
    return medoid_impl(csr, medoid_params, rep, totals, medoid_workspace, medoid_workspace_bytes, stream, kMdTail,
                       nullptr);
  }
  MedoidHead H{};
  if (int rc = medoid_impl(csr, medoid_params, rep, totals, medoid_workspace, medoid_workspace_bytes, stream,
                           kMdPrepare, &H))
    return rc;
  FusedCtx F{&H, rep, totals, csr->n_clusters, nullptr};
  const BinMeanHead head{fused_head, &F};
  if (int rc = bin_mean_impl(csr, bin_params, info, out, prec_out, charge_out, status, bin_workspace,
                             bin_workspace_bytes, stream, stage == 0 ? kBmAll : kBmHead, &head))
    return rc;
  if (stage == 0)
    return medoid_impl(csr, medoid_params, rep, totals, medoid_workspace, medoid_workspace_bytes, stream, kMdTail,
                       nullptr);
  if (handoff)
    return SPX_LAUNCH(handoff_count_kernel, dim3(1), dim3(spx::kWave), s, F.bm_counts, H.wide.counts, handoff);
  return SPX_SUCCESS;
}

int spx_bin_mean_medoid(const spx_csr* csr, const spx_bin_params* bin_params, const spx_batch_info* info,
                        spx_peaks_out* out, double* prec_out, int32_t* charge_out, int32_t* status, void* bin_workspace,
                        size_t bin_workspace_bytes, const spx_medoid_params* medoid_params, int64_t* rep,
                        double* totals, void* medoid_workspace, size_t medoid_workspace_bytes, void* stream) {
  return spx_bin_mean_medoid_stage(csr, bin_params, info, out, prec_out, charge_out, status, bin_workspace,
                                   bin_workspace_bytes, medoid_params, rep, totals, medoid_workspace,
                                   medoid_workspace_bytes, stream, 0, nullptr);
}

int spx_xcorr_distance(const spx_csr* csr, const spx_medoid_params* params, const int64_t* pairs, int64_t n_pairs,
                       double* out, void* stream) {
  if (!csr_ok(csr) || !params || (n_pairs > 0 && (!pairs || !out)))
    return fail(SPX_EINVAL, "spx_xcorr_distance: null argument");
  if (!(params->tolerance > 0)) return fail(SPX_EINVAL, "spx_xcorr_distance: tolerance must be > 0");
  if (n_pairs <= 0) return SPX_SUCCESS;
  spx::MedoidParams P{params->tolerance, 1.0 / params->tolerance};
  return SPX_LAUNCH(xcorr_pairs_kernel, dim3((unsigned)std::min<int64_t>(n_pairs, 65536)), dim3(spx::XC_BLOCK),
                    reinterpret_cast<hipStream_t>(stream), view(csr), P, pairs, n_pairs, out);
}

// ------------------------------------------------------------ binned cosine
size_t spx_binned_cosine_workspace_size(int64_t n_clusters, int64_t max_rep_peaks) {
  if (n_clusters < 0 || max_rep_peaks < 0) return 0;
  const int64_t cap = std::max<int64_t>(max_rep_peaks, 1);
  Carver w{nullptr, 0};
  carve_cosine(w, n_clusters);
  return w.used +
         (max_rep_peaks > spx::CS_RCAP ? (size_t)fallback_grid(n_clusters) * (size_t)spx::cos_slice_bytes(cap) : 0);
}

int spx_binned_cosine(const spx_csr* csr, const int64_t* rep_off, const double* rep_mz, const double* rep_inten,
                      const spx_cosine_params* params, double* cos_out, double* avg_out, int32_t* status,
                      int64_t max_rep_peaks, void* workspace, size_t workspace_bytes, void* stream) {
  if (!csr_ok(csr) || !rep_off || !params || !avg_out || !status || (csr->n_spectra && !cos_out))
    return fail(SPX_EINVAL, "spx_binned_cosine: null argument");
  if (!(params->mz_space > 0)) return fail(SPX_EINVAL, "spx_binned_cosine: mz_space must be > 0");
  const int64_t C = csr->n_clusters;
  const size_t need = spx_binned_cosine_workspace_size(C, max_rep_peaks);
  if (need == 0 || !workspace || workspace_bytes < need) return fail(SPX_ENOSPACE, "spx_binned_cosine: workspace too small");
  if (C == 0) return SPX_SUCCESS;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Carver w{static_cast<char*>(workspace), 0};
  const CosineWs W = carve_cosine(w, C);
  // np.arange(-s/2, stop, s): e0 = start, e1 = start + s, e_i = start + i * (e1 - e0)
  // (numpy DOUBLE_fill); scipy's on-edge rounding keeps int(-log10(min edge gap)) + 6 decimals
  spx::CosParams P;
  P.s = params->mz_space;
  P.start = -params->mz_space / 2.0;
  P.e1 = P.start + P.s;
  P.d = P.e1 - P.start;
  P.inv_d = 1.0 / P.d;
  const int dec = (int)(-std::log10(std::min(P.d, P.s))) + 6;
  P.p10 = std::pow(10.0, (double)dec);
  if (hipMemsetAsync(W.n_def, 0, sizeof(int32_t), s) != hipSuccess) return check_launch("spx_binned_cosine memset");
  if (int rc = SPX_LAUNCH(binned_cosine_kernel, dim3((unsigned)C), dim3(spx::CS_BLOCK), s, view(csr), P, rep_off,
                          rep_mz, rep_inten, cos_out, avg_out, status, W.def, W.n_def))
    return rc;
  if (max_rep_peaks <= spx::CS_RCAP) return SPX_SUCCESS;  // nothing can be deferred
  return SPX_LAUNCH(binned_cosine_global_kernel, dim3((unsigned)fallback_grid(C)), dim3(spx::CS_BLOCK), s, view(csr), P,
                    rep_off, rep_mz, rep_inten, cos_out, avg_out, status, W.def, W.n_def, W.scratch,
                    (int)std::min<int64_t>(max_rep_peaks, INT32_MAX - 1));
}

// ------------------------------------------------------------ cosine medoid
size_t spx_cosine_medoid_workspace_size(const spx_csr* csr, const spx_batch_info* info) {
  if (!csr || !info || csr->n_clusters < 0 || csr->n_spectra < 0 || csr->n_peaks < 0) return 0;
  Carver w{nullptr, 0};
  carve_cosine_medoid(w, csr->n_clusters, csr->n_spectra, csr->n_peaks);
  return w.used;
}

int spx_cosine_medoid(const spx_csr* csr, const spx_cosine_params* params, const spx_batch_info* info, int64_t* rep,
                      double* score, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  if (!csr_ok(csr) || !params || !info || !rep || !status)
    return fail(SPX_EINVAL, "spx_cosine_medoid: null argument");
  if (!(params->mz_space > 0)) return fail(SPX_EINVAL, "spx_cosine_medoid: mz_space must be > 0");
  const int64_t C = csr->n_clusters, S = csr->n_spectra;
  if (C > INT32_MAX) return fail(SPX_EINVAL, "spx_cosine_medoid: too many clusters");
  const size_t need = spx_cosine_medoid_workspace_size(csr, info);
  if (need == 0 || !workspace || workspace_bytes < need) return fail(SPX_ENOSPACE, "spx_cosine_medoid: workspace too small");
  if (C == 0) return SPX_SUCCESS;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Carver w{static_cast<char*>(workspace), 0};
  const spx::CosMedWs W = carve_cosine_medoid(w, C, S, csr->n_peaks);
  const spx::CosParams P = cosine_params(params->mz_space);
  const spx::CsrView V = view(csr);
  if (hipMemsetAsync(W.n_def, 0, sizeof(int32_t), s) != hipSuccess) return check_launch("spx_cosine_medoid memset");
  if (S > 0) {
    const int64_t waves = spx::CM_BLOCK / spx::kWave;
    const unsigned g1 = (unsigned)std::max<int64_t>(1, std::min<int64_t>((S + waves - 1) / waves, 16384));
    if (int rc = SPX_LAUNCH(cosine_medoid_bin_kernel, dim3(g1), dim3(spx::CM_BLOCK), s, V, P, W)) return rc;
    const unsigned g2 = (unsigned)std::max<int64_t>(1, std::min<int64_t>((S + spx::CM_BLOCK - 1) / spx::CM_BLOCK, 8192));
    if (int rc = SPX_LAUNCH(cosine_medoid_prefix_kernel, dim3(g2), dim3(spx::CM_BLOCK), s, V, W)) return rc;
  }
  const int rcap = cosine_medoid_rcap(info);
  const size_t lds = spx::cm_lds_bytes(rcap);
  if (lds > 65536 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(spx::cosine_medoid_pairs_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return fail(SPX_EHIP, "spx_cosine_medoid: LDS size attribute");
  hipLaunchKernelGGL(spx::cosine_medoid_pairs_kernel, dim3((unsigned)C), dim3(spx::CM_PAIR_BLOCK), lds, s, V, W, rcap, rep,
                     score, status);
  if (int rc = check_launch("cosine_medoid_pairs_kernel")) return rc;
  // nothing can be deferred when every cluster fits the LDS path by the caller's bounds
  if (info->max_cluster_spectra <= spx::CM_NCAP && info->max_cluster_peaks <= rcap) return SPX_SUCCESS;
  double* sc = score ? score : W.score;
  const unsigned gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>(C, 32));
  if (int rc = SPX_LAUNCH(cosine_medoid_rows_kernel, dim3(64, gy), dim3(spx::CM_BLOCK), s, V, W, sc)) return rc;
  const unsigned g4 = (unsigned)std::max<int64_t>(1, std::min<int64_t>((C + spx::CM_BLOCK - 1) / spx::CM_BLOCK, 1024));
  return SPX_LAUNCH(cosine_medoid_argmax_kernel, dim3(g4), dim3(spx::CM_BLOCK), s, V, W, sc, rep, status);
}

// ------------------------------------------------- explained b/y intensity
int spx_by_fraction(const double* mz, const double* inten, int64_t n_peaks, const int64_t* seg_begin,
                    const int64_t* seg_end, int64_t n_segments, const double* prec_mz, const int32_t* charge,
                    const uint8_t* seq, const int64_t* seq_off, const spx_by_params* params, double* fraction,
                    int32_t* status, void* stream) {
  static_assert(sizeof(spx::ByParams) == sizeof(spx_by_params), "ByParams mirrors spx_by_params");
  if (n_peaks < 0 || n_segments < 0) return fail(SPX_EINVAL, "spx_by_fraction: negative size");
  if (!params || (n_peaks > 0 && (!mz || !inten)) ||
      (n_segments > 0 && (!seg_begin || !seg_end || !prec_mz || !charge || !seq || !seq_off || !fraction || !status)))
    return fail(SPX_EINVAL, "spx_by_fraction: null argument");
  if (n_segments == 0) return SPX_SUCCESS;
  const int64_t blocks = (n_segments + spx::BY_WAVES - 1) / spx::BY_WAVES;
  if (blocks > INT32_MAX) return fail(SPX_EINVAL, "spx_by_fraction: too many segments");
  spx::ByParams P;
  std::memcpy(&P, params, sizeof(P));
  return SPX_LAUNCH(by_fraction_kernel, dim3((unsigned)blocks), dim3(spx::BY_WAVES * spx::kWave),
                    reinterpret_cast<hipStream_t>(stream), mz, inten, n_peaks, seg_begin, seg_end, n_segments, prec_mz,
                    charge, seq, seq_off, P, fraction, status);
}

// --------------------------------------------------------- best spectrum
int spx_best_score(const spx_csr* csr, const double* score, const int64_t* rank, int64_t* best, int32_t* status,
                   void* stream) {
  if (!csr || csr->n_clusters < 0 || !csr->cluster_off || !best || !status ||
      (csr->n_spectra > 0 && (!score || !rank)))
    return fail(SPX_EINVAL, "spx_best_score: null argument");
  const int64_t C = csr->n_clusters;
  if (C == 0) return SPX_SUCCESS;
  const int64_t blocks = (C + spx::BEST_WAVES - 1) / spx::BEST_WAVES;
  if (blocks > INT32_MAX) return fail(SPX_EINVAL, "spx_best_score: too many clusters");
  return SPX_LAUNCH(best_score_kernel, dim3((unsigned)blocks), dim3(spx::BEST_WAVES * spx::kWave),
                    reinterpret_cast<hipStream_t>(stream), C, csr->cluster_off, score, rank, best, status);
}

}  // extern "C"

// ---------------------------------------------------------------- compaction
namespace spx {
__global__ __launch_bounds__(256) void compact_kernel(CsrView v, const double* __restrict__ smz,
                                                      const double* __restrict__ sint, const int64_t* __restrict__ count,
                                                      const int64_t* __restrict__ out_off, double* __restrict__ dmz,
                                                      double* __restrict__ dint) {
  for (int64_t c = blockIdx.x; c < v.n_clusters; c += gridDim.x) {
    const int64_t src = v.spec_off[v.cluster_off[c]], dst = out_off[c], n = count[c];
    for (int64_t k = threadIdx.x; k < n; k += 256) {
      dmz[dst + k] = smz[src + k];
      dint[dst + k] = sint[src + k];
    }
  }
}
}  // namespace spx

extern "C" {

int spx_compact_peaks(const spx_csr* csr, const spx_peaks_out* src, const int64_t* out_off, double* dst_mz,
                      double* dst_inten, void* stream) {
  if (!csr_ok(csr) || !src || !src->count || !out_off) return fail(SPX_EINVAL, "spx_compact_peaks: null argument");
  if (csr->n_clusters == 0) return SPX_SUCCESS;
  const unsigned g = (unsigned)std::min<int64_t>(csr->n_clusters, 65535);
  return SPX_LAUNCH(compact_kernel, dim3(g), dim3(256), reinterpret_cast<hipStream_t>(stream), view(csr), src->mz,
                    src->inten, src->count, out_off, dst_mz, dst_inten);
}

// ------------------------------------------------------------ gather wire format
int spx_wire_pack(const double* mz, const double* inten, int64_t n, int32_t max_count, float* mi, void* count,
                  int32_t count_bytes, int32_t* n_fail, void* stream) {
  if (n < 0 || (n > 0 && (!mz || !inten || !mi || !count || !n_fail)))
    return fail(SPX_EINVAL, "spx_wire_pack: null argument");
  if (!(count_bytes == 1 || count_bytes == 2) || max_count < 1 || max_count > (count_bytes == 1 ? 255 : 65535))
    return fail(SPX_EINVAL, "spx_wire_pack: count_bytes must be 1 (max_count <= 255) or 2 (<= 65535)");
  if (n == 0) return SPX_SUCCESS;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float2* o = reinterpret_cast<float2*>(mi);
  if (count_bytes == 1)
    return SPX_LAUNCH(wire_pack_kernel<uint8_t>, dim3(wire_grid(n)), dim3(256), s, mz, inten, n, (uint32_t)max_count, o,
                      static_cast<uint8_t*>(count), n_fail);
  return SPX_LAUNCH(wire_pack_kernel<uint16_t>, dim3(wire_grid(n)), dim3(256), s, mz, inten, n, (uint32_t)max_count, o,
                    static_cast<uint16_t*>(count), n_fail);
}

int spx_wire_unpack(const float* mi, const void* count, int32_t count_bytes, int64_t n, double* mz, double* inten,
                    void* stream) {
  if (n < 0 || (n > 0 && (!mz || !inten || !mi || !count))) return fail(SPX_EINVAL, "spx_wire_unpack: null argument");
  if (!(count_bytes == 1 || count_bytes == 2)) return fail(SPX_EINVAL, "spx_wire_unpack: count_bytes must be 1 or 2");
  if (n == 0) return SPX_SUCCESS;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float2* v = reinterpret_cast<const float2*>(mi);
  if (count_bytes == 1)
    return SPX_LAUNCH(wire_unpack_kernel<uint8_t>, dim3(wire_grid(n)), dim3(256), s, v,
                      static_cast<const uint8_t*>(count), n, mz, inten);
  return SPX_LAUNCH(wire_unpack_kernel<uint16_t>, dim3(wire_grid(n)), dim3(256), s, v,
                    static_cast<const uint16_t*>(count), n, mz, inten);
}

// ------------------------------------------------------------ host transfers
int spx_copy_h2d(void* dst_device, const void* src_host, size_t nbytes, void* stream) {
  if (nbytes == 0) return SPX_SUCCESS;
  if (!dst_device || !src_host) return fail(SPX_EINVAL, "spx_copy_h2d: null pointer");
  const hipError_t e = spx::staged_copy(static_cast<char*>(dst_device), static_cast<const char*>(src_host), nbytes,
                                        reinterpret_cast<hipStream_t>(stream), true);
  if (e != hipSuccess) {
    std::snprintf(g_err, sizeof(g_err), "spx_copy_h2d: %s", hipGetErrorString(e));
    return SPX_EHIP;
  }
  return SPX_SUCCESS;
}

int spx_copy_d2h(void* dst_host, const void* src_device, size_t nbytes, void* stream) {
  if (nbytes == 0) return SPX_SUCCESS;
  if (!dst_host || !src_device) return fail(SPX_EINVAL, "spx_copy_d2h: null pointer");
  const hipError_t e = spx::staged_copy(static_cast<char*>(dst_host), static_cast<const char*>(src_device), nbytes,
                                        reinterpret_cast<hipStream_t>(stream), false);
  if (e != hipSuccess) {
    std::snprintf(g_err, sizeof(g_err), "spx_copy_d2h: %s", hipGetErrorString(e));
    return SPX_EHIP;
  }
  return SPX_SUCCESS;
}

// ------------------------------------------------------------ device-side MGF ingest
int spx_parse_mgf_text(const void* text, int64_t text_len, const int64_t* rec_begin, const int64_t* rec_end,
                       const int64_t* spec_off, int64_t n_records, int64_t n_peaks, int32_t general, double* mz,
                       double* inten, double* prec_mz, int32_t* charge, double* rt, int32_t* flags,
                       int32_t* rec_status, void* stream) {
  if (text_len < 0 || n_records < 0 || n_peaks < 0) return fail(SPX_EINVAL, "spx_parse_mgf_text: negative size");
  if (general != 0 && general != 1) return fail(SPX_EINVAL, "spx_parse_mgf_text: general must be 0 or 1");
  if ((text_len > 0 && !text) || (n_peaks > 0 && (!mz || !inten)))
    return fail(SPX_EINVAL, "spx_parse_mgf_text: null text or peak array");
  if (n_records > 0 && (!rec_begin || !rec_end || !spec_off || !prec_mz || !charge || !rt || !flags || !rec_status))
    return fail(SPX_EINVAL, "spx_parse_mgf_text: null record array");
  if (n_records == 0) return SPX_SUCCESS;
  const unsigned grid = (unsigned)std::min<int64_t>(n_records, int64_t(1) << 20);
  return SPX_LAUNCH(mgf_parse_kernel, dim3(grid), dim3(spx::kMgfBlock), reinterpret_cast<hipStream_t>(stream),
                    static_cast<const uint8_t*>(text), text_len, rec_begin, rec_end, spec_off, n_records, n_peaks,
                    (int)general, mz, inten, prec_mz, charge, rt, flags, rec_status);
}

// ------------------------------------------------------------ device-side MGF emit
size_t spx_format_peaks_workspace_size(int64_t n_segments, int64_t n_peaks) {
  if (n_segments < 0 || n_peaks < 0) return 0;
  Carver w{nullptr, 0};
  carve_format(w, n_segments);
  return w.used;
}

int spx_format_peaks(const double* mz, const double* inten, int64_t n_peaks, const int64_t* seg_begin,
                     const int64_t* seg_end, int64_t n_segments, int32_t skip_nan_inten, uint8_t* text,
                     int64_t text_capacity, int64_t* text_off, int32_t* flags, void* workspace, size_t workspace_bytes,
                     void* stream) {
  if (n_peaks < 0 || n_segments < 0 || text_capacity < 0) return fail(SPX_EINVAL, "spx_format_peaks: negative size");
  if ((n_peaks > 0 && (!mz || !inten)) || (n_segments > 0 && (!seg_begin || !seg_end)) || !text_off || !flags ||
      (text_capacity > 0 && !text))
    return fail(SPX_EINVAL, "spx_format_peaks: null argument");
  if (!workspace || workspace_bytes < spx_format_peaks_workspace_size(n_segments, n_peaks))
    return fail(SPX_EINVAL, "spx_format_peaks: workspace smaller than spx_format_peaks_workspace_size");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t S = n_segments;
  if (S == 0) {
    if (hipMemsetAsync(text_off, 0, sizeof(int64_t), s) != hipSuccess) return check_launch("spx_format_peaks memset");
    return SPX_SUCCESS;
  }
  Carver w{static_cast<char*>(workspace), 0};
  const FormatWs W = carve_format(w, S);
  const dim3 blk(spx::kFmtBlock);
  const dim3 gseg((unsigned)std::min<int64_t>((S + spx::kFmtBlock - 1) / spx::kFmtBlock, spx::kFmtSegGrid));
  // the peaks covered are known on the device only: the grid follows the array's size
  const dim3 gpk((unsigned)std::max<int64_t>(
      1, std::min<int64_t>((n_peaks + 2 * spx::kFmtBlock - 1) / (2 * spx::kFmtBlock), spx::kFmtPeakGrid)));
  int rc = SPX_LAUNCH(fmt_seg_sum_kernel, gseg, blk, s, seg_begin, seg_end, S, n_peaks, W.seg_part, flags);
  if (!rc) rc = SPX_LAUNCH(fmt_seg_scan_kernel, gseg, blk, s, seg_begin, seg_end, S, n_peaks, W.seg_part, W.voff);
  if (!rc) rc = SPX_LAUNCH(fmt_peaks_kernel<false>, gpk, blk, s, mz, inten, seg_begin, W.voff, S, skip_nan_inten, text,
                           text_capacity, text_off, flags, W.text_part);
  if (!rc) rc = SPX_LAUNCH(fmt_peaks_kernel<true>, gpk, blk, s, mz, inten, seg_begin, W.voff, S, skip_nan_inten, text,
                           text_capacity, text_off, flags, W.text_part);
  if (!rc) rc = SPX_LAUNCH(fmt_seg_fix_kernel, gseg, blk, s, W.voff, S, text_off);
  return rc;
}

// ------------------------------------------------------------ host side of the emit
int spx_repr_f64(double x, char* out) {
  if (!out) return fail(SPX_EINVAL, "spx_repr_f64: null buffer");
  return spx_repr::repr_f64(x, out);
}

int spx_mgf_splice_records(const char* path, int32_t append, int32_t style, int64_t n_records, const char* titles,
                           const int32_t* flags, const double* prec, const int64_t* charge, const double* rt,
                           const int64_t* text_off, const uint8_t* text, int32_t threads) {
  if (spx_splice::write_records(path, append, style, n_records, titles, flags, prec, charge, rt, text_off, text,
                                threads) != 0)
    return fail(SPX_EINVAL, "spx_mgf_splice_records: bad argument or I/O error");
  return SPX_SUCCESS;
}

}  // extern "C"
