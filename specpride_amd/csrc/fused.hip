// One pass of the headline step over a cluster: bin-mean consensus AND medoid
// representative (SURVEY.md §8(d) configs[4]: "medoid + binned consensus").
//
// The two register kernels run back to back inside ONE workgroup per cluster:
// bin_mean_reg_path (bin_mean.hip; binning.py:170-231), then medoid_small_body
// (medoid.hip; most_similar_representative.py:13-19, :60-111) over the same
// cluster, their LDS states overlaid (they never live at once).  The bodies and
// their hand-off lists are the separate kernels' own, so every result is
// bit-identical to spx_bin_mean + spx_medoid.
//
// Why fuse: bin-mean streams 16 B per peak and is bound by the traffic it issues;
// the medoid reads 8 B per peak and spends most of its lifetime in LDS-bound
// latency chains (rows, pairs, pairwise sums).  As two kernels, each fills the
// chip alone.  Fused, one CU holds workgroups in both kinds of phases at once.
// Since round 6 the pass reads each m/z ONCE for both methods: the bin-mean's phase
// A computes the medoid's ceil(mz/tol) bin beside its own from the same load and
// phase B ranks it, so the medoid's bit rows come from registers (medoid_from_codes)
// and its own m/z pass, offsets search and flat-layout bookkeeping are gone for every
// cluster the register path completes.
//
// The kernel is persistent: the grid is the device's resident workgroups, and each
// walks the clusters it claims from a queue head (one returning atomicAdd per cluster;
// the loop ends at the first claim >= C, and no workgroup ever waits on another, so
// the grid size is a tuning value only).  While a cluster's medoid runs -- the part of
// a lifetime that issues no global load of its own -- the workgroup's last wave claims
// the next cluster and fetches its header (offsets, charges, precursors: RegHeader,
// bin_mean.hip) into the other of two LDS buffers -- the claim during the medoid's rows,
// the dependent loads beside the waves that finish the medoid's tail -- so the next
// set-up reads LDS and waits for no round trip (FusedPrefetch).
#include "bin_mean.hip"
#include "medoid.hip"

namespace spx {

#ifndef SPX_FU_MINW
#define SPX_FU_MINW 5  // waves per SIMD: the bin-mean body's 96 VGPRs
#endif
#ifndef SPX_FU_STATIC
#define SPX_FU_STATIC 0  // 1: cluster blockIdx.x + k * gridDim.x instead of the queue (A/B: DESIGN.md)
#endif

union FusedSmem {
  BinHeadSmem b;
  MedoidRegSmem<MD_BLOCK, MR_UMAX, MD_KWMAX> m;
};
static_assert(BM_BLOCK == MD_BLOCK, "one workgroup shape for both bodies");

// The next cluster's header, fetched by ONE wave (all 64 lanes active) in four steps at
// wave-uniform program points: the claim goes out a phase ahead (the medoid's rows), the
// other three run back to back in the medoid's tail -- at once in a cluster of up to 32
// spectra, where this wave has no other work, and after its Gram tile past 32 -- and the
// wave waits for each step's loads itself:
//   claim    the queue head's atomicAdd                       -> tc
//   offsets  tc -> H->c; cluster_off[c], cluster_off[c + 1]   -> toff
//   spectra  toff -> H->s0, H->n; spec_off, charge, prec_mz   -> tso, tz, tp
//   commit   those -> H->p0, p1, rel[], charge[], prec[]
// The staged values live in registers only between two steps, all inside the medoid
// (whose register need is far below phase A's and C's); what a later step needs to know
// of an earlier one (the cluster, its spectra) it reads back from the header.  One object
// serves one cluster (a longer-lived one would carry its staged values, which not every
// path sets, through phases A-D of the next cluster: 8 VGPRs).  all() runs the four back to back,
// waiting for each: the kernel's first cluster, and after a cluster whose medoid did not
// take the stepped path (medoid_small_body, n <= 1, a deferral).
struct FusedPrefetch {
  uint32_t tc;
  int64_t toff, tso;
  int32_t tz;
  double tp;

  // `head`: the queue (BmCounter::kBmcUnused of the bin-mean workspace, zeroed by the call)
  // `k`: the claims this workgroup has made (the static order's step)
  __device__ __forceinline__ void claim(uint32_t* head, uint32_t& k) {
    tc = 0u;
#if SPX_FU_STATIC
    tc = blockIdx.x + k * gridDim.x;
#else
    if (lane_id() == 0) tc = atomicAdd(head, 1u);
#endif
    ++k;
  }
  // H: the buffer being filled, never the one the current cluster reads
  __device__ __forceinline__ void offsets(const CsrView& v, RegHeader* H) {
    const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)tc);
    const int32_t cn = (int64_t)c < v.n_clusters ? (int32_t)c : -1;
    if (lane_id() == 0) H->c = cn;
    toff = 0;
    if (cn >= 0) toff = v.cluster_off[(int64_t)cn + (lane_id() != 0)];
  }
  __device__ __forceinline__ void spectra(const CsrView& v, RegHeader* H) {
    if (__builtin_amdgcn_readfirstlane(H->c) < 0) return;
    const int64_t s0 = readlane64(toff, 0);
    const int64_t n64 = readlane64(toff, 1) - s0;
    const int32_t n = n64 >= 1 && n64 <= BR_NMAX ? (int32_t)n64 : BR_NMAX + 1;
    if (lane_id() == 0) {
      H->s0 = s0;
      H->n = n;
    }
    if (n > BR_NMAX) return;
    // lane j <= n: spectrum j's first peak (lane n: the cluster's end); lanes past n repeat it
    const int j = lane_id() < n ? lane_id() : n, jj = lane_id() < n ? lane_id() : n - 1;
    tso = v.spec_off[s0 + j];
    tz = v.charge[s0 + jj];
    tp = v.prec_mz[s0 + jj];
  }
  __device__ __forceinline__ void commit(RegHeader* H) {
    if (__builtin_amdgcn_readfirstlane(H->c) < 0) return;
    const int n = __builtin_amdgcn_readfirstlane(H->n);
    if (n > BR_NMAX) return;
    const int lane = lane_id();
    const int64_t p0 = readlane64(tso, 0);
    if (lane == 0) H->p0 = p0;
    if (lane == n) H->p1 = tso;
    if (lane <= n) H->rel[lane] = (int32_t)(tso - p0);  // (p1 - p0 >= 2^28: the set-up leaves before reading it)
    if (lane < n) {
      H->charge[lane] = tz;
      H->prec[lane] = tp;
    }
  }
  __device__ __forceinline__ void all(const CsrView& v, uint32_t* head, uint32_t& k, RegHeader* H) {
    claim(head, k);
    offsets(v, H);
    spectra(v, H);
    commit(H);
  }
};

// wave 3 prefetches: it owns peaks 189..251 of every spectrum, the fewest
__device__ __forceinline__ bool fused_prefetch_wave() {
  return __builtin_amdgcn_readfirstlane(wave_id()) == BM_BLOCK / kWave - 1;
}

// The medoid of a cluster the fused register path has binned (bin_mean_reg_path_t<true>
// returned kOk with every medoid bin inside [0, 32,768)): the codes hold this lane's
// peak of spectrum j -- peak 63 * wave + lane, lanes 0..62 own one each -- as its
// medoid column (the rank of ceil(mz/tol) among the cluster's occupied medoid bins),
// two spectra's columns per register after phase C.  P3 sets each spectrum's bit row straight from those registers
// (the spectrum of a peak is its step j: no offsets search), then medoid_tail runs
// P4..P6 exactly as medoid_small_body does, so rep and totals are the same bits
// (most_similar_representative.py:13-19, :60-111).  K > 64 * MD_KWMAX columns hands the
// cluster on as the register kernel would.
// The prefetching wave steps `pf` through the next cluster's header `Hn` between the
// phases.  Returns whether it did (false: a cluster that left early, the caller runs
// pf.all()).  The spectrum offsets, s0 and n come from the cluster's header `hd` again.
template <class Defer>
__device__ __forceinline__ bool medoid_from_codes(int64_t* rep, double* totals_out,
                                                  MedoidRegSmem<MD_BLOCK, MR_UMAX, MD_KWMAX>& L, int64_t c,
                                                  const int32_t (&code)[BR_NMAX], const MdSide& md,
                                                  const Defer& defer, const RegHeader& hd, FusedPrefetch& pf,
                                                  const CsrView& v, uint32_t* head, uint32_t& k, RegHeader* Hn) {
  const int tid = threadIdx.x, lane = lane_id(), wid = wave_id();
  const int64_t s0 = hd.s0;
  const int n = __builtin_amdgcn_readfirstlane(hd.n);
  if (n <= 1) {
    if (tid == 0) {
      rep[c] = n == 1 ? s0 : -1;
      if (totals_out && n == 1) totals_out[s0] = 0.0;
    }
    return false;
  }
  const int KW = ((md.K + 63) / 64) | 1;  // odd row stride, as medoid_small_body's
  if (KW > MD_KWMAX) {
    if (tid == 0) defer(c, s0, n);
    return false;
  }
  // lane j <= n: spectrum j's first peak relative to the cluster's first (lane n, and
  // every lane past it: the cluster's end)
  const int32_t rel = hd.rel[lane < n ? lane : n];
  // spectrum offsets (lane j < n: spectrum j's start; lane n: spectrum n-1's end)
  if (tid <= n) L.soff[tid] = rel;
  for (int w = tid; w < n * KW; w += MD_BLOCK) L.u.a.rows[w] = 0ull;
  __syncthreads();
  // the claim goes out right AFTER a full barrier (which waits for the wave's outstanding
  // loads) and has P3 to land; the other steps follow the barrier that opens the tail
  if (fused_prefetch_wave()) pf.claim(head, k);
  const uint32_t swz_nw = 2u * (uint32_t)KW;  // 32-bit words per row
  const uint32_t swz_m = swz_nw >= 32u ? 31u : (1u << (31 - __clz((int)swz_nw))) - 1u;  // 2^k - 1 < swz_nw
  const int fpos = wid * (kWave - 1) + lane;
  const bool owner = lane < kWave - 1;
  int ea = __builtin_amdgcn_readlane(rel, 0);  // spectrum j's first peak, carried from step to step
  const int kw8 = __builtin_amdgcn_readfirstlane(8 * KW);  // bytes per row, uniform
  reg_steps(n, [&](auto jc) __attribute__((always_inline)) {
    constexpr int j = decltype(jc)::value;
    const int a = ea;
    ea = __builtin_amdgcn_readlane(rel, j + 1);
    const int len = ea - a;
    // the row's byte offset is uniform: pinned to a scalar register it joins the address in
    // one shift-add (left to the compiler it became a constant move and a 24-bit mad)
    int row = j * kw8;
    asm volatile("" : "+s"(row));
    if (owner & (fpos < len)) {
      // phase C packed the columns of spectra 2k, 2k+1 into code[2k] (low, high half);
      // a last even spectrum (n odd) keeps its (slot, column) code
      uint32_t col;
      if constexpr (j & 1) col = (uint32_t)code[j - 1] >> 16;
      else col = j + 1 < n ? (uint32_t)code[j] & 0xFFFFu : (uint32_t)code[j] >> 16;
      // the register kernel's P3 word swizzle (a bijection per bit position)
      uint32_t wq = (col >> 5) + (col & swz_m);
      wq = min(wq, wq - swz_nw);
      atomicOr(reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(L.u.a.rows) + row) + wq, 1u << (col & 31));
    }
  });
  SPX_STAMP2(-1, 5);
  // up to 32 spectra the tail's work is wave 0's: the prefetching wave runs the remaining
  // steps on its own beside it, back to back, waiting for each step's loads.  Past 32 it has
  // a Gram tile of its own first and runs the steps behind the tail's hand-off barrier,
  // beside the two finishing waves (medoid_tail_regs calls the hook there) --
  // before the tail's last barrier in every case (Hn lies outside the medoid's LDS, and
  // the loop-top barrier publishes it)
  medoid_tail<MD_BLOCK, MR_UMAX, MD_KWMAX>(L, n, KW, s0, c, rep, totals_out,
                                           [&]() __attribute__((always_inline)) {
    if (!fused_prefetch_wave()) return;
    pf.offsets(v, Hn);
    pf.spectra(v, Hn);
    pf.commit(Hn);
  });
  return true;
}

// The kernel's arguments as one struct: the persistent loop re-reads what it needs from
// the kernel-argument segment in every iteration (scalar loads through a pointer the
// compiler cannot see through) instead of holding every argument in an SGPR across the
// whole loop, which spilled SGPRs into VGPR lanes and VGPRs into scratch.
// `queue`: the head the workgroups claim their clusters from, 0 at launch.
struct FusedArgs {
  CsrView v;
  BinMeanParams PB;
  PeaksOut out;
  double* prec_out;
  int32_t* charge_out;
  int32_t* status;
  StripedList bm_rest;
  MedoidParams PM;
  int64_t* rep;
  double* totals_out;
  StripedList md_wide;
  uint32_t* queue;
};

__global__ __launch_bounds__(BM_BLOCK, SPX_FU_MINW) void bin_mean_medoid_kernel(FusedArgs) {
  __shared__ FusedSmem L;
  __shared__ RegHeader H[2];  // the current cluster's header and the next one's
  // the one argument sits at the start of the kernel-argument segment
  using ArgsPtr = const FusedArgs __attribute__((address_space(4)))*;
  ArgsPtr ap = (ArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
  uint32_t k = 0u;  // clusters claimed
  if (fused_prefetch_wave()) {
    FusedPrefetch pf{};
    pf.all(((const FusedArgs*)ap)->v, ((const FusedArgs*)ap)->queue, k, &H[0]);
  }
  int cur = 0;
  // The cluster loop is written with a second entry that is never taken (`never` is 0,
  // which the compiler cannot know).  With two entries the cycle is no natural loop, so the
  // optimiser does not hoist the bodies' per-thread index arithmetic (LDS addresses, MFMA
  // fragment coordinates, step offsets: hundreds of values) in front of it, where they would
  // stay live across every phase: as a plain loop the kernel spilled 150 SGPRs and 300 VGPRs;
  // like this each phase computes its indices where it uses them, as the one-cluster kernel did.
  int never = 0;
  asm volatile("" : "+s"(never));
  if (never) {
    // (entered from a block of its own: with two outside predecessors the cycle has no
    // preheader for the machine-level hoisting either)
    asm volatile("" : "+s"(never));
    goto next_cluster;
  }
cluster : {
  asm volatile("" : "+s"(ap));  // this cluster's argument reads start here
  const FusedArgs& A = *(const FusedArgs*)ap;
  const RegHeader& hd = H[cur];
  RegHeader* Hn = &H[cur ^ 1];
  lds_barrier();  // the header is complete (and the medoid before it has read its last LDS word)
  const int32_t c32 = __builtin_amdgcn_readfirstlane(hd.c);
  if (c32 < 0) return;  // the claim was >= C: nothing left (uniform)
  const int64_t c = c32;
  SPX_STAMP2(-1, 0);
  auto defer = [&](int64_t cc, int64_t, int) {
    A.rep[cc] = -4;  // medoid_reg_kernel's hand-off, verbatim
    striped_push(A.md_wide, (int32_t)cc);
  };
  // bin-mean first: its phase A reads each m/z once for BOTH methods' bins
  int32_t code[BR_NMAX];
  MdSide md{A.PM.tol, A.PM.inv_tol, 1, 0};
  const int32_t st = bin_mean_reg_path_t<true>(A.v, A.PB, L.b, c, A.out, A.prec_out, A.charge_out, code, &md, &hd);
  if (threadIdx.x == 0) {  // bin_mean_reg_kernel's hand-off, verbatim
    if (st != kNotHere) A.status[c] = st;
    if (st == kNotHere || st == kDeferred) striped_push(A.bm_rest, (int32_t)c);
  }
  SPX_STAMP2(-1, 4);
  __syncthreads();  // the bin-mean LDS is dead: the medoid's takes its place
  FusedPrefetch pf{};
  bool fetched = false;
  if (st == kOk && !md.out) {  // uniform
    fetched = medoid_from_codes(A.rep, A.totals_out, L.m, c, code, md, defer, hd, pf, A.v, A.queue, k, Hn);
  } else {
    // the register path stopped before its codes were complete (more than 50 spectra,
    // a long / unsorted / NaN spectrum, mixed charges, > 1,536 bins) or a medoid bin is
    // out of its range: the medoid's own body, which reads the m/z itself
    medoid_small_body<MD_BLOCK, MR_UMAX, MD_KWMAX>(A.v, A.PM, A.rep, A.totals_out, L.m, c, defer);
  }
  if (!fetched && fused_prefetch_wave()) pf.all(A.v, A.queue, k, Hn);
}
next_cluster:
  cur ^= 1;
  goto cluster;
}

// The hand-off counts of one fused pass (spx_bin_mean_medoid_stage, stage 1): the
// clusters each register body left on its list -- out[0] bin-mean (for
// bin_mean_wide_kernel), out[1] medoid (for medoid_wide_kernel).  Both zero: the
// leftover chains (stage 2) have nothing to do for this batch.
__global__ __launch_bounds__(kWave) void handoff_count_kernel(const int32_t* bm_counts, const int32_t* md_counts,
                                                              int32_t* out) {
  const int l = threadIdx.x;
  const int32_t a = wave_sum(bm_counts[l * kListLine]);
  const int32_t b = wave_sum(md_counts[l * kListLine]);
  if (l == 0) {
    out[0] = a;
    out[1] = b;
  }
}

}  // namespace spx
