// Cosine medoid: per cluster, the member with the highest average binned cosine to
// the cluster's members, itself included (reference: src/benchmark.py:19-38,
// cos_dist / average_cos_dist, every member taken as the representative in turn;
// restated in oracle/np_oracle.py, composed in tests/cosine_medoid_cases.py).
//
//   score[i] = (sum_j cos_dist(member_i, member_j), j = 0..n-1 in order) / n
//   rep      = the first i with the maximal score (replaced only on >)
//
// Every pair keeps cos_dist's own rules (binned_cosine.hip): the cut at
// max(last m/z of the two), numpy's DOUBLE_fill edges, scipy's on-edge shift into the
// last bin, sums per bin in input order, 0.0 if either norm is 0.
//
// Stage 1, cosine_medoid_bin_kernel (one wave per spectrum): unbounded bin indices,
// a stable rank sort by (bin, input index) -- skipped when the bins are already
// non-decreasing --, runs of equal bins with A_b summed in input order, and per run
// E_b = the part of A_b whose peaks round onto the run's own left edge: under a cut
// whose last edge is that edge (kc + 1 == the run's bin) they are the pair's on-edge
// peaks.  cosine_medoid_prefix_kernel (one thread per spectrum) then writes the
// exclusive prefix of A_b^2 SEQUENTIALLY in bin order.  All of it lies in a workspace
// slice aligned with spec_off (there are never more runs than peaks).
//
// Stage 2, cosine_medoid_pairs_kernel (one workgroup per cluster of <= CM_NCAP
// members and <= the LDS run budget): the members' run bins and sums staged in LDS,
// one lane per unordered pair: the cut of each of the two (a backward scan for the
// runs past the cut, the norm from the prefix), then a two-pointer merge of the run
// lists in ascending bin order.  The merge order and the prefix order are the same
// and the products commute, so
//   * S(i, j) has the same bits whichever of the two comes first, and is evaluated
//     once per unordered pair;
//   * two members with equal peaks score exactly what a member scores against
//     itself (a / sqrt(a * a)), so duplicates tie bit for bit and the lower index
//     wins, as in the reference.
// Row sums are sequential over j, then one divide; the argmax is a sequential scan.
// Larger clusters go to cosine_medoid_rows_kernel (a wave per row over the global
// runs, the same pair body) and cosine_medoid_argmax_kernel.
// (included after binned_cosine.hip: CosParams, cs_bin, cs_edge, np_around, wave_lds_sync)
#include "spx_device.hpp"

namespace spx {

constexpr int CM_BLOCK = 256;       // stage 1, prefix, rows, argmax
// Stage 2's workgroup: the waves that share one cluster's LDS image.  A configs[1] batch
// sizes the image at ~140 KB, one workgroup per CU, so the workgroup's own waves are all
// that hides the merge's LDS latency: 100k clusters measured 66.9 ms at 256 threads,
// 50.1 at 512, 45.2 at 1,024 (the whole call).
#ifndef SPX_CM_PAIR_BLOCK
#define SPX_CM_PAIR_BLOCK 1024
#endif
constexpr int CM_PAIR_BLOCK = SPX_CM_PAIR_BLOCK;
constexpr int CM_NCAP = 64;         // members of a cluster on the LDS path
// Run budget of the LDS path: 12 B a run (bin + A_b) next to the 64-member pair
// triangle (16.6 KB) in the CU's 160 KiB.  The launch sizes its dynamic LDS from the
// batch's largest cluster, so ordinary batches take far less.
constexpr int CM_LDS_RUNS = 11264;
constexpr int CM_TRI = CM_NCAP * (CM_NCAP + 1) / 2;
constexpr int32_t CM_KINV = 0x7fffffff;  // a peak no cut keeps (below e_0, NaN): sorts last
constexpr int32_t CM_LMAX = 0x7ffffff0;  // edge counts and bins stay below this
enum : int32_t { kCmEmpty = 1, kCmBad = 2 };

struct CosMedWs {
  int32_t* rb;    // [P] run bins, spectrum s at spec_off[s]
  double* rA;     // [P] A_b
  double* rE;     // [P] on-edge part of A_b
  double* rA2;    // [P] exclusive prefix of A_b^2; stage 1's (key, index) pairs before that
  int32_t* nr;    // [S] runs
  int32_t* L;     // [S] len(np.arange(-s/2, last m/z, s))
  int32_t* nE;    // [S] runs with E_b != 0
  int32_t* flag;  // [S] kCmEmpty | kCmBad
  double* tot2;   // [S] sum of A_b^2
  double* score;  // [S] scores of the deferred clusters when the caller passes none
  int32_t* n_def; // clusters past the LDS path, and
  int32_t* def;   // [C] their list
};

__host__ __device__ inline size_t cm_lds_bytes(int rcap) {
  return (size_t)8 * (CM_TRI + rcap + CM_NCAP) + (size_t)4 * (rcap + 3 * CM_NCAP + 1);
}

// global memory written by some lanes of this wave, read by others
__device__ __forceinline__ void wave_gsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ __launch_bounds__(CM_BLOCK) void cosine_medoid_bin_kernel(CsrView v, CosParams P, CosMedWs W) {
  const int lane = lane_id();
  const int64_t nwaves = (int64_t)gridDim.x * (CM_BLOCK / kWave);
  const double xlim = cs_edge(P, CM_LMAX);
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  int2* kp = reinterpret_cast<int2*>(W.rA2);  // (bin, sorted input index) per peak
  for (int64_t s = (int64_t)blockIdx.x * (CM_BLOCK / kWave) + wave_id(); s < v.n_spectra; s += nwaves) {
    const int64_t a = v.spec_off[s], e = v.spec_off[s + 1];
    const int64_t m64 = e - a;
    if (m64 <= 0 || m64 > CM_LMAX) {
      if (lane == 0) {
        W.nr[s] = 0; W.L[s] = 0; W.nE[s] = 0;
        W.flag[s] = m64 <= 0 ? kCmEmpty : kCmBad;
      }
      continue;
    }
    const int m = (int)m64;
    bool bad = false, uns = false;
    int32_t carry = -1;
    int nv = 0;  // peaks some cut can keep
    for (int ch = 0; ch < m; ch += kWave) {
      const int q = ch + lane;
      const bool in = q < m;
      int32_t key = CM_KINV;
      if (in) {
        const double x = v.mz[a + q];
        if (x >= P.start) {
          if (x < xlim) key = (int32_t)cs_bin(P, x);
          else bad = true;
        }
      }
      int32_t prev = __shfl_up(key, 1, kWave);
      if (lane == 0) prev = carry;
      uns |= in && key < prev;
      nv += __popcll(__ballot(in && key != CM_KINV));
      if (in) kp[a + q] = make_int2(key, q);
      carry = __shfl(key, kWave - 1, kWave);
    }
    const bool unsorted = __ballot(uns) != 0ull;
    const double Lf = ceil((v.mz[e - 1] - P.start) / P.s);  // len(np.arange(start, mz[-1], s))
    if (__ballot(bad) != 0ull || !(Lf >= 2.0 && Lf <= (double)CM_LMAX)) {
      if (lane == 0) { W.nr[s] = 0; W.L[s] = 0; W.nE[s] = 0; W.flag[s] = kCmBad; }
      continue;
    }
    wave_gsync();
    if (unsorted) {  // stable rank sort by (bin, index)
      for (int ch = 0; ch < m; ch += kWave) {
        const int q = ch + lane;
        const bool in = q < m;
        const int32_t key = in ? kp[a + q].x : 0;
        int rank = 0;
        for (int j = 0; j < m; ++j) {
          const int32_t kj = kp[a + j].x;
          rank += kj < key || (kj == key && j < q);
        }
        if (in) kp[a + rank].y = q;
      }
      wave_gsync();
    }
    // runs of equal bins: A_b and E_b summed in input order by the run's first lane
    int nruns = 0, nE = 0;
    bool nonfin = false;
    int32_t ck = -1;
    for (int ch = 0; ch < nv; ch += kWave) {
      const int r = ch + lane;
      const bool in = r < nv;
      int32_t key = -2;
      if (in) key = kp[a + (unsorted ? kp[a + r].y : r)].x;
      int32_t prev = __shfl_up(key, 1, kWave);
      if (lane == 0) prev = ck;
      const bool head = in && key != prev;
      const unsigned long long hm = __ballot(head);
      double E = 0.0;
      if (head) {
        const int id = nruns + __popcll(hm & ((1ull << lane) - 1ull));
        const double re = np_around(cs_edge(P, key), P.p10);
        double A = 0.0;  // np.bincount: out[bin] = 0.0, then += w in input order
        for (int t = r; t < nv; ++t) {
          const int it = unsorted ? kp[a + t].y : t;
          if (kp[a + it].x != key) break;
          const double I = v.inten[a + it];
          A += I;
          if (np_around(v.mz[a + it], P.p10) == re) E += I;
        }
        W.rb[a + id] = key;
        W.rA[a + id] = A;
        W.rE[a + id] = E;
        nonfin |= !(fabs(A) < inf) || !(fabs(E) < inf);
      }
      nE += __popcll(__ballot(head && E != 0.0));
      nruns += __popcll(hm);
      ck = __shfl(key, kWave - 1, kWave);
    }
    const bool any_nonfin = __ballot(nonfin) != 0ull;
    if (lane == 0) {
      W.nr[s] = nruns;
      W.L[s] = (int32_t)Lf;
      W.nE[s] = nE;
      W.flag[s] = any_nonfin ? kCmBad : 0;
    }
  }
}

// rA2[r] = A_0^2 + ... + A_{r-1}^2, added one by one in bin order: the order the pair
// merge adds its products in, so a spectrum's dot product with an equal one is its norm
__global__ __launch_bounds__(CM_BLOCK) void cosine_medoid_prefix_kernel(CsrView v, CosMedWs W) {
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  for (int64_t s = (int64_t)blockIdx.x * CM_BLOCK + threadIdx.x; s < v.n_spectra; s += (int64_t)gridDim.x * CM_BLOCK) {
    const int64_t a = v.spec_off[s];
    const int nr = W.nr[s];
    double acc = 0.0;
    for (int r = 0; r < nr; ++r) {
      const double A = W.rA[a + r];
      W.rA2[a + r] = acc;
      acc += A * A;
    }
    W.tot2[s] = acc;
    if (!(acc < inf)) W.flag[s] |= kCmBad;
  }
}

struct CmMember {
  const int32_t* rb;  // LDS or global
  const double* rA;
  const double* rA2;  // global
  const double* rE;
  int nr, L, nE;
  double tot2;
};

struct CmCut {
  int base;    // runs with a bin < kc
  double Akc;  // A'_{kc}: the run of bin kc plus the on-edge peaks of bin kc + 1
  double aa;   // the norm under the cut
};

__device__ __forceinline__ CmCut cm_cut(const CmMember& M, int32_t kc) {
  int ic = M.nr;  // runs with a bin <= kc
  while (ic > 0 && M.rb[ic - 1] > kc) --ic;
  const bool kc_run = ic > 0 && M.rb[ic - 1] == kc;
  const int base = kc_run ? ic - 1 : ic;
  double extra = 0.0;
  if (M.nE > 0 && ic < M.nr && M.rb[ic] == kc + 1) extra = M.rE[ic];
  const double pre = base < M.nr ? M.rA2[base] : M.tot2;
  const double Akc = (kc_run ? M.rA[ic - 1] : 0.0) + extra;
  return CmCut{base, Akc, pre + Akc * Akc};
}

// cos_dist of two members; the same bits for (X, Y) and (Y, X)
__device__ __forceinline__ double cm_pair(const CmMember& X, const CmMember& Y, bool self) {
  const int32_t kc = (X.L > Y.L ? X.L : Y.L) - 2;  // the last bin of np.arange(start, max_mz, s)
  const CmCut cx = cm_cut(X, kc);
  if (self) return cx.aa == 0.0 ? 0.0 : cx.aa / sqrt(cx.aa * cx.aa);
  const CmCut cy = cm_cut(Y, kc);
  // two-pointer merge in ascending bin order; the products are loaded every step (one
  // LDS round trip a step, no divergent branch) and added only where the bins match
  double ab = 0.0;
  for (int p = 0, q = 0; p < cx.base && q < cy.base;) {
    const int32_t bx = X.rb[p], by = Y.rb[q];
    const double sum = ab + X.rA[p] * Y.rA[q];
    ab = bx == by ? sum : ab;
    p += bx <= by;
    q += by <= bx;
  }
  ab += cx.Akc * cy.Akc;
  return (cx.aa == 0.0 || cy.aa == 0.0) ? 0.0 : ab / sqrt(cx.aa * cy.aa);
}

__device__ __forceinline__ CmMember cm_global_member(const CsrView& v, const CosMedWs& W, int64_t s) {
  const int64_t a = v.spec_off[s];
  return CmMember{W.rb + a, W.rA + a, W.rA2 + a, W.rE + a, W.nr[s], W.L[s], W.nE[s], W.tot2[s]};
}

// first pair of row i in the row-major upper triangle (diagonal included) of n members
__device__ __forceinline__ int cm_row_start(int i, int n) { return i * n - (i * (i - 1)) / 2; }

__global__ __launch_bounds__(CM_PAIR_BLOCK) void cosine_medoid_pairs_kernel(CsrView v, CosMedWs W, int rcap, int64_t* rep,
                                                                          double* score, int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) char cm_smem[];
  double* tri = reinterpret_cast<double*>(cm_smem);  // S(i, j), i <= j
  double* lA = tri + CM_TRI;
  double* mtot = lA + rcap;
  int32_t* lb = reinterpret_cast<int32_t*>(mtot + CM_NCAP);
  int32_t* moff = lb + rcap;  // [CM_NCAP + 1]
  int32_t* mL = moff + CM_NCAP + 1;
  int32_t* mnE = mL + CM_NCAP;
  const int tid = threadIdx.x, lane = lane_id(), wid = wave_id();
  const int64_t c = blockIdx.x;
  const int64_t s0 = v.cluster_off[c], s1 = v.cluster_off[c + 1];
  const int64_t n64 = s1 - s0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (n64 <= 0) {
    if (tid == 0) { rep[c] = -1; status[c] = kOk; }
    return;
  }
  int f = 0;
  for (int64_t j = tid; j < n64; j += CM_PAIR_BLOCK) f |= W.flag[s0 + j];
  const bool empty = __syncthreads_or(f & kCmEmpty);
  const bool bad = __syncthreads_or(f & kCmBad);
  if (empty || bad) {  // an empty member: the reference's mz[-1] raises IndexError
    if (score)
      for (int64_t j = tid; j < n64; j += CM_PAIR_BLOCK) score[s0 + j] = nan;
    if (tid == 0) { rep[c] = -1; status[c] = empty ? kEmpty : kDeferred; }
    return;
  }
  bool defer = n64 > CM_NCAP;
  const int n = defer ? 0 : (int)n64;
  if (tid < n) {
    moff[tid + 1] = W.nr[s0 + tid];
    mL[tid] = W.L[s0 + tid];
    mnE[tid] = W.nE[s0 + tid];
    mtot[tid] = W.tot2[s0 + tid];
  }
  __syncthreads();
  if (tid == 0) {
    moff[0] = 0;
    int64_t tot = 0;
    for (int i = 0; i < n; ++i) {
      tot += moff[i + 1];
      moff[i + 1] = tot > rcap ? rcap + 1 : (int32_t)tot;
    }
  }
  __syncthreads();
  defer = defer || moff[n] > rcap;
  if (defer) {
    if (tid == 0) {
      status[c] = kDeferred;
      rep[c] = -1;
      W.def[atomicAdd(W.n_def, 1)] = (int32_t)c;
    }
    return;
  }
  for (int mI = wid; mI < n; mI += CM_PAIR_BLOCK / kWave) {
    const int64_t a = v.spec_off[s0 + mI];
    const int o = moff[mI], nr = moff[mI + 1] - o;
    for (int r = lane; r < nr; r += kWave) {
      lb[o + r] = W.rb[a + r];
      lA[o + r] = W.rA[a + r];
    }
  }
  __syncthreads();
  const int npairs = n * (n + 1) / 2;
  for (int t = tid; t < npairs; t += CM_PAIR_BLOCK) {
    const float b = (float)(2 * n + 1);
    int i = (int)((b - sqrtf(b * b - 8.0f * (float)t)) * 0.5f);
    i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    while (i + 1 < n && cm_row_start(i + 1, n) <= t) ++i;
    while (cm_row_start(i, n) > t) --i;
    const int j = i + (t - cm_row_start(i, n));
    const int64_t ai = v.spec_off[s0 + i], aj = v.spec_off[s0 + j];
    const CmMember X{lb + moff[i], lA + moff[i], W.rA2 + ai, W.rE + ai, moff[i + 1] - moff[i], mL[i], mnE[i], mtot[i]};
    const CmMember Y{lb + moff[j], lA + moff[j], W.rA2 + aj, W.rE + aj, moff[j + 1] - moff[j], mL[j], mnE[j], mtot[j]};
    tri[t] = cm_pair(X, Y, i == j);
  }
  __syncthreads();
  if (tid < n) {  // average_cos_dist: the sequential sum over the members in order, one divide
    double sum = 0.0;
    for (int j = 0; j < n; ++j) {
      const int lo = tid < j ? tid : j, hi = tid < j ? j : tid;
      sum += tri[cm_row_start(lo, n) + hi - lo];
    }
    sum /= (double)n;
    if (score) score[s0 + tid] = sum;
    mtot[tid] = sum;
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    for (int i = 1; i < n; ++i)
      if (mtot[i] > mtot[best]) best = i;
    rep[c] = s0 + best;
    status[c] = kOk;
  }
}

// Deferred clusters (more than CM_NCAP members, or more runs than the LDS image holds):
// a wave per row i over the runs in the workspace; the lanes take 64 partners at a
// time, lane 0 adds their cosines in member order.
__global__ __launch_bounds__(CM_BLOCK) void cosine_medoid_rows_kernel(CsrView v, CosMedWs W, double* score) {
  __shared__ double buf[CM_BLOCK / kWave][kWave];
  const int lane = lane_id(), wid = wave_id();
  const int32_t nd = *W.n_def;
  for (int32_t d = blockIdx.y; d < nd; d += gridDim.y) {
    const int64_t c = W.def[d];
    const int64_t s0 = v.cluster_off[c], n = v.cluster_off[c + 1] - s0;
    for (int64_t i = (int64_t)blockIdx.x * (CM_BLOCK / kWave) + wid; i < n;
         i += (int64_t)gridDim.x * (CM_BLOCK / kWave)) {
      const CmMember X = cm_global_member(v, W, s0 + i);
      double sum = 0.0;
      for (int64_t j0 = 0; j0 < n; j0 += kWave) {
        const int64_t j = j0 + lane;
        double val = 0.0;
        if (j < n) {
          if (j == i) {
            val = cm_pair(X, X, true);
          } else {
            const CmMember Y = cm_global_member(v, W, s0 + j);
            val = i < j ? cm_pair(X, Y, false) : cm_pair(Y, X, false);
          }
        }
        buf[wid][lane] = val;
        wave_lds_sync();
        if (lane == 0) {
          const int cnt = n - j0 < kWave ? (int)(n - j0) : kWave;
          for (int t = 0; t < cnt; ++t) sum += buf[wid][t];
        }
        wave_lds_sync();
      }
      if (lane == 0) score[s0 + i] = sum / (double)n;
    }
  }
}

__global__ __launch_bounds__(CM_BLOCK) void cosine_medoid_argmax_kernel(CsrView v, CosMedWs W, const double* score,
                                                                       int64_t* rep, int32_t* status) {
  const int32_t nd = *W.n_def;
  for (int32_t d = blockIdx.x * CM_BLOCK + threadIdx.x; d < nd; d += gridDim.x * CM_BLOCK) {
    const int64_t c = W.def[d];
    const int64_t s0 = v.cluster_off[c], s1 = v.cluster_off[c + 1];
    int64_t best = s0;
    double bs = score[s0];
    for (int64_t s = s0 + 1; s < s1; ++s) {
      const double x = score[s];
      if (x > bs) { bs = x; best = s; }
    }
    rep[c] = best;
    status[c] = kOk;
  }
}

}  // namespace spx
