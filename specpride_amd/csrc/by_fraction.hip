// Explained b/y intensity: benchmark.fraction_of_by (reference src/benchmark.py:40-61)
// for every segment of a peak array in one launch.
//
// Per spectrum the reference builds a spectrum_utils MsmsSpectrum (peaks sorted by
// m/z), keeps 100 <= m/z <= 1400, drops the peaks within 50 ppm of the precursor at
// charges z..1, annotates the b and y ions of the peptide (charges 1..max(1, z-1),
// 50 ppm, the most intense peak of each window) and returns the annotated share of the
// remaining intensity.  What the two libraries compute is restated in DESIGN.md
// section 4 (parity is unpinned at that boundary); every constant is in ByParams.
//
// One wave per spectrum, BY_WAVES spectra per workgroup:
//   pass 1  one coalesced pass over the segment: every m/z finite?  non-decreasing?
//           the kept predicate (range and precursor windows), `current`, and the first
//           and last kept index (the span).  A segment of at most BY_STAGE peaks leaves
//           its m/z in LDS, so pass 2's searches and scans do not go back to memory.
//   pass 2  the lanes take the fragments 64 at a time.  A lane forms its fragment's m/z
//           with pyteomics' order of operations from the residue masses in LDS, finds
//           the window's best peak -- sorted spectrum: binary search for a bound just
//           below the window, then a scan to a bound just above it; unsorted: a scan of
//           the whole span -- under one comparator (intensity descending with NaN
//           first, m/z ascending, index ascending: np.argmax over the sorted peaks),
//           and sets the peak's bit in the wave's LDS bitmap (integer ds_or).
//   pass 3  the set bits' intensities are summed: a peak several fragments chose counts
//           once.
// The bitmap covers BY_CHUNK peaks of the span; a longer span repeats passes 2 and 3 per
// chunk, so spectrum length is unbounded.  Nothing is sorted, nothing is written but the
// two outputs, and there are no float atomics: `current` and `by_current` are lane-strided
// partial sums folded by a fixed butterfly (deterministic; not the reference's sequential
// order, within n * 2^-53 of it for non-negative intensities).
//
// LDS per workgroup: 4 x (2 KiB residue masses + 512 B precursor m/z + 512 B bitmap +
// 2 KiB staged m/z) + the 26 letter masses = 20.25 KiB, so LDS admits 7 workgroups a CU,
// as many waves (7 a SIMD) as the registers admit.  The kernel is latency-bound on a
// wave's chain of dependent steps, not on HBM.
//
// Limits: sequences of at most BY_MAX_SEQ residues and charges of
// at most BY_MAX_CHARGE; beyond them, for a segment range outside [0, n_peaks] or
// reversed, and for a non-finite m/z or precursor m/z the segment is kDeferred
// (SPX_UNRESOLVED) with a NaN fraction.
#include "spx_device.hpp"

namespace spx {

constexpr int BY_WAVES = 4;
constexpr int BY_MAX_SEQ = 256;
constexpr int BY_MAX_CHARGE = 64;
constexpr int BY_CHUNK = 4096;  // peaks one bitmap covers (BY_CHUNK / 32 words a wave)
constexpr int BY_STAGE = 256;   // a segment of at most this many peaks keeps its m/z in LDS for pass 2

// spx_by_params, field for field (spx_api.hip asserts the size)
struct ByParams {
  double aa_mass[26];
  double h, o, proton, precursor_proton, min_mz, max_mz, tol_ppm;
};

__device__ __forceinline__ void by_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool by_finite(double x) {
  return ((uint64_t)__double_as_longlong(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// a remaining peak: inside the m/z range and outside every precursor window
// (rc[0..z): the precursor's m/z at charges 1..z, in LDS)
__device__ __forceinline__ bool by_kept(double m, double min_mz, double max_mz, double tol, const double* rc, int z) {
  if (!(m >= min_mz && m <= max_mz)) return false;
  for (int c = 0; c < z; ++c) {
    const double r = rc[c];
    if (fabs((m - r) / r * 1e6) <= tol) return false;
  }
  return true;
}

// peak a before peak b in a window: np.argmax over the peaks in (m/z, index) order
__device__ __forceinline__ bool by_better(double va, double ma, int64_t ka, double vb, double mb, int64_t kb) {
  const bool na = va != va, nb = vb != vb;
  if (na != nb) return na;
  if (!na && va != vb) return va > vb;
  return ma < mb || (ma == mb && ka < kb);
}

// the annotated peak of the fragment at m/z f among peaks [k0, k1], or -1.  kStaged: the
// segment's m/z are in LDS (smz[k - b]), else they are read from global memory.
template <bool kStaged>
__device__ __forceinline__ int64_t by_pick(const double* __restrict__ mz, const double* smz, int64_t b,
                                           const double* __restrict__ inten, int64_t k0, int64_t k1, bool sorted,
                                           double f, double min_mz, double max_mz, double tol, const double* rc, int z) {
  auto at = [&](int64_t k) { return kStaged ? smz[k - b] : mz[k]; };
  int64_t lo = k0;
  // the window lies inside [f - d, f + d]: d exceeds |f| * tol * 1e-6 by more than the
  // rounding of the predicate below
  const double d = fabs(f) * (tol * 1.000001e-6 + 1e-15);
  const double lo_b = f - d, hi_b = f + d;
  if (sorted) {
    int64_t hi = k1 + 1;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (at(mid) < lo_b) lo = mid + 1; else hi = mid;
    }
  }
  int64_t best = -1;
  double bv = 0.0, bm = 0.0;
  for (int64_t k = lo; k <= k1; ++k) {
    const double m = at(k);
    if (sorted && !(m <= hi_b)) break;
    const double x = (m - f) / f * 1e6;
    if (x >= -tol && x <= tol && by_kept(m, min_mz, max_mz, tol, rc, z)) {
      const double v = inten[k];
      if (best < 0 || by_better(v, m, k, bv, bm, best)) { best = k; bv = v; bm = m; }
    }
  }
  return best;
}

__global__ __launch_bounds__(BY_WAVES * kWave) void by_fraction_kernel(
    const double* __restrict__ mz, const double* __restrict__ inten, int64_t n_peaks,
    const int64_t* __restrict__ seg_begin, const int64_t* __restrict__ seg_end, int64_t S,
    const double* __restrict__ prec_mz, const int32_t* __restrict__ charge, const uint8_t* __restrict__ seq,
    const int64_t* __restrict__ seq_off, ByParams P, double* __restrict__ fraction, int32_t* __restrict__ status) {
  __shared__ double s_aa[32];
  __shared__ double s_res[BY_WAVES][BY_MAX_SEQ];
  __shared__ double s_rc[BY_WAVES][BY_MAX_CHARGE];
  __shared__ uint32_t s_bm[BY_WAVES][BY_CHUNK / 32];
  __shared__ double s_mz[BY_WAVES][BY_STAGE];
#pragma unroll
  for (int k = 0; k < 26; ++k)
    if (threadIdx.x == k) s_aa[k] = P.aa_mass[k];
  __syncthreads();
  const int64_t s = (int64_t)blockIdx.x * BY_WAVES + wave_id();
  if (s >= S) return;  // wave-uniform, after the only workgroup barrier
  const int lane = lane_id();
  double* res = s_res[wave_id()];
  double* rc = s_rc[wave_id()];
  uint32_t* bm = s_bm[wave_id()];
  double* smz = s_mz[wave_id()];
  const double nan = __longlong_as_double(0x7ff8000000000000ll);

  const int64_t b = seg_begin[s], e = seg_end[s];
  const int64_t q0 = seq_off[s], L64 = seq_off[s + 1] - q0;
  const int z = charge[s];
  const double pmz = prec_mz[s];
  if (b < 0 || e > n_peaks || b > e || q0 < 0 || L64 < 0 || L64 > BY_MAX_SEQ) {
    if (lane == 0) { fraction[s] = nan; status[s] = kDeferred; }
    return;
  }
  const int L = (int)L64;

  // the residues' masses; a character that is no residue makes the sequence invalid
  bool bad = false;
  for (int j = lane; j < L; j += kWave) {
    const int a = (int)seq[q0 + j] - 'A';
    const double w = s_aa[(a >= 0 && a < 26) ? a : 0];
    const bool ok = a >= 0 && a < 26 && w == w;
    bad |= !ok;
    res[j] = ok ? w : 0.0;
  }
  if (__ballot(bad) != 0ull) {  // parser.fast_valid fails: 0.0 before the spectrum is looked at
    if (lane == 0) { fraction[s] = 0.0; status[s] = kOk; }
    return;
  }
  if (z > BY_MAX_CHARGE || !by_finite(pmz)) {
    if (lane == 0) { fraction[s] = nan; status[s] = kDeferred; }
    return;
  }
  // remove_precursor_peak: the precursor at charges z..1 (lane c - 1 forms r_c)
  if (lane < z) {
    const double neutral = (pmz - P.precursor_proton) * (double)z;
    rc[lane] = neutral / (double)(lane + 1) + P.precursor_proton;
  }
  by_wave_sync();
  const int zr = z > 0 ? z : 0;

  // pass 1
  double cur = 0.0;
  int64_t kmin = INT64_MAX, kmax = -1;
  bool finite = true, sorted = true;
  const bool staged = e - b <= BY_STAGE;  // wave-uniform
  for (int64_t k = b + lane; k < e; k += kWave) {
    const double m = mz[k], v = inten[k];
    if (staged) smz[k - b] = m;
    const double pm = k > b ? mz[k - 1] : m;
    finite &= by_finite(m);
    sorted &= pm <= m;
    if (by_kept(m, P.min_mz, P.max_mz, P.tol_ppm, rc, zr)) {
      cur += v;
      kmin = k < kmin ? k : kmin;
      kmax = k > kmax ? k : kmax;
    }
  }
  if (__ballot(!finite) != 0ull) {
    if (lane == 0) { fraction[s] = nan; status[s] = kDeferred; }
    return;
  }
  sorted = __ballot(!sorted) == 0ull;
  cur = wave_sum_f64(cur);
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const int64_t a = __shfl_xor(kmin, o, kWave), c = __shfl_xor(kmax, o, kWave);
    kmin = a < kmin ? a : kmin;
    kmax = c > kmax ? c : kmax;
  }
  if (!(cur > 0.0)) {  // nothing left, all zero, or a NaN among the remaining intensities
    if (lane == 0) { fraction[s] = 0.0; status[s] = kOk; }
    return;
  }

  // passes 2 and 3, per chunk of the span
  const int zq = z - 1 > 1 ? z - 1 : 1;
  const int F = L >= 2 ? 2 * (L - 1) * zq : 0;
  const double water = P.h * 2.0 + P.o, b_delta = (P.h * -2.0) + (P.o * -1.0);
  double by = 0.0;
  for (int64_t cb = kmin; cb <= kmax; cb += BY_CHUNK) {
    bm[lane] = 0u;
    bm[lane + kWave] = 0u;
    by_wave_sync();
    for (int t0 = 0; t0 < F; t0 += kWave) {
      const int t = t0 + lane;
      if (t < F) {
        const int q = t % zq + 1, u = t / zq, i = (u >> 1) + 1;
        const bool is_y = u & 1;
        // mass.fast_mass: residues left to right, then water, then the ion type's change
        double m = 0.0;
        const int j1 = is_y ? L : i;
        for (int j = is_y ? i : 0; j < j1; ++j) m += res[j];
        m += water;
        if (!is_y) m += b_delta;
        const double f = (m + P.proton * (double)q) / (double)q;
        const int64_t w = staged ? by_pick<true>(mz, smz, b, inten, kmin, kmax, sorted, f, P.min_mz, P.max_mz,
                                                 P.tol_ppm, rc, zr)
                                 : by_pick<false>(mz, smz, b, inten, kmin, kmax, sorted, f, P.min_mz, P.max_mz,
                                                  P.tol_ppm, rc, zr);
        if (w >= cb && w - cb < BY_CHUNK) atomicOr(&bm[(w - cb) >> 5], 1u << ((w - cb) & 31));
      }
    }
    by_wave_sync();
    const int64_t ce = kmax + 1 - cb < BY_CHUNK ? kmax + 1 : cb + BY_CHUNK;
    for (int64_t k = cb + lane; k < ce; k += kWave) {
      const int r = (int)(k - cb);
      if ((bm[r >> 5] >> (r & 31)) & 1u) by += inten[k];
    }
    by_wave_sync();  // the next chunk's zeroing after these reads
  }
  by = wave_sum_f64(by);
  if (lane == 0) { fraction[s] = by / cur; status[s] = kOk; }
}

}  // namespace spx
