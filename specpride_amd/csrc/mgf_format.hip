// Device-side MGF emit: the peak lines "repr(mz) repr(inten)\n" of a list of peak
// segments, formatted in HBM (spx_format_peaks, include/specpride.h).
// The counterpart of mgf_parse.hip: the digits are repr_core.hpp's, the arithmetic
// the host writer and spx_repr_f64 run.
//
// Work is divided over PEAKS, not segments.  The valid segments' lengths are scanned
// into voff[S + 1]: "virtual peak" v in [voff[i], voff[i + 1]) is peak seg_begin[i] +
// (v - voff[i]) of segment i (overlapping and out-of-order segments are simply listed
// again), and the V = voff[S] virtual peaks are cut into equal runs of 256-peak tiles,
// one run per workgroup: a 70,000-peak segment spreads over the grid, a thousand
// one-peak segments share a few tiles.
//
// Line lengths depend on the data, so the text cannot be placed before they are
// summed.  The lines are FORMATTED TWICE: fmt_peaks_kernel<false> sums each
// workgroup's bytes (digits and lengths only), fmt_peaks_kernel<true> generates the
// digits again, scans the tile's lengths, writes the characters into LDS and stores
// the tile's text in 16-byte units.  Keeping (digits, exponent, length) between the
// passes instead would cost 24 B of HBM written and read back per peak against 16 B
// of input read again, and a workspace that grows with the peaks covered -- which
// overlapping segments make independent of n_peaks; this way the workspace is the
// S + 1 offsets and two fixed arrays of per-workgroup sums.
//
// Kernels (all on the caller's stream, no inter-workgroup communication inside one):
//   fmt_seg_sum_kernel    per-workgroup sums of the segment lengths; flags bit1
//   fmt_seg_scan_kernel   voff = exclusive scan of the lengths
//   fmt_peaks_kernel<0>   per-workgroup text bytes
//   fmt_peaks_kernel<1>   text, text_off of the non-empty segments, flags bit0
//   fmt_seg_fix_kernel    text_off of the empty segments
#pragma once
#include "repr_core.hpp"
#include "spx_device.hpp"

namespace spx {

constexpr int kFmtBlock = 256;
constexpr int kFmtLine = 2 * spx_repr::kMaxLen + 2;  // 50: the longest peak line
constexpr int kFmtSegGrid = 1024;                    // workgroups of the segment passes, at most
constexpr int kFmtPeakGrid = 2048;                   // workgroups of the peak passes, at most
constexpr int kFmtFlagCapacity = 1, kFmtFlagRange = 2;
constexpr int kFmtLdsBytes = 16 + kFmtBlock * kFmtLine;  // a tile's text behind its 16-byte misalignment

// peaks of segment i; 0 for a range that is reversed or leaves [0, n_peaks]
__device__ __forceinline__ int64_t fmt_seg_len(const int64_t* seg_begin, const int64_t* seg_end, int64_t i,
                                               int64_t n_peaks, bool& bad) {
  const int64_t b = seg_begin[i], e = seg_end[i];
  bad = b < 0 || e < b || e > n_peaks;
  return bad ? 0 : e - b;
}

// the workgroup's run [a, b) of n items: equal runs of whole 256-item tiles
__device__ __forceinline__ void fmt_run(int64_t n, int64_t& a, int64_t& b) {
  const int64_t tiles = (n + kFmtBlock - 1) / kFmtBlock;
  const int64_t per = (tiles + gridDim.x - 1) / gridDim.x * kFmtBlock;
  a = min(n, (int64_t)blockIdx.x * per);
  b = min(n, a + per);
}

// sum over the workgroup (every thread gets it); tmp: kFmtBlock / 64 + 1 entries of LDS
__device__ __forceinline__ int64_t fmt_block_sum(int64_t v, int64_t* tmp) {
  int64_t total;
  block_exclusive_scan<kFmtBlock, int64_t>(v, tmp, total);
  return total;
}

// part[0 .. blockIdx.x) summed, and all of part[0 .. gridDim.x) into `all`
__device__ __forceinline__ int64_t fmt_sum_before(const int64_t* part, int64_t* tmp, int64_t& all) {
  int64_t before = 0, every = 0;
  for (unsigned j = threadIdx.x; j < gridDim.x; j += kFmtBlock) {
    const int64_t p = part[j];
    every += p;
    if (j < blockIdx.x) before += p;
  }
  all = fmt_block_sum(every, tmp);
  return fmt_block_sum(before, tmp);
}

// the last s in [lo, hi) with voff[s] <= v (voff[lo] <= v < voff[hi]): v's segment --
// never an empty one, those share their successor's offset
__device__ __forceinline__ int64_t fmt_seg_of(const int64_t* voff, int64_t lo, int64_t hi, int64_t v) {
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (voff[mid] <= v) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kFmtBlock) void fmt_seg_sum_kernel(const int64_t* __restrict__ seg_begin,
                                                                const int64_t* __restrict__ seg_end, int64_t S,
                                                                int64_t n_peaks, int64_t* __restrict__ part,
                                                                int32_t* __restrict__ flags) {
  __shared__ int64_t tmp[kFmtBlock / kWave + 1];
  int64_t a, b;
  fmt_run(S, a, b);
  int64_t sum = 0;
  bool any_bad = false;
  for (int64_t i = a + threadIdx.x; i < b; i += kFmtBlock) {
    bool bad;
    sum += fmt_seg_len(seg_begin, seg_end, i, n_peaks, bad);
    any_bad |= bad;
  }
  sum = fmt_block_sum(sum, tmp);
  if (threadIdx.x == 0) part[blockIdx.x] = sum;
  if (__ballot(any_bad) != 0ull && lane_id() == 0) atomicOr(flags, kFmtFlagRange);
}

__global__ __launch_bounds__(kFmtBlock) void fmt_seg_scan_kernel(const int64_t* __restrict__ seg_begin,
                                                                 const int64_t* __restrict__ seg_end, int64_t S,
                                                                 int64_t n_peaks, const int64_t* __restrict__ part,
                                                                 int64_t* __restrict__ voff) {
  __shared__ int64_t tmp[kFmtBlock / kWave + 1];
  int64_t a, b, all;
  fmt_run(S, a, b);
  int64_t base = fmt_sum_before(part, tmp, all);
  if (blockIdx.x == 0 && threadIdx.x == 0) voff[S] = all;
  for (int64_t t = a; t < b; t += kFmtBlock) {
    const int64_t i = t + threadIdx.x;
    bool bad;
    const int64_t len = i < b ? fmt_seg_len(seg_begin, seg_end, i, n_peaks, bad) : 0;
    int64_t total;
    const int64_t excl = block_exclusive_scan<kFmtBlock, int64_t>(len, tmp, total);
    if (i < b) voff[i] = base + excl;
    base += total;
  }
}

// kEmit = false: part[workgroup] = the bytes of the workgroup's lines.
// kEmit = true: the text itself (part holds every workgroup's bytes).
template <bool kEmit>
__global__ __launch_bounds__(kFmtBlock) void fmt_peaks_kernel(
    const double* __restrict__ mz, const double* __restrict__ inten, const int64_t* __restrict__ seg_begin,
    const int64_t* __restrict__ voff, int64_t S, int32_t skip_nan, uint8_t* __restrict__ text, int64_t text_capacity,
    int64_t* __restrict__ text_off, int32_t* __restrict__ flags, int64_t* __restrict__ part) {
  __shared__ int64_t tmp[kFmtBlock / kWave + 1];
  __shared__ int32_t tmp32[kFmtBlock / kWave + 1];
  __shared__ int64_t s_seg[2];
  __shared__ uint4 s_text[kEmit ? (kFmtLdsBytes + 15) / 16 : 1];
  const int64_t V = voff[S];
  int64_t v0, v1;
  fmt_run(V, v0, v1);
  int64_t at = 0;     // kEmit: where the next tile's text starts
  bool write = true;  // kEmit: the text fits
  if constexpr (kEmit) {
    int64_t all;
    at = fmt_sum_before(part, tmp, all);
    write = all <= text_capacity;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      text_off[S] = all;
      if (!write) atomicOr(flags, kFmtFlagCapacity);
    }
  }
  int64_t bytes = 0;  // !kEmit: this thread's share
  uint8_t* const lds = reinterpret_cast<uint8_t*>(s_text);
  for (int64_t t = v0; t < v1; t += kFmtBlock) {
    // the tile's first and last segment bound every lane's search
    if (threadIdx.x == 0) s_seg[0] = fmt_seg_of(voff, 0, S, t);
    if (threadIdx.x == kWave) s_seg[1] = fmt_seg_of(voff, 0, S, min(t + kFmtBlock, v1) - 1);
    __syncthreads();
    const int64_t v = t + threadIdx.x;
    const bool active = v < v1;
    int32_t len = 0;
    int64_t seg = 0, vfirst = 0;
    spx_repr::Decimal dm{}, di{};
    if (active) {
      seg = fmt_seg_of(voff, s_seg[0], s_seg[1] + 1, v);
      vfirst = voff[seg];
      const int64_t p = seg_begin[seg] + (v - vfirst);
      const double it = inten[p];
      if (!(skip_nan && it != it)) {
        dm = spx_repr::decompose(mz[p]);
        di = spx_repr::decompose(it);
        len = spx_repr::length(dm) + spx_repr::length(di) + 2;
      }
    }
    if constexpr (!kEmit) {
      bytes += len;
      __syncthreads();  // s_seg is rewritten by the next tile
    } else {
      int32_t total;
      const int32_t excl = block_exclusive_scan<kFmtBlock, int32_t>(len, tmp32, total);
      if (active && v == vfirst) text_off[seg] = at + excl;  // (a skipped first line: where it would start)
      if (write) {
        // the tile's text sits in LDS as it will in memory, behind the bytes that
        // precede it in its first 16-byte unit
        const int32_t pad = (int32_t)((reinterpret_cast<uintptr_t>(text) + (uint64_t)at) & 15);
        if (len) {
          uint8_t* o = lds + pad + excl;
          o += spx_repr::emit(dm, o);
          *o++ = ' ';
          o += spx_repr::emit(di, o);
          *o = '\n';
        }
        __syncthreads();
        uint8_t* const dst = text + at - pad;  // 16-byte aligned; bytes [pad, end) of it are this tile's
        const int32_t end = pad + total;
        for (int32_t u = threadIdx.x * 16; u < end; u += kFmtBlock * 16) {
          if (u >= pad && u + 16 <= end) {
            *reinterpret_cast<uint4*>(dst + u) = s_text[u >> 4];
          } else {  // the tile's first and last unit: shared with its neighbours' text
            for (int32_t k = max(u, pad); k < min(u + 16, end); ++k) dst[k] = lds[k];
          }
        }
      }
      __syncthreads();  // the LDS text and s_seg are rewritten by the next tile
      at += total;
    }
  }
  if constexpr (!kEmit) {
    bytes = fmt_block_sum(bytes, tmp);
    if (threadIdx.x == 0) part[blockIdx.x] = bytes;
  }
}

// an empty segment's block is empty at the start of the next non-empty segment's (or
// at the end of the text); reads only what fmt_peaks_kernel<true> wrote
__global__ __launch_bounds__(kFmtBlock) void fmt_seg_fix_kernel(const int64_t* __restrict__ voff, int64_t S,
                                                                int64_t* __restrict__ text_off) {
  const int64_t V = voff[S];
  for (int64_t i = (int64_t)blockIdx.x * kFmtBlock + threadIdx.x; i < S; i += (int64_t)gridDim.x * kFmtBlock) {
    const int64_t v = voff[i];
    if (voff[i + 1] != v) continue;
    text_off[i] = v == V ? text_off[S] : text_off[fmt_seg_of(voff, i, S, v)];
  }
}

}  // namespace spx
