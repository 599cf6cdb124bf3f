// MGF text -> cluster-segmented CSR on the device (spx_parse_mgf_text; the opt-in
// device-side ingest of the three CLIs).
//
// The host indexes the file (spx_mgf_index: byte range and peak-line count per
// record, no number parsed), copies the raw bytes to HBM and lists the records in
// destination (cluster) order with spec_off built from the index's peak counts.
// One workgroup then walks one record in tiles of kMgfTile bytes:
//   - every thread classifies kMgfPer byte positions: a position starts a line after
//     '\n', or after '\r' when the byte itself is not '\n' (Python's universal
//     newlines, as mgf_io.cpp's next_line splits them);
//   - the starts of peak lines (first byte a digit) are ranked by a block scan and
//     compacted into an LDS list, so full waves parse them, one thread per line,
//     into mz/inten[spec_off[r] + rank];
//   - the thread that finds any other line (headers, END IONS) handles it itself.
//
// The oracle is the host parser (mgf_io.cpp parse_range / parse_range_general,
// pinned to Python float()).  The kernel accepts only the canonical subset whose
// meaning it can decide with certainty and reports every other record as
// SPX_MGF_REPARSE; the caller re-parses those on the host.  A wrong value under
// SPX_MGF_OK is never allowed, a flag is always safe.  Canonical: ASCII without NUL;
// header keys at most once, upper case at column 0 (TITLE, PEPMASS=<dec> [general:
// <dec> <dec>], CHARGE=<digits>[+] [general: or -], RTINSECONDS=<dec>; any other line
// that starts with an upper-case letter is ignored, as the host ignores it); peak
// lines "<dec><sep><dec>" by the rules of fast_peak_line; one END IONS line after
// them, then only blank lines (the binning grammar also passes over "BEGIN IONS"
// lines, which its host parser ignores: the next record's lies in this one's range).
// <dec> = digits[.digits], <= 19 significant and <= 27 fraction digits.
//
// Decimal to double: w / 10^f with w <= 2^53 and f <= 22 is one correctly rounded
// IEEE divide of exact operands (Clinger), the same expression the host evaluates.
// Every other value (16-19 digit repr text, f of 23..27) is decided exactly in
// integers: q = floor(w 2^s / 5^f) with s chosen so that q has at least 64 bits,
// the remainder as the sticky bit, round half to even at 53 bits, scale by 2^(-s-f).
//
// Every byte read lies in [rec_begin, rec_end) of a record whose range was checked
// against text_len; every peak written lies in [spec_off[r], spec_off[r+1]) checked
// against n_peaks.  A record with more peak lines than its slot is flagged and the
// extra lines are skipped.
#pragma once
#include "spx_device.hpp"

namespace spx {

constexpr int kMgfBlock = 256;
constexpr int kMgfPer = 4;                       // byte positions one thread classifies per tile
constexpr int kMgfTile = kMgfBlock * kMgfPer;    // 1,024 bytes
constexpr int kMgfOk = 0, kMgfReparse = 1;       // = SPX_MGF_OK / SPX_MGF_REPARSE

__device__ const double kMgfPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                         1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
__device__ const uint64_t kMgfPow5[28] = {1ull,
                                          5ull,
                                          25ull,
                                          125ull,
                                          625ull,
                                          3125ull,
                                          15625ull,
                                          78125ull,
                                          390625ull,
                                          1953125ull,
                                          9765625ull,
                                          48828125ull,
                                          244140625ull,
                                          1220703125ull,
                                          6103515625ull,
                                          30517578125ull,
                                          152587890625ull,
                                          762939453125ull,
                                          3814697265625ull,
                                          19073486328125ull,
                                          95367431640625ull,
                                          476837158203125ull,
                                          2384185791015625ull,
                                          11920928955078125ull,
                                          59604644775390625ull,
                                          298023223876953125ull,
                                          1490116119384765625ull,
                                          7450580596923828125ull};

// w / 10^frac (w < 2^64, 0 <= frac <= 27), correctly rounded to nearest even.
__device__ inline double mgf_decimal(uint64_t w, int frac) {
  if (w <= (uint64_t(1) << 53) && frac <= 22) return frac ? (double)w / kMgfPow10[frac] : (double)w;
  // w > 0 here.  N = w 2^s in [2^126, 2^127), D = 5^frac < 2^63: q = N / D > 2^63.
  const int s = __clzll((long long)w) + 63;
  const unsigned __int128 N = (unsigned __int128)w << s;
  const uint64_t D = kMgfPow5[frac];
  const unsigned __int128 q = N / D;
  const bool sticky = (uint64_t)(N % D) != 0;
  const uint64_t hi = (uint64_t)(q >> 64), lo = (uint64_t)q;
  const int L = hi ? 128 - __clzll((long long)hi) : 64 - __clzll((long long)lo);  // bit length, >= 64
  const int sh = L - 53;                                                          // >= 11
  uint64_t m = (uint64_t)(q >> sh);
  const unsigned __int128 rest = q & (((unsigned __int128)1 << sh) - 1);
  const unsigned __int128 half = (unsigned __int128)1 << (sh - 1);
  if (rest > half || (rest == half && (sticky || (m & 1)))) ++m;  // m <= 2^53: exact as a double
  return ldexp((double)m, sh - s - frac);
}

__device__ __forceinline__ bool mgf_digit(uint8_t c) { return (unsigned)(c - '0') <= 9u; }
__device__ __forceinline__ bool mgf_eol(uint8_t c) { return c == '\n' || c == '\r'; }

// digits[.digits] at t[p] (first byte a digit), p advanced past it; the value as
// mgf_io.cpp's scan_unsigned + decimal_value give it.  False: not decidable here.
__device__ inline bool mgf_scan_dec(const uint8_t* __restrict__ t, int64_t& p, int64_t e, double& out) {
  if (p >= e || !mgf_digit(t[p])) return false;
  uint64_t w = 0;
  int nd = 0, frac = 0;
  for (; p < e && mgf_digit(t[p]); ++p) {
    const unsigned d = t[p] - '0';
    if (w == 0 && d == 0) continue;  // leading zeros: no significant digit
    if (nd < 20) ++nd;  // saturates: 20 = too many
    if (nd <= 19) w = w * 10 + d;
  }
  if (p < e && t[p] == '.') {
    ++p;
    for (; p < e && mgf_digit(t[p]); ++p) {
      const unsigned d = t[p] - '0';
      if (frac < 64) ++frac;
      if (w == 0 && d == 0) continue;
      if (nd < 20) ++nd;
      if (nd <= 19) w = w * 10 + d;
    }
  }
  if (nd > 19 || frac > 27) return false;
  out = mgf_decimal(w, frac);
  return true;
}

// [p, p + n) == lit, inside [.., e)
__device__ inline bool mgf_prefix(const uint8_t* __restrict__ t, int64_t p, int64_t e, const char* lit, int n) {
  if (e - p < n) return false;
  for (int i = 0; i < n; ++i)
    if (t[p + i] != (uint8_t)lit[i]) return false;
  return true;
}
// the same, ignoring ASCII case (lit in lower case)
__device__ inline bool mgf_prefix_ci(const uint8_t* __restrict__ t, int64_t p, int64_t e, const char* lit, int n) {
  if (e - p < n) return false;
  for (int i = 0; i < n; ++i)
    if ((t[p + i] | 0x20) != (uint8_t)lit[i]) return false;
  return true;
}
// p is the record's end or a line terminator
__device__ __forceinline__ bool mgf_at_eol(const uint8_t* __restrict__ t, int64_t p, int64_t e) {
  return p >= e || mgf_eol(t[p]);
}

// "<dec><sep><dec>" + end of line at p (fast_peak_line): single = exactly one space.
__device__ inline bool mgf_peak_line(const uint8_t* __restrict__ t, int64_t p, int64_t e, bool single, double& a,
                                     double& v) {
  if (!mgf_scan_dec(t, p, e, a)) return false;
  if (p >= e || (t[p] != ' ' && (single || t[p] != '\t'))) return false;
  ++p;
  if (!single)
    while (p < e && (t[p] == ' ' || t[p] == '\t')) ++p;
  if (!mgf_scan_dec(t, p, e, v)) return false;
  return mgf_at_eol(t, p, e);
}

// CHARGE value: 1..9 digits, then '+' (general: or '-'), then the end of the line.
__device__ inline bool mgf_charge(const uint8_t* __restrict__ t, int64_t p, int64_t e, bool general, int& out) {
  int n = 0, v = 0;
  for (; p < e && mgf_digit(t[p]); ++p) {
    if (++n > 9) return false;
    v = v * 10 + (t[p] - '0');
  }
  if (n == 0) return false;
  if (p < e && t[p] == '+') ++p;
  else if (general && p < e && t[p] == '-') { v = -v; ++p; }
  out = v;
  return mgf_at_eol(t, p, e);
}

struct MgfShared {
  uint8_t tile[kMgfTile + 1];   // [0]: the byte before the tile
  uint16_t list[kMgfTile];      // tile-relative starts of the tile's peak lines, in order
  int tmp[kMgfBlock / kWave + 1];
  int bad, n_end, n_prec, n_charge, n_rt, n_title, charge;
  unsigned long long end_pos;   // position of the first END IONS line
  unsigned long long last_pos;  // 1 + the largest position of a header or peak line
  double prec, rt;
};

// A line at p that is neither blank nor a peak line, found by one thread.
__device__ inline void mgf_other_line(const uint8_t* __restrict__ t, int64_t b, int64_t p, int64_t e, bool general,
                                      MgfShared& S, int& bad, unsigned long long& last) {
  const uint8_t c = t[p];
  if (c < 'A' || c > 'Z') { bad = 1; return; }  // blanks, signs, lower case: the host strips or parses these
  if (mgf_prefix(t, p, e, "END IONS", 8)) {
    if (!mgf_at_eol(t, p + 8, e)) { bad = 1; return; }
    atomicAdd(&S.n_end, 1);
    atomicMin(&S.end_pos, (unsigned long long)p);
    return;
  }
  if (mgf_prefix(t, p, e, "BEGIN IONS", 10)) {
    // general: the record's first line (checked there); no other can lie in a record.
    // binning: the host parser ignores the line wherever it stands.
    if (!mgf_at_eol(t, p + 10, e) || (general && p != b)) bad = 1;
    return;
  }
  if ((unsigned long long)p + 1 > last) last = (unsigned long long)p + 1;
  double x;
  int z;
  int64_t q;
  if (!general) {
    if (mgf_prefix(t, p, e, "TITLE=", 6)) {
      if (p != b) bad = 1;  // a TITLE= line starts a record
      q = p + 6;
      while (q < e && !mgf_eol(t[q]) && t[q] != ';') ++q;
      if (q >= e || t[q] != ';') bad = 1;  // no "id;usi": the reference's parts[1] raises, the host falls back
    } else if (mgf_prefix(t, p, e, "PEPMASS=", 8)) {
      q = p + 8;
      if (mgf_scan_dec(t, q, e, x) && mgf_at_eol(t, q, e)) { atomicAdd(&S.n_prec, 1); S.prec = x; }
      else bad = 1;
    } else if (mgf_prefix(t, p, e, "CHARGE=", 7)) {
      if (mgf_charge(t, p + 7, e, false, z)) { atomicAdd(&S.n_charge, 1); S.charge = z; }
      else bad = 1;
    }
    return;  // any other line: ignored by the host parser too
  }
  q = p;
  while (q < e && !mgf_eol(t[q]) && t[q] != '=') ++q;
  if (q >= e || t[q] != '=') return;  // no '=': neither a peak nor a parameter, ignored
  const int kl = q - p > 64 ? 64 : (int)(q - p);
  ++q;
  if (kl == 5 && mgf_prefix_ci(t, p, e, "title", 5)) {
    if (mgf_prefix(t, p, e, "TITLE", 5)) atomicAdd(&S.n_title, 1);
    else bad = 1;
  } else if (kl == 7 && mgf_prefix_ci(t, p, e, "pepmass", 7)) {
    bool ok = mgf_prefix(t, p, e, "PEPMASS", 7) && mgf_scan_dec(t, q, e, x);
    if (ok && !mgf_at_eol(t, q, e)) {  // "<dec> <dec>": the precursor intensity, parsed and dropped
      double y;
      ok = t[q] == ' ' || t[q] == '\t';
      while (q < e && (t[q] == ' ' || t[q] == '\t')) ++q;
      ok = ok && mgf_scan_dec(t, q, e, y) && mgf_at_eol(t, q, e);
    }
    if (ok) { atomicAdd(&S.n_prec, 1); S.prec = x; }
    else bad = 1;
  } else if (kl == 6 && mgf_prefix_ci(t, p, e, "charge", 6)) {
    if (mgf_prefix(t, p, e, "CHARGE", 6) && mgf_charge(t, q, e, true, z)) { atomicAdd(&S.n_charge, 1); S.charge = z; }
    else bad = 1;
  } else if (kl == 11 && mgf_prefix_ci(t, p, e, "rtinseconds", 11)) {
    if (mgf_prefix(t, p, e, "RTINSECONDS", 11) && mgf_scan_dec(t, q, e, x) && mgf_at_eol(t, q, e)) {
      atomicAdd(&S.n_rt, 1);
      S.rt = x;
    } else {
      bad = 1;
    }
  }
}

__global__ __launch_bounds__(kMgfBlock) void mgf_parse_kernel(
    const uint8_t* __restrict__ text, int64_t text_len, const int64_t* __restrict__ rec_begin,
    const int64_t* __restrict__ rec_end, const int64_t* __restrict__ spec_off, int64_t n_records, int64_t n_peaks,
    int general, double* __restrict__ mz, double* __restrict__ inten, double* __restrict__ prec,
    int32_t* __restrict__ charge, double* __restrict__ rt, int32_t* __restrict__ flags,
    int32_t* __restrict__ status) {
  __shared__ MgfShared S;
  const int tid = (int)threadIdx.x;
  const double kNaN = __longlong_as_double(0x7ff8000000000000ll);
  for (int64_t r = blockIdx.x; r < n_records; r += gridDim.x) {
    const int64_t b = rec_begin[r], e = rec_end[r], o0 = spec_off[r], o1 = spec_off[r + 1];
    if (b < 0 || e < b || e > text_len || o0 < 0 || o1 < o0 || o1 > n_peaks) {  // uniform: nothing is read
      if (tid == 0) {
        prec[r] = kNaN;
        rt[r] = kNaN;
        charge[r] = 0;
        flags[r] = 0;
        status[r] = kMgfReparse;
      }
      continue;
    }
    const int64_t npk = o1 - o0;
    if (tid == 0) {
      S.bad = 0;
      S.n_end = S.n_prec = S.n_charge = S.n_rt = S.n_title = 0;
      S.charge = 0;
      S.end_pos = ~0ull;
      S.last_pos = 0ull;
      S.prec = S.rt = kNaN;
      // the record's first line: TITLE=... (binning) or exactly BEGIN IONS (general)
      if (general ? !(mgf_prefix(text, b, e, "BEGIN IONS", 10) && mgf_at_eol(text, b + 10, e))
                  : !mgf_prefix(text, b, e, "TITLE=", 6))
        S.bad = 1;
    }
    __syncthreads();
    int bad = 0;
    unsigned long long last = 0;
    int64_t running = 0;  // peak lines before this tile (uniform)
    for (int64_t t0 = b; t0 < e; t0 += kMgfTile) {
      const int n = e - t0 < kMgfTile ? (int)(e - t0) : kMgfTile;
      for (int i = tid; i < n; i += kMgfBlock) S.tile[1 + i] = text[t0 + i];
      if (tid == 0) S.tile[0] = t0 > b ? text[t0 - 1] : (uint8_t)'\n';
      __syncthreads();
      int cnt = 0, mask = 0;
#pragma unroll
      for (int j = 0; j < kMgfPer; ++j) {
        const int i = tid * kMgfPer + j;
        if (i >= n) break;
        const uint8_t c = S.tile[1 + i], pv = S.tile[i];
        if (c >= 0x80 || c == 0) bad = 1;
        if (pv == '\n' || (pv == '\r' && c != '\n')) {
          if (mgf_digit(c)) { mask |= 1 << j; ++cnt; }
          else if (!mgf_eol(c)) mgf_other_line(text, b, t0 + i, e, general != 0, S, bad, last);
        }
      }
      int total;
      int k = block_exclusive_scan<kMgfBlock, int>(cnt, S.tmp, total);
#pragma unroll
      for (int j = 0; j < kMgfPer; ++j)
        if (mask & (1 << j)) S.list[k++] = (uint16_t)(tid * kMgfPer + j);
      __syncthreads();
      for (int q = tid; q < total; q += kMgfBlock) {
        const int64_t kk = running + q, p = t0 + S.list[q];
        if ((unsigned long long)p + 1 > last) last = (unsigned long long)p + 1;
        double a, v;
        if (kk >= npk) {
          bad = 1;  // more peak lines than the index counted: skipped, never written
        } else if (mgf_peak_line(text, p, e, general == 0, a, v)) {
          mz[o0 + kk] = a;
          inten[o0 + kk] = v;
        } else {
          bad = 1;
        }
      }
      running += total;
      __syncthreads();  // the tile and the list are rewritten next
    }
    if (bad) atomicOr(&S.bad, 1);
    if (last) atomicMax(&S.last_pos, last);
    __syncthreads();
    if (tid == 0) {
      bool ok = !S.bad && S.n_end == 1 && S.last_pos <= S.end_pos && running == npk && S.n_prec <= 1 &&
                S.n_charge <= 1 && S.n_rt <= 1 && S.n_title <= 1;
      // the binning parser carries PEPMASS / CHARGE over from the record parsed before
      if (!general && (S.n_prec == 0 || S.n_charge == 0)) ok = false;
      prec[r] = S.n_prec ? S.prec : kNaN;
      charge[r] = S.n_charge ? S.charge : 0;
      rt[r] = (general && S.n_rt) ? S.rt : kNaN;
      flags[r] = (S.n_prec ? 1 : 0) | (S.n_charge ? 2 : 0) | ((general && S.n_rt) ? 4 : 0) |
                 ((general && S.n_title) ? 8 : 0);
      status[r] = ok ? kMgfOk : kMgfReparse;
    }
    __syncthreads();  // S is reset for the next record
  }
}

}  // namespace spx
