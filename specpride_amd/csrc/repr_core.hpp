// Python repr(float) -- shortest round-trip decimal digits, Python's layout -- as
// one digit-generation core for the host (g++) and the device (hipcc): the format
// kernel (mgf_format.hip), the splicing MGF writer's header floats (mgf_splice.hpp)
// and spx_repr_f64 run the same arithmetic.
//
// Digits: the Schubfach construction (R. Giulietti, "The Schubfach way to render
// doubles").  v = c * 2^q; with k = floor(log10(2^q)) (or of 3/4 * 2^q at a power of
// two, where the lower neighbour is half as far) the rounding interval's two ends and
// v itself are scaled by 10^-k through ONE 128-bit table entry g(-k) (tools/
// gen_repr_tables.py) and rounded to odd, which keeps every comparison below exact:
// there is no "undecided" case and no fallback.  The shortest candidate in the
// interval wins (one digit fewer first), ties to the one closest to v, then to even.
//
// Layout (Python's float_repr_style 'short', format code 'r'): decimal exponent e of
// d.ddd in [-4, 16) positional ("0.0001", "123.45", "100.0"), otherwise d[.ddd]e+XX
// with at least two exponent digits.  At most 24 bytes ("-2.2250738585072014e-308").
#pragma once
#include <stdint.h>

#include "repr_pow10_table.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPX_HD __host__ __device__ inline
#else
#define SPX_HD inline
#endif

namespace spx_repr {

constexpr int kMaxLen = 24;

// usable from device code as well: a constant-initialised constexpr array
static constexpr uint64_t kPow10[SPX_REPR_POW10_MAX - SPX_REPR_POW10_MIN + 1][2] = {SPX_REPR_POW10_ENTRIES};

enum Kind : int32_t { kFinite = 0, kNan = 1, kInf = 2 };

// x = (-1)^neg * digits * 10^(exp - nd + 1): nd significant digits (no trailing
// zero; zero is the one digit 0), exp the decimal exponent of the first digit.
struct Decimal {
  uint64_t digits;
  int32_t exp, nd;
  int32_t kind, neg;
};

// exact for the ranges the core uses them on (enumerated by tools/gen_repr_tables.py)
SPX_HD int32_t floor_log10_pow2(int32_t e) { return (e * 1262611) >> 22; }
SPX_HD int32_t floor_log10_three_quarters_pow2(int32_t e) { return (e * 1262611 - 524031) >> 22; }
SPX_HD int32_t floor_log2_pow10(int32_t e) { return (e * 1741647) >> 19; }

// floor(g * cp / 2^128), with the bits shifted out ORed into bit 0 ("round to odd")
SPX_HD uint64_t round_to_odd(uint64_t ghi, uint64_t glo, uint64_t cp) {
  const unsigned __int128 x = (unsigned __int128)glo * cp;
  const unsigned __int128 y = (unsigned __int128)ghi * cp + (uint64_t)(x >> 64);
  return (uint64_t)(y >> 64) | (uint64_t)((uint64_t)y > 1);
}

// shortest digits of c * 2^q (c > 0): value = digits * 10^k
SPX_HD void shortest(uint64_t c, int32_t q, bool lower_closer, uint64_t& digits, int32_t& k) {
  const uint64_t odd = c & 1;  // an odd c's interval is open: IEEE rounds ties to even
  const uint64_t cbl = 4 * c - 2 + (lower_closer ? 1 : 0), cb = 4 * c, cbr = 4 * c + 2;
  k = lower_closer ? floor_log10_three_quarters_pow2(q) : floor_log10_pow2(q);
  const int32_t h = q + floor_log2_pow10(-k) + 1;  // 1..4
  const uint64_t ghi = kPow10[-k - SPX_REPR_POW10_MIN][0], glo = kPow10[-k - SPX_REPR_POW10_MIN][1];
  const uint64_t vbl = round_to_odd(ghi, glo, cbl << h);
  const uint64_t vb = round_to_odd(ghi, glo, cb << h);
  const uint64_t vbr = round_to_odd(ghi, glo, cbr << h);
  const uint64_t lower = vbl + odd, upper = vbr - odd;
  const uint64_t s = vb >> 2;  // v * 10^-k = s + a fraction, in quarter units in vb
  if (s >= 10) {               // a multiple of 10 inside the interval: one digit fewer
    const uint64_t sp = s / 10;
    const bool up_in = lower <= 40 * sp, wp_in = 40 * sp + 40 <= upper;
    if (up_in != wp_in) {
      digits = sp + (wp_in ? 1 : 0);
      k += 1;
      return;
    }
  }
  const bool u_in = lower <= 4 * s, w_in = 4 * s + 4 <= upper;
  if (u_in != w_in) {
    digits = s + (w_in ? 1 : 0);
    return;
  }
  const uint64_t mid = 4 * s + 2;  // both or neither: the one closer to v, ties to even
  digits = s + ((vb > mid || (vb == mid && (s & 1))) ? 1 : 0);
}

SPX_HD Decimal decompose(double x) {
  uint64_t bits;
  __builtin_memcpy(&bits, &x, sizeof(bits));
  Decimal d;
  d.neg = (int32_t)(bits >> 63);
  d.digits = 0;
  d.exp = 0;
  d.nd = 1;
  d.kind = kFinite;
  const uint64_t frac = bits & ((uint64_t(1) << 52) - 1);
  const int32_t be = (int32_t)((bits >> 52) & 0x7FF);
  if (be == 0x7FF) {
    d.kind = frac ? kNan : kInf;
    return d;
  }
  if (be == 0 && frac == 0) return d;  // +-0.0
  const uint64_t c = be ? (frac | (uint64_t(1) << 52)) : frac;
  const int32_t q = be ? be - 1075 : -1074;
  uint64_t dg;
  int32_t k;
  shortest(c, q, frac == 0 && be > 1, dg, k);
  if (dg % 100000000u == 0) {
    dg /= 100000000u;
    k += 8;
  }
  while (dg % 10 == 0) {
    dg /= 10;
    ++k;
  }
  int32_t nd = 1;
  for (uint64_t p = 10; nd < 17 && dg >= p; p *= 10) ++nd;
  d.digits = dg;
  d.nd = nd;
  d.exp = k + nd - 1;
  return d;
}

SPX_HD bool positional(const Decimal& d) { return d.exp >= -4 && d.exp < 16; }

// bytes of the repr
SPX_HD int32_t length(const Decimal& d) {
  if (d.kind != kFinite) return d.kind == kNan ? 3 : 3 + d.neg;
  const int32_t e = d.exp, nd = d.nd;
  if (positional(d)) {
    if (e >= nd - 1) return d.neg + e + 3;  // digits, zeros, ".0"
    if (e < 0) return d.neg + 1 - e + nd;   // "0.", -e-1 zeros, digits
    return d.neg + nd + 1;
  }
  const int32_t a = e < 0 ? -e : e;
  return d.neg + nd + (nd > 1 ? 1 : 0) + 2 + (a >= 100 ? 3 : 2);
}

// digit i of the nd digits goes to out[i], or to out[i + 1] from the `point`-th on
template <class Byte>
SPX_HD void put_digits(Byte* out, uint64_t digits, int32_t nd, int32_t point) {
  uint32_t lo = (uint32_t)(digits % 1000000000u), hi = (uint32_t)(digits / 1000000000u);  // 9 + 8 digits
  int32_t i = nd - 1;
  for (int32_t n = 0; n < 9 && i >= 0; ++n, --i) {
    out[i + (i >= point ? 1 : 0)] = (Byte)('0' + lo % 10);
    lo /= 10;
  }
  for (; i >= 0; --i) {
    out[i + (i >= point ? 1 : 0)] = (Byte)('0' + hi % 10);
    hi /= 10;
  }
}

// the repr's bytes into out (length(d) of them, no terminator); returns the length
template <class Byte>
SPX_HD int32_t emit(const Decimal& d, Byte* out) {
  Byte* o = out;
  if (d.kind == kNan) {
    o[0] = 'n'; o[1] = 'a'; o[2] = 'n';
    return 3;
  }
  if (d.neg) *o++ = '-';
  if (d.kind == kInf) {
    o[0] = 'i'; o[1] = 'n'; o[2] = 'f';
    return 3 + d.neg;
  }
  const int32_t e = d.exp, nd = d.nd;
  if (positional(d)) {
    if (e >= nd - 1) {
      put_digits(o, d.digits, nd, nd);
      o += nd;
      for (int32_t i = nd - 1; i < e; ++i) *o++ = '0';
      *o++ = '.';
      *o++ = '0';
    } else if (e < 0) {
      *o++ = '0';
      *o++ = '.';
      for (int32_t i = -1; i > e; --i) *o++ = '0';
      put_digits(o, d.digits, nd, nd);
      o += nd;
    } else {
      put_digits(o, d.digits, nd, e + 1);
      o[e + 1] = '.';
      o += nd + 1;
    }
  } else {
    put_digits(o, d.digits, nd, 1);
    if (nd > 1) {
      o[1] = '.';
      o += nd + 1;
    } else {
      o += 1;
    }
    *o++ = 'e';
    *o++ = e < 0 ? '-' : '+';
    int32_t a = e < 0 ? -e : e;
    if (a >= 100) {
      *o++ = (Byte)('0' + a / 100);
      a %= 100;
    }
    *o++ = (Byte)('0' + a / 10);
    *o++ = (Byte)('0' + a % 10);
  }
  return (int32_t)(o - out);
}

// repr(x) into out (room for kMaxLen bytes, no terminator); returns the length
template <class Byte>
SPX_HD int32_t repr_f64(double x, Byte* out) {
  return emit(decompose(x), out);
}

}  // namespace spx_repr
