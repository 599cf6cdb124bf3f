// Host writer of MGF records whose peak lines are already text (spx_format_peaks'
// output copied back): formats only the record headers and "END IONS", copies each
// record's peak block verbatim, and writes the records in order.  Same three styles,
// flags and block-overlapped file writing as mgf_io.cpp's record writer, whose output
// it equals byte for byte; header floats come from repr_core.hpp.  Plain C++ (no HIP):
// built into libspecpride_hip.so by spx_api.hip, and into a stand-alone program by
// tools/host_emit_check.cpp.
#pragma once
#include <algorithm>
#include <charconv>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "repr_core.hpp"

namespace spx_splice {

struct Records {
  int style = 0;  // 0 binning, 1 gap-average, 2 medoid (mgf_io.cpp format_record)
  std::vector<const char*> tp;
  std::vector<size_t> tl;
  const int32_t* flags = nullptr;  // styles 1-2: bit0 PEPMASS, bit1 CHARGE, bit2 RTINSECONDS, bit3 TITLE
  const double* prec = nullptr;
  const int64_t* charge = nullptr;
  const double* rt = nullptr;
  const int64_t* text_off = nullptr;  // record c's peak lines: text[text_off[c] .. text_off[c + 1])
  const uint8_t* text = nullptr;
};

inline char* put(char* o, const char* s, size_t k) {
  std::memcpy(o, s, k);
  return o + k;
}
inline char* put_int(char* o, long long v) { return std::to_chars(o, o + 24, v).ptr; }
inline char* put_repr(char* o, double x) { return o + spx_repr::repr_f64(x, o); }

// "BEGIN IONS", 4 keys and their values, "END IONS": < 192 bytes besides the title
inline size_t record_cap(size_t title_len, int64_t text_bytes) { return 192 + title_len + (size_t)text_bytes; }

inline char* format_record(const Records& R, int64_t c, char* o) {
  const size_t tl = R.tl[(size_t)c];
  const char* t = R.tp[(size_t)c];
  const int32_t f = R.flags ? R.flags[c] : 0xf;
  o = put(o, "BEGIN IONS\n", 11);
  auto title = [&]() { o = put(o, "TITLE=", 6); o = put(o, t, tl); *o++ = '\n'; };
  auto pepmass = [&]() { o = put(o, "PEPMASS=", 8); o = put_repr(o, R.prec[c]); *o++ = '\n'; };
  auto rtsec = [&]() { o = put(o, "RTINSECONDS=", 12); o = put_repr(o, R.rt[c]); *o++ = '\n'; };
  auto charge = [&]() {  // |z| then the sign
    const int64_t z = R.charge[c];
    o = put(o, "CHARGE=", 7);
    o = put_int(o, z < 0 ? -z : z);
    *o++ = z < 0 ? '-' : '+';
    *o++ = '\n';
  };
  if (R.style == 0) {
    title();
    pepmass();
    o = put(o, "CHARGE=", 7);
    o = put_int(o, R.charge[c]);
    o = put(o, "+\n", 2);
  } else if (R.style == 1) {
    if ((f & 8) && tl > 0) title();
    if (f & 1) pepmass();
    if (f & 4) rtsec();
    if (f & 2) charge();
  } else {
    if (f & 8) title();
    if (f & 1) pepmass();
    if (f & 2) charge();
    if (f & 4) rtsec();
  }
  const int64_t a = R.text_off[c], b = R.text_off[c + 1];
  if (b > a) o = put(o, reinterpret_cast<const char*>(R.text) + a, (size_t)(b - a));
  return put(o, "END IONS\n\n", 10);
}

// '\n'-joined strings -> pointers and lengths (C entries)
inline void split_lines(const char* s, int64_t C, std::vector<const char*>& p, std::vector<size_t>& l) {
  p.resize((size_t)C);
  l.resize((size_t)C);
  for (int64_t c = 0; c < C; ++c) {
    const char* nl = std::strchr(s, '\n');
    p[(size_t)c] = s;
    l[(size_t)c] = nl ? (size_t)(nl - s) : std::strlen(s);
    s = nl ? nl + 1 : s + l[(size_t)c];
  }
}

// Records [0, C) built on T threads in blocks and written in order; the write of one
// round overlaps the building of the next.  0, or -1 on an I/O error.
inline int write_blocks(FILE* f, const Records& R, int64_t C, int T) {
  constexpr int64_t kBlock = 2048;
  std::vector<std::string> parts[2];
  parts[0].resize((size_t)T);
  parts[1].resize((size_t)T);
  std::thread writer;
  int rc = 0;
  int cur = 0;
  for (int64_t c0 = 0; c0 < C; c0 += kBlock * T, cur ^= 1) {
    std::vector<std::thread> pool;
    for (int t = 0; t < T; ++t) {
      pool.emplace_back([&, t, c0, cur]() {
        const int64_t a = std::min(C, c0 + t * kBlock), b = std::min(C, a + kBlock);
        std::string& out = parts[cur][(size_t)t];
        size_t cap = 0;
        for (int64_t c = a; c < b; ++c) cap += record_cap(R.tl[(size_t)c], R.text_off[c + 1] - R.text_off[c]);
        out.resize(cap);
        char* o = &out[0];
        for (int64_t c = a; c < b; ++c) o = format_record(R, c, o);
        out.resize((size_t)(o - out.data()));
      });
    }
    for (auto& th : pool) th.join();
    if (writer.joinable()) writer.join();
    writer = std::thread([&, cur]() {
      for (auto& s : parts[cur])
        if (!s.empty() && std::fwrite(s.data(), 1, s.size(), f) != s.size()) rc = -1;
    });
  }
  if (writer.joinable()) writer.join();
  return rc;
}

// The arguments of mgf_io.cpp's record writer with (text_off, text) in place of
// (off, mz, it).  Every argument is checked before the file is opened: -1 (and no
// file touched) on a bad one -- null arrays, a style outside 0..2, offsets that
// are negative or decrease.  -1 as well on an I/O error.
inline int write_records(const char* path, int append, int style, int64_t C, const char* titles,
                         const int32_t* flags, const double* prec, const int64_t* charge, const double* rt,
                         const int64_t* text_off, const uint8_t* text, int threads) {
  if (!path || C < 0 || style < 0 || style > 2 || (C > 0 && (!titles || !prec || !charge || !text_off)) ||
      (style != 0 && C > 0 && (!flags || !rt)))
    return -1;
  if (C > 0) {
    if (text_off[0] < 0 || (text_off[C] > 0 && !text)) return -1;
    for (int64_t c = 0; c < C; ++c)
      if (text_off[c + 1] < text_off[c]) return -1;
  }
  Records R;
  R.style = style;
  split_lines(titles ? titles : "", C, R.tp, R.tl);
  R.flags = flags;
  R.prec = prec;
  R.charge = charge;
  R.rt = rt;
  R.text_off = text_off;
  R.text = text;
  FILE* f = std::fopen(path, append ? "ab" : "wb");
  if (!f) return -1;
  const int T = threads > 0 ? threads : (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  int rc = write_blocks(f, R, C, T);
  if (std::fclose(f) != 0) rc = -1;
  return rc;
}

}  // namespace spx_splice
