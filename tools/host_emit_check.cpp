// Stand-alone check of the host half of the device-side MGF emit, meant to be built
// with the sanitizers (it links nothing of HIP):
//
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o host_emit_check tools/host_emit_check.cpp && ./host_emit_check
//
// It runs csrc/repr_core.hpp over the doubles that reach its corners (every power of
// two and its neighbours, subnormals, the layout thresholds, random bit patterns),
// checking that each repr is at most 24 bytes, has the length the core predicts and
// reads back (strtod) as the same double; then csrc/mgf_splice.hpp over a few hundred
// records in the three styles with several threads, plain and append, checking the
// file against the same records assembled in memory.  Exit status 0 = all held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../specpride_amd/csrc/mgf_splice.hpp"

static int g_fail = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      std::fprintf(stderr, __VA_ARGS__); \
      std::fprintf(stderr, "\n");   \
      ++g_fail;                     \
    }                               \
  } while (0)

static void check_value(double x) {
  char buf[spx_repr::kMaxLen + 1];
  std::memset(buf, '#', sizeof(buf));
  const spx_repr::Decimal d = spx_repr::decompose(x);
  const int n = spx_repr::emit(d, buf);
  CHECK(n >= 1 && n <= spx_repr::kMaxLen && n == spx_repr::length(d), "length of %a: %d", x, n);
  CHECK(buf[spx_repr::kMaxLen] == '#', "wrote past 24 bytes for %a", x);
  buf[n] = 0;
  const double back = std::strtod(buf, nullptr);
  uint64_t a, b;
  std::memcpy(&a, &x, 8);
  std::memcpy(&b, &back, 8);
  if (std::isnan(x)) CHECK(std::strcmp(buf, "nan") == 0, "nan -> %s", buf);
  else CHECK(a == b, "%a -> %s reads back as %a", x, buf, back);
}

static std::string slurp(const char* path) {
  std::string s;
  if (FILE* f = std::fopen(path, "rb")) {
    char tmp[1 << 16];
    size_t k;
    while ((k = std::fread(tmp, 1, sizeof(tmp), f)) > 0) s.append(tmp, k);
    std::fclose(f);
  }
  return s;
}

int main() {
  // ---- the digit core
  for (int e = -1074; e <= 1023; ++e) {
    const double p = std::ldexp(1.0, e);
    check_value(p);
    check_value(std::nextafter(p, INFINITY));
    check_value(std::nextafter(p, -INFINITY));
    check_value(-p);
  }
  const double listed[] = {0.0, -0.0, 1e-5, 9.999e-5, 1e-4, 0.001, 1e15, 9999999999999998.0, 1e16, 1e17, 1e21, 1e22,
                           1e23, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 0.1, 0.3, 2.0 / 3.0,
                           123456789012345680.0, NAN, INFINITY, -INFINITY, -2.2250738585072014e-308};
  for (double x : listed) check_value(x);
  std::mt19937_64 rng(7);
  for (int i = 0; i < 200000; ++i) {
    const uint64_t u = rng();
    double x;
    std::memcpy(&x, &u, 8);
    check_value(x);
    check_value(50.0 + (double)(u >> 11) * (2950.0 / 9007199254740992.0));
  }

  // ---- the splicing writer
  const int64_t C = 300;
  std::vector<double> prec(C), rt(C);
  std::vector<int64_t> charge(C), text_off(C + 1, 0);
  std::vector<int32_t> flags(C);
  std::string titles, text;
  std::vector<std::string> title(C), block(C);
  for (int64_t c = 0; c < C; ++c) {
    title[c] = "cluster-" + std::to_string(c % 17) + ";scan:" + std::to_string(c);
    titles += title[c];
    if (c + 1 < C) titles += '\n';
    prec[c] = 300.0 + (double)(rng() % 1000000) / 977.0;
    rt[c] = (double)(rng() % 7200000) / 1000.0;
    charge[c] = (int64_t)(rng() % 7) - 2;
    flags[c] = (int32_t)(c % 16);
    const int np = c % 5 == 2 ? 0 : (int)(rng() % 30);
    for (int k = 0; k < np; ++k) {
      char line[64];
      char* o = line;
      o += spx_repr::repr_f64(100.0 + (double)(rng() % 1900000) / 1000.0, o);
      *o++ = ' ';
      o += spx_repr::repr_f64(std::ldexp((double)(rng() % 100000), (int)(rng() % 40) - 20), o);
      *o++ = '\n';
      block[c].append(line, (size_t)(o - line));
    }
    text += block[c];
    text_off[c + 1] = (int64_t)text.size();
  }
  const char* path = "host_emit_check.out.mgf";
  for (int style = 0; style < 3; ++style) {
    std::string want;
    for (int64_t c = 0; c < C; ++c) {
      char num[32];
      const int f = flags[c];
      std::string pep = "PEPMASS=" + std::string(num, (size_t)spx_repr::repr_f64(prec[c], num)) + "\n";
      std::string rts = "RTINSECONDS=" + std::string(num, (size_t)spx_repr::repr_f64(rt[c], num)) + "\n";
      const int64_t z = charge[c];
      std::string chg = "CHARGE=" + std::to_string(z < 0 ? -z : z) + (z < 0 ? "-" : "+") + "\n";
      want += "BEGIN IONS\n";
      if (style == 0) want += "TITLE=" + title[c] + "\n" + pep + "CHARGE=" + std::to_string(z) + "+\n";
      else if (style == 1) want += ((f & 8) ? "TITLE=" + title[c] + "\n" : "") + ((f & 1) ? pep : "") +
                                   ((f & 4) ? rts : "") + ((f & 2) ? chg : "");
      else want += ((f & 8) ? "TITLE=" + title[c] + "\n" : "") + ((f & 1) ? pep : "") + ((f & 2) ? chg : "") +
                   ((f & 4) ? rts : "");
      want += block[c] + "END IONS\n\n";
    }
    for (int threads : {1, 4}) {
      std::remove(path);
      const uint8_t* tx = reinterpret_cast<const uint8_t*>(text.data());
      int rc = spx_splice::write_records(path, 0, style, C, titles.c_str(), flags.data(), prec.data(), charge.data(),
                                         rt.data(), text_off.data(), tx, threads);
      CHECK(rc == 0 && slurp(path) == want, "style %d, %d threads: file differs", style, threads);
      rc = spx_splice::write_records(path, 1, style, C, titles.c_str(), flags.data(), prec.data(), charge.data(),
                                     rt.data(), text_off.data(), tx, threads);
      CHECK(rc == 0 && slurp(path) == want + want, "style %d, %d threads: append differs", style, threads);
    }
  }
  std::remove(path);
  // bad arguments leave no file behind
  text_off[5] = text_off[4] - 1;
  CHECK(spx_splice::write_records(path, 0, 0, C, titles.c_str(), flags.data(), prec.data(), charge.data(), rt.data(),
                                  text_off.data(), reinterpret_cast<const uint8_t*>(text.data()), 2) == -1,
        "decreasing offsets accepted");
  CHECK(slurp(path).empty(), "a rejected call wrote a file");
  std::printf("host_emit_check: %s\n", g_fail ? "FAILED" : "ok");
  return g_fail ? 1 : 0;
}
