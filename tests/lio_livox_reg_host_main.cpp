// Stand-alone driver of the LIO-Livox ScanRegistration host code
// (csrc/slio_llreg.cpp with the formulas of csrc/slio_llreg.hpp) for
// tests/test_lio_livox_reg_cpu.py, which builds it with
// -fsanitize=address,undefined and runs it as a child process.  The messages are
// scan-like curves over two walls with a step between them, dealt to the lines
// in turn, at the sizes where the loops start to run, at the part counts 1,
// 100 and 150 with m - 11 one below, at and one above them, with non-finite
// points, repeated points, points the x filters drop, a zero time span and the
// 20000-point limit of a line.  Every output buffer is allocated at exactly
// the size the entry promises to stay within, so a write past it is the
// sanitizer's to find.  Exits 0 when every call returned what it should.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "slio.h"
#include "slio_frontend.h"

namespace slio {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace slio

static int fails = 0;
#define EXPECT(c)                                          \
  do {                                                     \
    if (!(c)) {                                            \
      std::printf("line %d: %s\n", __LINE__, #c);          \
      ++fails;                                             \
    }                                                      \
  } while (0)

struct Msg {
  std::vector<float> xyz;
  std::vector<uint8_t> refl, line;
  std::vector<uint32_t> ot;
  int64_t n() const { return (int64_t)line.size(); }
};

// n returns along a Lissajous curve over a wall at x = 8 and, for rays to the
// left, a wall at x = 12, dealt to n_lines lines in turn
static Msg curve(int n, int n_lines) {
  Msg m;
  for (int i = 0; i < n; ++i) {
    const double az = 0.6 * std::sin(0.003 * i), el = -0.05 + 0.2 * std::sin(0.0171 * i);
    const double wall = az > 0.2 ? 12.0 : 8.0;
    const double r = wall / (std::cos(el) * std::cos(az)) + 0.002 * std::sin(12.9898 * i);
    m.xyz.push_back((float)(r * std::cos(el) * std::cos(az)));
    m.xyz.push_back((float)(r * std::cos(el) * std::sin(az)));
    m.xyz.push_back((float)(r * std::sin(el)));
    m.refl.push_back((uint8_t)(i * 37 % 256));
    m.line.push_back((uint8_t)(i % n_lines));
    m.ot.push_back((uint32_t)(1000 * (i + 1)));
  }
  return m;
}

static slio_llreg_params params(int n_scans, int part_num, int lidar_type = 0) {
  slio_llreg_params p;
  EXPECT(slio_llreg_params_default(&p) == SLIO_OK);
  p.n_scans = n_scans;
  p.part_num = part_num;
  p.lidar_type = lidar_type;
  return p;
}

// the Pc2 runs put NaN and infinite intensities into the cloud (only x, y and z are tested for finiteness)
static bool g_bad_intensity = false;

// one run with every output at its promised size; want_cloud < 0: not checked
static void run(const slio_llreg_params& p, const Msg& m, bool pc2, int want_cloud, int want_rc = SLIO_OK) {
  const size_t n = (size_t)m.n();
  std::vector<float> cloud(8 * n), corner(8 * n), surf(8 * n), lines(4 * n), xyzi(4 * n);
  std::vector<int32_t> flags(n);
  std::vector<uint8_t> vis(n);
  int32_t counts[3] = {-1, -1, -1}, ls[6], fs[6];
  for (size_t i = 0; i < n; ++i) {
    std::memcpy(&xyzi[4 * i], &m.xyz[3 * i], 12);
    xyzi[4 * i + 3] = (float)m.refl[i];
    if (g_bad_intensity && i % 97 < 9 && i % 4 == 0) xyzi[4 * i + 3] = i % 8 ? NAN : (i % 16 ? INFINITY : -INFINITY);
  }
  const int rc = pc2 ? slio_llreg_extract_pc2_host(&p, xyzi.data(), (int64_t)n, cloud.data(), corner.data(),
                                                   surf.data(), counts, ls, fs, flags.data(), vis.data(), lines.data())
                     : slio_llreg_extract_host(&p, m.xyz.data(), m.refl.data(), m.line.data(), m.ot.data(), (int64_t)n,
                                               cloud.data(), corner.data(), surf.data(), counts, ls, fs, flags.data(),
                                               vis.data(), lines.data());
  EXPECT(rc == want_rc);
  if (rc != SLIO_OK) return;
  EXPECT(counts[0] >= 0 && counts[0] <= (int)n && counts[1] >= 0 && counts[2] >= 0 &&
         counts[1] + counts[2] <= counts[0]);
  if (want_cloud >= 0) EXPECT(counts[0] == want_cloud);
  int sum_l = 0, sum_f = 0;
  for (int l = 0; l < 6; ++l) {
    EXPECT(fs[l] >= 0 && fs[l] <= ls[l] && ls[l] <= 20000);
    if (l >= p.n_scans) EXPECT(ls[l] == 0);
    sum_l += ls[l];
    sum_f += fs[l];
  }
  EXPECT(sum_l == counts[0]);
  int off = 0, nc = 0, ns = 0;
  for (int l = 0; l < 6; ++l) {
    for (int i = 0; i < fs[l]; ++i) {
      const int f = flags[off + i];
      EXPECT(f == 0 || f == 1 || f == 2 || f == 3 || f == 300 || f == 100 || f == 101 || f == 150);
      if (vis[off + i]) EXPECT(i >= 5 && i < fs[l] - 5);
    }
    EXPECT(fs[l] <= 10 || vis[off + 5] == 1);
    off += fs[l];
  }
  EXPECT(off == sum_f);
  for (int i = 0; i < counts[0]; ++i) {
    const float lab = cloud[8 * i + 6];
    EXPECT(lab == 0.f || lab == 1.f || lab == 2.f);
    nc += lab == 1.f;
    ns += lab == 2.f;
    EXPECT(cloud[8 * i + 7] == 0.f);
  }
  EXPECT(nc == counts[1] && ns == counts[2]);
  // every output optional
  int32_t again[3];
  const int rc2 = pc2 ? slio_llreg_extract_pc2_host(&p, xyzi.data(), (int64_t)n, nullptr, nullptr, nullptr, again,
                                                    nullptr, nullptr, nullptr, nullptr, nullptr)
                      : slio_llreg_extract_host(&p, m.xyz.data(), m.refl.data(), m.line.data(), m.ot.data(),
                                                (int64_t)n, nullptr, nullptr, nullptr, again, nullptr, nullptr,
                                                nullptr, nullptr, nullptr);
  EXPECT(rc2 == SLIO_OK && std::memcmp(again, counts, sizeof again) == 0);
}

int main() {
  // per-line sizes 0, 1, 10, 11, 12 and the sizes around the part counts, one line
  for (int pn : {1, 100, 150})
    for (int m : {0, 1, 10, 11, 12, pn + 10, pn + 11, pn + 12, 700}) run(params(1, pn), curve(m, 1), false, m);
  // six, four and one line used of six present; an absent line; the Pc2 path
  for (int ns : {1, 4, 6}) run(params(ns, 150), curve(3000, 6), false, -1);
  {
    Msg m = curve(3000, 6);
    for (auto& l : m.line)
      if (l == 3) l = 4;
    run(params(6, 150), m, false, 3000);
    run(params(4, 100, 2), m, true, 3000);
    run(params(6, 100, 0), m, true, 3000);
    run(params(3, 100), m, true, -1, SLIO_EINVAL);
  }
  // non-finite intensities on the Pc2 path, parts short and long
  {
    g_bad_intensity = true;
    const Msg m = curve(3000, 4);
    for (int pn : {1, 3, 100}) run(params(4, pn, 2), m, true, 3000);
    g_bad_intensity = false;
  }
  // non-finite points at the start, at the end and in runs; x the filters drop; NaN x passes them
  for (int type : {0, 1, 2}) {
    Msg m = curve(2400, 4);
    for (int i : {0, 1, 2, 3, 400, 401, 402, 403, 404, 405, 2396, 2397, 2398, 2399})
      m.xyz[3 * i + i % 3] = i % 2 ? NAN : INFINITY;
    for (int i = 800; i < 900; ++i) m.xyz[3 * i] = -m.xyz[3 * i];
    m.xyz[3 * 1000] = 0.005f;
    m.xyz[3 * 1001] = -0.005f;
    run(params(4, 100, type), m, false, type == 2 ? 2398 : 2298);
    run(params(4, 100, type), m, true, type == 2 ? 2398 : 2298);
  }
  // repeated points (zero vectors, 0 / 0 in the ray angles) and a zero time span
  {
    Msg m = curve(900, 2);
    for (int a = 100; a < 140; ++a) std::memcpy(&m.xyz[3 * (a + 2)], &m.xyz[3 * a], 12);
    run(params(2, 150), m, false, 900);
    for (auto& t : m.ot) t = 0;
    run(params(2, 150), m, false, 900);
    for (auto& t : m.ot) t = 4000000000u;  // four seconds: sec and nsec both non-zero
    run(params(2, 150), m, false, 900);
  }
  // the limit of a line
  {
    Msg m = curve(20001, 1);
    run(params(1, 150), m, false, -1, SLIO_ECAPACITY);
    m.line[7] = 1;
    run(params(2, 150), m, false, 20001);
    run(params(1, 1), curve(20000, 1), false, 20000);
  }
  // argument errors and the small entries
  {
    const Msg m = curve(16, 1);
    int32_t counts[3], a = 0, b = 0, c = 0, d = 0;
    slio_llreg_params p = params(1, 150);
    EXPECT(slio_llreg_extract_host(nullptr, m.xyz.data(), m.refl.data(), m.line.data(), m.ot.data(), 16, nullptr,
                                   nullptr, nullptr, counts, nullptr, nullptr, nullptr, nullptr, nullptr) ==
           SLIO_EINVAL);
    EXPECT(slio_llreg_extract_host(&p, nullptr, m.refl.data(), m.line.data(), m.ot.data(), 16, nullptr, nullptr,
                                   nullptr, counts, nullptr, nullptr, nullptr, nullptr, nullptr) == SLIO_EINVAL);
    EXPECT(slio_llreg_extract_host(&p, m.xyz.data(), m.refl.data(), m.line.data(), m.ot.data(), -1, nullptr, nullptr,
                                   nullptr, counts, nullptr, nullptr, nullptr, nullptr, nullptr) == SLIO_EINVAL);
    EXPECT(slio_llreg_extract_host(&p, m.xyz.data(), m.refl.data(), m.line.data(), m.ot.data(), 16, nullptr, nullptr,
                                   nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SLIO_EINVAL);
    p.part_num = 0;
    EXPECT(slio_llreg_extract_host(&p, m.xyz.data(), m.refl.data(), m.line.data(), m.ot.data(), 16, nullptr, nullptr,
                                   nullptr, counts, nullptr, nullptr, nullptr, nullptr, nullptr) == SLIO_EINVAL);
    EXPECT(slio_llreg_tiles(&a, &b, &c, &d) == SLIO_OK && a >= 4 && b >= 20000 && b % a == 0 && c >= 1 && c <= 58);
    EXPECT(slio_llreg_tiles(nullptr, &b, &c, &d) == SLIO_EINVAL);
    EXPECT(slio_llreg_params_default(nullptr) == SLIO_EINVAL);
  }

  std::printf(fails ? "FAILED %d\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
