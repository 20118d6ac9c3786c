// Stand-alone driver of the scanRegistration host code (csrc/slio_lreg.cpp with
// the formulas of csrc/slio_lreg.hpp) for tests/test_livox_reg_cpu.py, which
// builds it with -fsanitize=address,undefined and runs it as a child process.
// The clouds are a scan-like curve over two walls with a step between them,
// cut to the sizes at which the loops start to run and to the 32000-point
// limit, with non-finite points, repeated points and points on the axes.
// Every output buffer is allocated at exactly the size the entry promises to
// stay within, so a write past it is the sanitizer's to find.  Exits 0 when
// every call returned what it should.
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

// n returns along a Lissajous curve over a wall at x = 8 and, for rays to the
// left, a wall at x = 12: steps in depth, flat stretches, and a little ripple
static std::vector<float> curve(int n) {
  std::vector<float> c(4 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    const double az = 0.6 * std::sin(0.003 * i), el = -0.05 + 0.2 * std::sin(0.0171 * i);
    const double wall = az > 0.2 ? 12.0 : 8.0;
    const double r = wall / (std::cos(el) * std::cos(az)) + 0.002 * std::sin(12.9898 * i);
    c[4 * i] = (float)(r * std::cos(el) * std::cos(az));
    c[4 * i + 1] = (float)(r * std::cos(el) * std::sin(az));
    c[4 * i + 2] = (float)(r * std::sin(el));
    c[4 * i + 3] = (float)(i % 200);
  }
  return c;
}

static void run(const std::vector<float>& c, int64_t n, int want_n) {
  const int cap = (int)(n < 32000 ? n : 32000);
  std::vector<int32_t> flags((size_t)cap);
  std::vector<uint8_t> vis((size_t)cap);
  std::vector<float> cloud(4 * (size_t)cap), corner(4 * (size_t)cap), surf(4 * (size_t)cap);
  int32_t counts[3] = {-1, -1, -1}, stats[12];
  EXPECT(slio_lreg_classify_host(c.data(), n, flags.data(), vis.data(), cloud.data(), corner.data(), surf.data(),
                                 counts, stats) == SLIO_OK);
  EXPECT(counts[0] <= cap && counts[1] >= 0 && counts[2] >= 0 && counts[1] + counts[2] <= counts[0]);
  if (want_n >= 0) EXPECT(counts[0] == want_n);
  int nv = 0;
  for (int i = 0; i < counts[0]; ++i) {
    EXPECT(flags[i] == 0 || flags[i] == 1 || flags[i] == 100 || flags[i] == 150 || flags[i] == 250);
    if (vis[i]) {
      EXPECT(i >= 5 && i < counts[0] - 5);
      ++nv;
    }
  }
  EXPECT(nv == stats[0] + stats[1]);
  EXPECT(counts[0] <= 10 ? nv == 0 : vis[5] == 1);
  // every output optional
  int32_t again[3];
  EXPECT(slio_lreg_classify_host(c.data(), n, nullptr, nullptr, nullptr, nullptr, nullptr, again, nullptr) == SLIO_OK);
  EXPECT(std::memcmp(again, counts, sizeof again) == 0);
}

int main() {
  const std::vector<float> base = curve(33000);
  for (int n : {0, 1, 10, 11, 12, 15, 16, 63, 64, 65, 69, 70, 255, 256, 257, 2300}) run(base, n, n);
  for (int n : {32000, 32001, 33000}) run(base, n, 32000);

  // non-finite points: at the start, at the end, in runs, and nothing else
  {
    std::vector<float> c(base.begin(), base.begin() + 4 * 700);
    for (int i : {0, 1, 2, 100, 101, 102, 103, 255, 256, 257, 697, 698, 699}) c[4 * i + i % 3] = i % 2 ? NAN : INFINITY;
    run(c, 700, 700 - 13);
    for (int i = 0; i < 700; ++i) c[4 * i + 1] = -INFINITY;
    run(c, 700, 0);
  }
  // a cut inside the limit that only non-finite points shorten
  {
    std::vector<float> c = base;
    for (int i : {17, 31999, 32000, 32500}) c[4 * i] = NAN;
    run(c, 33000, 32000 - 2);
  }
  // repeated points (zero vectors in normalize) and points on the axes
  {
    std::vector<float> c(base.begin(), base.begin() + 4 * 400);
    for (int a = 30; a < 45; ++a) std::memcpy(&c[4 * (a + 1)], &c[4 * a], 16);
    const float ax[4][3] = {{0, 2, 0}, {0, -2, 0}, {0, 0, 3}, {0, 0, -3}};
    for (int k = 0; k < 4; ++k) std::memcpy(&c[4 * (100 + 8 * k)], ax[k], 12);
    std::vector<float> cloud(4 * 400);
    int32_t counts[3];
    EXPECT(slio_lreg_classify_host(c.data(), 400, nullptr, nullptr, cloud.data(), nullptr, nullptr, counts, nullptr) ==
           SLIO_OK);
    const int want_id[4] = {30, 9, 20, 40};
    for (int k = 0; k < 4; ++k) EXPECT((int)cloud[4 * (100 + 8 * k) + 3] == want_id[k]);
    for (int i = 0; i < 4 * 400; ++i) EXPECT(std::isfinite(cloud[i]));
    run(c, 400, 400);
    std::vector<float> zeros(4 * 64, 0.0f);
    run(zeros, 64, 64);
  }

  // plane_judge: a line, a plane, a ball, the size limits
  {
    float line[12], plane[15] = {0, 0, 2, 1, 0, 2, 0, 1, 2, 1, 1, 2, 0.5f, 0.2f, 2}, big[3 * 64];
    for (int j = 0; j < 4; ++j) {
      line[3 * j] = 3.0f + 0.3f * j;
      line[3 * j + 1] = 1.0f - 0.2f * j;
      line[3 * j + 2] = 0.5f + 0.1f * j;
    }
    for (int j = 0; j < 3 * 64; ++j) big[j] = std::sin(1.7f * j) * (1 + j % 5);
    int32_t is = -1;
    EXPECT(slio_lreg_plane_judge(line, 4, 100, &is) == SLIO_OK && is == 1);
    EXPECT(slio_lreg_plane_judge(plane, 5, 100, &is) == SLIO_OK && is == 0);
    EXPECT(slio_lreg_plane_judge(big, 64, 100, &is) == SLIO_OK && is == 0);
    EXPECT(slio_lreg_plane_judge(line, 1, 100, &is) == SLIO_OK && is == 0);
    EXPECT(slio_lreg_plane_judge(big, 65, 100, &is) == SLIO_EINVAL);
    EXPECT(slio_lreg_plane_judge(line, 0, 100, &is) == SLIO_EINVAL);
    EXPECT(slio_lreg_plane_judge(nullptr, 4, 100, &is) == SLIO_EINVAL);
    EXPECT(slio_lreg_plane_judge(line, 4, 100, nullptr) == SLIO_EINVAL);
  }

  // argument errors and the small entries
  {
    int32_t counts[3], a = 0, b = 0;
    EXPECT(slio_lreg_classify_host(nullptr, 4, nullptr, nullptr, nullptr, nullptr, nullptr, counts, nullptr) ==
           SLIO_EINVAL);
    EXPECT(slio_lreg_classify_host(base.data(), -1, nullptr, nullptr, nullptr, nullptr, nullptr, counts, nullptr) ==
           SLIO_EINVAL);
    EXPECT(slio_lreg_classify_host(base.data(), 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
           SLIO_EINVAL);
    EXPECT(slio_lreg_chain_tile(&a, &b) == SLIO_OK && a >= 4 && b >= 32000 && b % a == 0);
    EXPECT(slio_lreg_chain_tile(nullptr, &b) == SLIO_EINVAL);
    slio_lreg_params p;
    EXPECT(slio_lreg_params_default(&p) == SLIO_OK && p.device == 0 && p.max_points == 32000);
    EXPECT(slio_lreg_params_default(nullptr) == SLIO_EINVAL);
  }

  std::printf(fails ? "FAILED %d\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
