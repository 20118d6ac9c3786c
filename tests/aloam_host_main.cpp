// Stand-alone driver of the A-LOAM scanRegistration host code
// (csrc/slio_aloam.cpp with the formulas of csrc/slio_aloam.hpp) for
// tests/test_aloam_cpu.py, which builds it with -fsanitize=address,undefined
// and runs it as a child process.  The clouds are spinning sweeps over a wavy
// wall for the three layouts, cut to the sizes at which the loops start to
// run, with non-finite points, points nearer than the range limit, points
// outside the layout, repeated points, a scan that is the whole cloud and a
// scan whose VoxelGrid overflows.  Every output buffer is allocated at exactly
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

// cols firings of the beams at elev0 + k * step degrees, clockwise, on a wavy wall with steps
static std::vector<float> sweep(int cols, int beams, double elev0, double step) {
  std::vector<float> c;
  for (int i = 0; i < cols; ++i)
    for (int k = 0; k < beams; ++k) {
      const double az = M_PI - (i + 0.3 * std::sin(1.3 * i + k)) * (2 * M_PI / cols);
      const double el = (elev0 + step * k + 0.02 * std::sin(7.1 * i + k)) * M_PI / 180;
      const double r = 12 * (1 + 0.2 * std::sin(5 * az) + 0.1 * (std::sin(23 * az + k) > 0.5)) +
                       0.004 * std::sin(12.9898 * (i * beams + k));
      c.push_back((float)(r * std::cos(el) * std::cos(az)));
      c.push_back((float)(r * std::cos(el) * std::sin(az)));
      c.push_back((float)(r * std::sin(el)));
    }
  return c;
}

static void run(const std::vector<float>& c, int64_t n, int n_scans, int want_n, int32_t* stats_out = nullptr) {
  slio_aloam_params p;
  EXPECT(slio_aloam_params_default(&p) == SLIO_OK);
  p.n_scans = n_scans;
  p.max_points = (int32_t)(n > 0 ? n : 1);
  const size_t m = (size_t)n;
  std::vector<float> cl[5];
  for (auto& v : cl) v.resize(4 * m);
  std::vector<int32_t> start((size_t)n_scans), end((size_t)n_scans), label(m);
  std::vector<float> curv(m);
  std::vector<uint8_t> picked(m);
  int32_t counts[5] = {-1, -1, -1, -1, -1}, stats[18];
  EXPECT(slio_aloam_register_host(&p, c.data(), n, cl[0].data(), cl[1].data(), cl[2].data(), cl[3].data(),
                                  cl[4].data(), start.data(), end.data(), curv.data(), label.data(), picked.data(),
                                  counts, stats) == SLIO_OK);
  EXPECT(counts[0] <= n && counts[1] <= counts[2] && counts[2] <= counts[0] && counts[3] <= counts[0] &&
         counts[4] <= counts[0]);
  EXPECT(counts[0] == n - stats[0] - stats[1] - stats[2]);
  if (want_n >= 0) EXPECT(counts[0] == want_n);
  EXPECT(counts[1] <= 12 * n_scans && counts[2] <= 120 * n_scans && counts[3] <= 24 * n_scans);
  EXPECT(counts[3] == stats[13]);
  int prev = 0;
  for (int s = 0; s < n_scans; ++s) {
    EXPECT(start[s] == prev + 5 && end[s] >= start[s] - 11);
    prev = end[s] + 6;
  }
  EXPECT(prev == counts[0]);
  for (int i = 0; i < counts[0]; ++i) {
    EXPECT(label[i] >= -1 && label[i] <= 2 && picked[i] <= 1);
    EXPECT((int)cl[0][4 * i + 3] >= 0 && (int)cl[0][4 * i + 3] < n_scans);
  }
  // every output optional
  int32_t again[5];
  EXPECT(slio_aloam_register_host(&p, c.data(), n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, again, nullptr) == SLIO_OK);
  EXPECT(std::memcmp(again, counts, sizeof again) == 0);
  if (stats_out) std::memcpy(stats_out, stats, sizeof stats);
}

int main() {
  const std::vector<float> v16 = sweep(400, 16, -15, 2);
  for (int n : {0, 1, 5, 10, 11, 12, 16 * 16, 16 * 17, 16 * 18, 16 * 23, 1000, 6400}) run(v16, n, 16, n);
  int32_t st[18];
  run(v16, 6400, 16, 6400, st);
  EXPECT(st[12] > 0 && st[13] > 0 && st[14] > 0 && st[15] > 0);  // both breaks, flats, marks across a seam
  // 32 lines centred in the bins; 64 lines: the lower block's beams above id 50 are dropped
  run(sweep(150, 32, -92.0 / 3.0 + 2.0 / 3.0, 4.0 / 3.0), 150 * 32, 32, 150 * 32);
  {
    std::vector<float> c = sweep(100, 33, 2 - 32 / 3.0, 1 / 3.0), lo = sweep(100, 31, -8.83 - 15.5, 0.5);
    c.insert(c.end(), lo.begin(), lo.end());
    run(c, 6400, 64, -1, st);
    EXPECT(st[3] > 0 && st[2] >= st[3]);
  }
  // non-finite points at the start, the end and in runs; points too close; points outside the layout
  {
    std::vector<float> c(v16.begin(), v16.begin() + 3 * 2000);
    for (int i : {0, 1, 2, 100, 101, 102, 103, 255, 256, 257, 1997, 1998, 1999}) c[3 * i + i % 3] = i % 2 ? NAN : INFINITY;
    for (int i = 500; i < 520; ++i) c[3 * i] = c[3 * i + 1] = c[3 * i + 2] = 0.01f;
    for (int i = 900; i < 930; ++i) c[3 * i + 2] = 40.0f;
    run(c, 2000, 16, 2000 - 13 - 20 - 30, st);
    EXPECT(st[0] == 13 && st[1] == 20 && st[2] == 30);
    for (int i = 0; i < 2000; ++i) c[3 * i + 1] = -INFINITY;
    run(c, 2000, 16, 0);
    std::vector<float> high(3 * 64);
    for (int i = 0; i < 64; ++i) high[3 * i] = 1.0f, high[3 * i + 1] = 0.1f * i, high[3 * i + 2] = 30.0f;
    run(high, 64, 16, 0);
    std::vector<float> zeros(3 * 64, 0.0f);
    run(zeros, 64, 16, 0);
    slio_aloam_params p;
    slio_aloam_params_default(&p);
    p.minimum_range = 0.0;  // the points at the origin survive the filters: a NaN elevation is dropped
    int32_t counts[5];
    EXPECT(slio_aloam_register_host(&p, zeros.data(), 64, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, nullptr, counts, st) == SLIO_OK);
    EXPECT(counts[0] == 0 && st[2] == 64);
  }
  // repeated points; one scan that is the whole cloud
  {
    std::vector<float> c = sweep(3000, 1, 1.0, 0);
    for (int a = 300; a < 330; ++a) std::memcpy(&c[3 * (a + 1)], &c[3 * a], 12);
    run(c, 3000, 16, 3000, st);
    EXPECT(st[11] == 15);
  }
  // a scan whose less-flat points span more voxels than an int counts
  {
    std::vector<float> c;
    for (int k = 0; k < 200; ++k) {
      const double az = M_PI - k * (M_PI / 200), el = (1.0 + 0.4 * std::sin(1.7 * k)) * M_PI / 180, r = 1838.0;
      c.push_back((float)(r * std::cos(az)));
      c.push_back((float)(r * std::sin(az)));
      c.push_back((float)(r * std::tan(el)));
    }
    run(c, 200, 16, 200, st);
    EXPECT(st[17] == 1);
  }
  // argument errors and the small entries
  {
    slio_aloam_params p;
    int32_t counts[5], a = 0, b = 0;
    EXPECT(slio_aloam_params_default(&p) == SLIO_OK && p.n_scans == 16 && p.max_points == 400000 &&
           p.minimum_range == 0.1 && p.scan_period == 0.1);
    EXPECT(slio_aloam_params_default(nullptr) == SLIO_EINVAL);
    EXPECT(slio_aloam_register_host(nullptr, v16.data(), 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, nullptr, nullptr, counts, nullptr) == SLIO_EINVAL);
    EXPECT(slio_aloam_register_host(&p, nullptr, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, nullptr, counts, nullptr) == SLIO_EINVAL);
    EXPECT(slio_aloam_register_host(&p, v16.data(), -1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, nullptr, counts, nullptr) == SLIO_EINVAL);
    EXPECT(slio_aloam_register_host(&p, v16.data(), 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, nullptr, nullptr, nullptr) == SLIO_EINVAL);
    p.n_scans = 48;
    EXPECT(slio_aloam_register_host(&p, v16.data(), 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, nullptr, counts, nullptr) == SLIO_EINVAL);
    p.n_scans = 16;
    p.max_points = 3;
    EXPECT(slio_aloam_register_host(&p, v16.data(), 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, nullptr, counts, nullptr) == SLIO_ECAPACITY);
    EXPECT(slio_aloam_tile(&a, &b) == SLIO_OK && a >= 64 && b >= a);
    EXPECT(slio_aloam_tile(nullptr, &b) == SLIO_EINVAL);
  }

  std::printf(fails ? "FAILED %d\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
