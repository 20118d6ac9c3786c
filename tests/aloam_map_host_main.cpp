// Stand-alone driver of the A-LOAM laserMapping host code
// (csrc/slio_aloam_map.cpp with the formulas of csrc/slio_aloam_map.hpp) for
// tests/test_aloam_map_cpu.py, which builds it with
// -fsanitize=address,undefined and runs it as a child process.  The scene is a
// patch of ground with three poles seen from poses that drift and then jump far
// enough for every shift loop to run; the clouds are cut to the sizes at which
// the loops start to run (0, 1, 4, 5 and 6 map points, an empty class), with
// coincident, collinear and non-finite points; every buffer is allocated at
// exactly the size the entry promises to stay within, so a write past it is the
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

static void push(std::vector<float>& c, double x, double y, double z) {
  c.push_back((float)x);
  c.push_back((float)y);
  c.push_back((float)z);
  c.push_back(0.f);
}

// n points up three poles / on a patch of ground, seen from a sensor at (dx, 0, 0)
static std::vector<float> poles(int n, double dx) {
  std::vector<float> c;
  const double at[3][2] = {{3, 2}, {-4, 5}, {6, -3}};
  for (int i = 0; i < n; ++i) push(c, at[i % 3][0] - dx, at[i % 3][1], -1.0 + 0.05 * (i / 3));
  return c;
}
static std::vector<float> ground(int n, double dx) {
  std::vector<float> c;
  for (int i = 0; i < n; ++i) push(c, -6.0 + 0.45 * (i % 28) - dx, -6.0 + 0.45 * (i / 28), -1.7 + 0.01 * std::sin(i));
  return c;
}
static int64_t pts(const std::vector<float>& c) { return (int64_t)(c.size() / 4); }

static void check_state(slio_aloam_map_host_handle h, const slio_aloam_map_result& r) {
  int64_t n = 0, total[2] = {0, 0};
  for (int kind = 0; kind < 2; ++kind) {
    EXPECT(slio_aloam_map_host_get_stack(h, kind, nullptr, 0, &n) == SLIO_OK && n == r.stack_size[kind]);
    std::vector<float> s(3 * (size_t)n);
    EXPECT(slio_aloam_map_host_get_stack(h, kind, s.data(), n, &n) == SLIO_OK);
    if (n) EXPECT(slio_aloam_map_host_get_stack(h, kind, s.data(), n - 1, &n) == SLIO_ECAPACITY);
    for (int c = 0; c < 21 * 21 * 11; ++c) {
      EXPECT(slio_aloam_map_host_get_cube(h, kind, c, nullptr, 0, &n) == SLIO_OK);
      std::vector<float> q(3 * (size_t)n);
      EXPECT(slio_aloam_map_host_get_cube(h, kind, c, q.data(), n, &n) == SLIO_OK);
      total[kind] += n;
    }
  }
  EXPECT(total[0] >= 0 && total[1] >= 0);
  int32_t m = 0;
  EXPECT(slio_aloam_map_host_get_association(h, nullptr, nullptr, nullptr, nullptr, 1 << 20, &m) == SLIO_OK);
  EXPECT(m == r.stack_size[0] + r.stack_size[1]);
  std::vector<uint8_t> kind((size_t)m);
  std::vector<double> rec(6 * (size_t)m);
  std::vector<int32_t> idx(5 * (size_t)m);
  std::vector<float> sqd(5 * (size_t)m);
  EXPECT(slio_aloam_map_host_get_association(h, kind.data(), rec.data(), idx.data(), sqd.data(), m, &m) == SLIO_OK);
  if (m)
    EXPECT(slio_aloam_map_host_get_association(h, kind.data(), nullptr, nullptr, nullptr, m - 1, &m) == SLIO_ECAPACITY);
  for (int32_t s = 0; s < m; ++s) {
    EXPECT(kind[s] <= 4);
    const int32_t lim = r.map_size[s < r.stack_size[0] ? 0 : 1];
    for (int j = 0; j < 5; ++j) EXPECT(idx[5 * s + j] >= -1 && idx[5 * s + j] < lim);
  }
}

static void sweeps(float leaf_c, float leaf_s, const std::vector<std::vector<float>>& corner,
                   const std::vector<std::vector<float>>& surf, const std::vector<double>& tx, bool bad_point = false) {
  slio_aloam_map_params p;
  slio_aloam_map_host_handle h = nullptr;
  EXPECT(slio_aloam_map_params_default(&p) == SLIO_OK);
  p.leaf_corner = leaf_c;
  p.leaf_surf = leaf_s;
  p.max_scan = 2000;
  p.max_points = 20000;
  EXPECT(slio_aloam_map_host_create(&h, &p) == SLIO_OK && h);
  for (size_t k = 0; k < tx.size(); ++k) {
    std::vector<float> c = corner[k % corner.size()], s = surf[k % surf.size()];
    if (bad_point && pts(c) > 2) c[4] = NAN, c[9] = INFINITY;
    const double a = 0.002 * (double)k, q[4] = {0, 0, std::sin(a), std::cos(a)}, t[3] = {tx[k], 0.01 * (double)k, 0.0};
    slio_aloam_map_result r;
    EXPECT(slio_aloam_map_host_run(h, c.data(), pts(c), s.data(), pts(s), q, t, &r) == SLIO_OK);
    EXPECT(r.nvalid >= 1 && r.nvalid <= 75 && r.stack_size[0] <= pts(c) && r.stack_size[1] <= pts(s));
    EXPECT(r.optimized == (r.map_size[0] > 10 && r.map_size[1] > 50));
    for (int pass = 0; pass < 2 && r.optimized; ++pass) {
      EXPECT(r.pass[pass].iterations >= 0 && r.pass[pass].iterations <= 4 && r.pass[pass].stop >= 0 &&
             r.pass[pass].stop <= 3);
      EXPECT(r.pass[pass].cost_last <= r.pass[pass].cost_first);
      EXPECT(r.pass[pass].corner <= r.stack_size[0] && r.pass[pass].plane <= r.stack_size[1]);
    }
    for (int i = 0; i < 4; ++i) EXPECT(r.q_w_curr[i] == r.q_w_curr[i] && r.q_wmap_wodom[i] == r.q_wmap_wodom[i]);
    check_state(h, r);
  }
  EXPECT(slio_aloam_map_host_destroy(h) == SLIO_OK);
}

int main() {
  const std::vector<float> none;
  // the drifting fixture, then the jumps that run the shift loops
  sweeps(0.4f, 0.8f, {poles(90, 0), poles(90, 0.1), poles(90, 0.2)},
         {ground(700, 0), ground(700, 0.1), ground(700, 0.2)}, {0.0, 0.1, 0.2, -380.0, 380.0, 780.0});
  // a fine leaf: every point alone in its voxel, then PCL's pass-through
  sweeps(0.02f, 0.02f, {poles(257, 0)}, {ground(513, 0)}, {0.0, 0.02});
  sweeps(1e-6f, 1e-6f, {poles(30, 0)}, {ground(120, 0)}, {0.0, 0.02});
  // the sizes at which the loops start to run; an empty class
  for (int n : {0, 1, 4, 5, 6, 10, 11})
    sweeps(0.05f, 0.05f, {poles(n, 0)}, {ground(5 * n, 0)}, {0.0, 0.01, 0.02});
  sweeps(0.05f, 0.05f, {none}, {ground(300, 0)}, {0.0, 0.01});
  sweeps(0.05f, 0.05f, {poles(60, 0)}, {none}, {0.0, 0.01});
  sweeps(0.05f, 0.05f, {poles(60, 0), none}, {ground(300, 0), none}, {0.0, 0.01, 0.02});
  // non-finite points are dropped by the VoxelGrid
  sweeps(0.05f, 0.05f, {poles(60, 0)}, {ground(300, 0)}, {0.0, 0.01}, true);
  // the fits on coincident, collinear, planar and non-finite neighbours
  {
    double a[3], b[3], n[3], d, lam[3], vec[9], x[3];
    const double same[15] = {1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3};
    double line[15], plane[15], nan[15];
    for (int i = 0; i < 5; ++i) {
      line[3 * i] = 0.1 * i, line[3 * i + 1] = 1.0, line[3 * i + 2] = 0.0;
      plane[3 * i] = 0.3 * (i % 2), plane[3 * i + 1] = 0.3 * (i / 2), plane[3 * i + 2] = 2.0;
      nan[3 * i] = NAN, nan[3 * i + 1] = 0, nan[3 * i + 2] = INFINITY;
    }
    EXPECT(slio_aloam_map_host_fit_line(same, a, b, lam, vec) == 3);
    EXPECT(slio_aloam_map_host_fit_line(line, a, b, lam, vec) == 1 && std::fabs(std::fabs(a[0] - b[0]) - 0.2) < 1e-12);
    EXPECT(slio_aloam_map_host_fit_line(plane, a, b, nullptr, nullptr) == 4);
    EXPECT(slio_aloam_map_host_fit_line(nan, a, b, lam, vec) == 3);
    EXPECT(slio_aloam_map_host_fit_plane(plane, n, &d, x) == 2 && std::fabs(std::fabs(n[2]) - 1.0) < 1e-12);
    EXPECT(slio_aloam_map_host_fit_plane(line, n, &d, x) == 3);
    EXPECT(slio_aloam_map_host_fit_plane(same, n, &d, nullptr) == 3);
    EXPECT(slio_aloam_map_host_fit_plane(nan, n, &d, x) == 3);
    EXPECT(slio_aloam_map_host_fit_line(nullptr, a, b, lam, vec) == SLIO_EINVAL);
    EXPECT(slio_aloam_map_host_fit_plane(plane, nullptr, &d, x) == SLIO_EINVAL);
  }
  // the evaluation at the group sizes of the sums
  for (int n : {0, 1, 31, 32, 33, 255, 256, 257, 256 * 32, 256 * 33 + 1}) {
    std::vector<float> xyz(3 * (size_t)n);
    std::vector<uint8_t> kind((size_t)n);
    std::vector<double> rec(6 * (size_t)n, 0.0);
    for (int i = 0; i < n; ++i) {
      xyz[3 * i] = 0.01f * (float)(i % 100), xyz[3 * i + 1] = 1.f, xyz[3 * i + 2] = 0.5f;
      kind[i] = (uint8_t)(i % 5);
      double* r = &rec[6 * (size_t)i];
      if (kind[i] == 1) r[0] = 0.1, r[3] = -0.1, r[1] = r[4] = 1.0;
      if (kind[i] == 2) r[2] = 1.0, r[3] = -0.45;
    }
    const double q[4] = {0, 0, 0.01, 0.99995}, t[3] = {0.1, 0, 0};
    double A[21], g[6], cost;
    int32_t cnt[4];
    EXPECT(slio_aloam_map_host_evaluate(xyz.data(), kind.data(), rec.data(), n, q, t, A, g, &cost, cnt) == SLIO_OK);
    EXPECT(cnt[0] == (n + 3) / 5 && cnt[1] == (n + 2) / 5 && cnt[2] == (n + 1) / 5 && cost >= 0 && cost == cost);
  }
  // argument errors
  {
    slio_aloam_map_params p;
    slio_aloam_map_host_handle h = nullptr;
    slio_aloam_map_result r;
    const double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0}, z[4] = {0, 0, 0, 0};
    double o[7];
    int32_t cen[3] = {10, 10, 5}, ctr[3], sh[3], list[75], n;
    EXPECT(slio_aloam_map_params_default(nullptr) == SLIO_EINVAL && slio_aloam_map_params_default(&p) == SLIO_OK);
    EXPECT(slio_aloam_map_host_create(nullptr, &p) == SLIO_EINVAL);
    EXPECT(slio_aloam_map_host_create(&h, nullptr) == SLIO_EINVAL);
    p.max_scan = 2;
    p.max_points = 3;
    EXPECT(slio_aloam_map_host_create(&h, &p) == SLIO_OK);
    const std::vector<float> c = poles(3, 0);
    EXPECT(slio_aloam_map_host_run(h, c.data(), 3, nullptr, 0, q, t, &r) == SLIO_ECAPACITY);
    EXPECT(slio_aloam_map_host_run(h, c.data(), 2, nullptr, 1, q, t, &r) == SLIO_EINVAL);
    EXPECT(slio_aloam_map_host_run(h, c.data(), 2, nullptr, 0, z, t, &r) == SLIO_EINVAL);
    EXPECT(slio_aloam_map_host_run(h, c.data(), 2, nullptr, 0, q, t, nullptr) == SLIO_EINVAL);
    EXPECT(slio_aloam_map_host_get_stack(h, 0, nullptr, 0, nullptr) == SLIO_ESTATE);
    EXPECT(slio_aloam_map_host_run(h, c.data(), 2, nullptr, 0, q, t, &r) == SLIO_OK && r.stack_size[0] == 2);
    EXPECT(slio_aloam_map_host_run(h, c.data(), 2, nullptr, 0, q, t, &r) == SLIO_ECAPACITY);
    EXPECT(slio_aloam_map_host_get_cube(h, 2, 0, nullptr, 0, nullptr) == SLIO_EINVAL);
    EXPECT(slio_aloam_map_host_get_cube(h, 0, 4851, nullptr, 0, nullptr) == SLIO_EINVAL);
    EXPECT(slio_aloam_map_host_destroy(h) == SLIO_OK && slio_aloam_map_host_destroy(nullptr) == SLIO_OK);
    EXPECT(slio_aloam_map_predict(q, t, q, t, o, o + 4) == SLIO_OK && o[3] == 1.0);
    EXPECT(slio_aloam_map_predict(nullptr, t, q, t, o, o + 4) == SLIO_EINVAL);
    const double far[3] = {-380.0, 380.0, 130.0}, bad[3] = {1e7, 0, 0};
    EXPECT(slio_aloam_map_host_select(far, cen, ctr, sh, list, &n) == SLIO_OK);
    EXPECT(sh[0] == 1 && sh[1] == -1 && sh[2] == -1);
    EXPECT(n == 75 && cen[0] == 11 && cen[1] == 9 && cen[2] == 4);
    EXPECT(slio_aloam_map_host_select(bad, cen, ctr, sh, list, &n) == SLIO_EINVAL && cen[0] == 11);
    EXPECT(slio_aloam_map_host_select(far, nullptr, ctr, sh, list, &n) == SLIO_EINVAL);
  }

  std::printf(fails ? "FAILED %d\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
