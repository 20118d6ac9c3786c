// Stand-alone driver of the A-LOAM laserOdometry host code
// (csrc/slio_aloam_odom.cpp with the formulas of csrc/slio_aloam_odom.hpp) for
// tests/test_aloam_odom_cpu.py, which builds it with
// -fsanitize=address,undefined and runs it as a child process.  The clouds are
// rings of a wavy wall seen from two poses, cut to the sizes at which the
// loops start to run (last clouds of 0, 1 and 2 points, one ring, the top
// ring), with coincident and collinear points; every buffer is allocated at
// exactly the size the entry promises to stay within, so a write past it is
// the sanitizer's to find.  Exits 0 when every call returned what it should.
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

// rings ring0 .. ring0 + rings - 1 of `per` points each on a wavy wall, seen from a sensor moved by (dx, yaw)
static std::vector<float> wall(int rings, int per, int ring0, double dx, double yaw, double phase = 0.0) {
  std::vector<float> c;
  for (int r = 0; r < rings; ++r)
    for (int i = 0; i < per; ++i) {
      const double az = -1.2 + 2.4 * (i + phase) / per, el = (-15.0 + 2.0 * r) * M_PI / 180;
      const double rg = 8 * (1 + 0.2 * std::sin(5 * az) + 0.1 * (std::sin(23 * az) > 0.5));
      const double x = rg * std::cos(el) * std::cos(az) - dx, y = rg * std::cos(el) * std::sin(az), z = rg * std::sin(el);
      c.push_back((float)(std::cos(yaw) * x + std::sin(yaw) * y));
      c.push_back((float)(-std::sin(yaw) * x + std::cos(yaw) * y));
      c.push_back((float)z);
      c.push_back((float)(ring0 + r) + 0.1f * i / per);
    }
  return c;
}

static int64_t pts(const std::vector<float>& c) { return (int64_t)(c.size() / 4); }

static void pass(const std::vector<float>& sharp, const std::vector<float>& flat, const std::vector<float>& cl,
                 const std::vector<float>& sl, int want_rc = SLIO_OK) {
  const double q[4] = {0, 0, 0.01, 0.99995}, t[3] = {0.1, 0.0, 0.0};
  const size_t slots = (size_t)(pts(sharp) + pts(flat));
  std::vector<int32_t> corr(3 * slots);
  const int rc = slio_aloam_odom_host_associate(sharp.data(), pts(sharp), flat.data(), pts(flat), cl.data(), pts(cl),
                                                sl.data(), pts(sl), q, t, corr.data());
  EXPECT(rc == want_rc);
  if (rc != SLIO_OK) return;
  for (size_t s = 0; s < slots; ++s) {
    const int64_t n = s < (size_t)pts(sharp) ? pts(cl) : pts(sl);
    for (int k = 0; k < 3; ++k) EXPECT(corr[3 * s + k] >= -1 && corr[3 * s + k] < n);
    if (corr[3 * s] < 0) EXPECT(corr[3 * s + 1] < 0 && corr[3 * s + 2] < 0);
  }
  double A[21], g[6], cost;
  int32_t cnt[4];
  EXPECT(slio_aloam_odom_host_evaluate(sharp.data(), pts(sharp), flat.data(), pts(flat), cl.data(), pts(cl), sl.data(),
                                       pts(sl), corr.data(), q, t, A, g, &cost, cnt) == SLIO_OK);
  EXPECT(cnt[0] <= pts(sharp) && cnt[1] <= pts(flat) && cnt[2] <= cnt[0] + cnt[1] && cnt[3] <= cnt[0] + cnt[1]);
  EXPECT(cost >= 0 && cost == cost);
  slio_aloam_odom_params p;
  slio_aloam_odom_state st;
  slio_aloam_odom_result res;
  EXPECT(slio_aloam_odom_params_default(&p) == SLIO_OK && slio_aloam_odom_host_init(&st) == SLIO_OK);
  p.n_scans = 64;
  p.max_points = (int32_t)(pts(cl) > pts(sl) ? pts(cl) : pts(sl)) + 1;
  for (int k = 0; k < 3; ++k) {
    EXPECT(slio_aloam_odom_host_run(&p, &st, sharp.data(), pts(sharp), flat.data(), pts(flat), cl.data(), pts(cl),
                                    sl.data(), pts(sl), &res) == SLIO_OK);
    EXPECT(res.inited == (k > 0) && res.published == (k % 2 == 0) && res.frame_count == 1 + k % 2);
    for (int a = 0; a < 2 && k; ++a) {
      EXPECT(res.pass[a].iterations >= 0 && res.pass[a].iterations <= 4 && res.pass[a].stop >= 0 &&
             res.pass[a].stop <= 3);
      EXPECT(res.pass[a].cost_last <= res.pass[a].cost_first);
    }
    for (int a = 0; a < 4; ++a) EXPECT(res.q_w_curr[a] == res.q_w_curr[a]);
  }
}

int main() {
  const std::vector<float> none;
  const std::vector<float> cl = wall(16, 12, 0, 0, 0), sl = wall(16, 40, 0, 0, 0, 0.4);
  const std::vector<float> sharp = wall(16, 2, 0, 0.1, 0.01, 0.2), flat = wall(16, 4, 0, 0.1, 0.01, 0.3);
  pass(sharp, flat, cl, sl);
  pass(none, none, cl, sl);
  pass(sharp, none, cl, sl);
  pass(none, flat, cl, sl);
  pass(sharp, flat, none, none);
  for (int n : {1, 2, 3, 12, 13}) {
    std::vector<float> c(cl.begin(), cl.begin() + 4 * n), s(sl.begin(), sl.begin() + 4 * n);
    pass(sharp, flat, c, s);
  }
  pass(sharp, flat, wall(1, 50, 0, 0, 0), wall(1, 50, 63, 0, 0));      // one ring; the top ring
  pass(sharp, flat, wall(3, 20, 61, 0, 0), wall(2, 30, 62, 0, 0));     // the rings up to the top one
  {
    std::vector<float> c = cl, s = sl;  // coincident and collinear points
    for (int i = 0; i < 24; ++i) std::memcpy(&c[4 * i], &c[0], 12);
    for (int i = 0; i < 120; ++i) s[4 * i + 1] = 0.f, s[4 * i + 2] = 0.f;
    pass(sharp, flat, c, s);
  }
  {
    std::vector<float> c = cl;  // ids that decrease, an id of 64, a NaN id
    c[4 * 30 + 3] = 0.f;
    pass(sharp, flat, c, sl, SLIO_EINVAL);
    c = cl;
    c[4 * (pts(cl) - 1) + 3] = 64.f;
    pass(sharp, flat, c, sl, SLIO_EINVAL);
    c = sl;
    c[3] = NAN;
    pass(sharp, flat, cl, c, SLIO_EINVAL);
  }
  // the controller: a rejected step (a cost that rises), a non-positive pivot, the stops
  {
    slio_aloam_odom_lm lm;
    std::memset(&lm, 0, sizeof lm);
    lm.q[3] = 1;
    EXPECT(slio_aloam_odom_lm_step(&lm, 0, nullptr, nullptr, 0) == SLIO_OK && lm.mu == 1e4 && lm.nu == 2);
    for (int k = 0; k < 6; ++k) lm.A[k * 6 - k * (k - 1) / 2] = 1 + k, lm.g[k] = 0.1 * (k + 1);
    lm.cost = 1;
    for (int k = 0; k < 4; ++k) {
      EXPECT(slio_aloam_odom_lm_step(&lm, 1, nullptr, nullptr, 0) == SLIO_OK && !lm.done && lm.pivots_ok);
      EXPECT(slio_aloam_odom_lm_step(&lm, 2, lm.A, lm.g, 2.0) == SLIO_OK && !lm.last_accepted);
    }
    EXPECT(lm.done && lm.stop == 0 && lm.iterations == 4 && lm.mu == 1e4 / 1024);
    EXPECT(slio_aloam_odom_lm_step(&lm, 2, lm.A, lm.g, 2.0) == SLIO_ESTATE);
    EXPECT(slio_aloam_odom_lm_step(&lm, 0, nullptr, nullptr, 0) == SLIO_OK);
    lm.A[0] = -1e9;
    EXPECT(slio_aloam_odom_lm_step(&lm, 1, nullptr, nullptr, 0) == SLIO_OK && !lm.pivots_ok);
    EXPECT(slio_aloam_odom_lm_step(&lm, 2, lm.A, lm.g, 0.5) == SLIO_OK && lm.done && lm.stop == 3);
    EXPECT(slio_aloam_odom_lm_step(&lm, 0, nullptr, nullptr, 0) == SLIO_OK);
    for (int k = 0; k < 6; ++k) lm.g[k] = 0;
    EXPECT(slio_aloam_odom_lm_step(&lm, 1, nullptr, nullptr, 0) == SLIO_OK && lm.done && lm.stop == 1);
    EXPECT(slio_aloam_odom_lm_step(nullptr, 0, nullptr, nullptr, 0) == SLIO_EINVAL);
    EXPECT(slio_aloam_odom_lm_step(&lm, 3, nullptr, nullptr, 0) == SLIO_EINVAL);
    EXPECT(slio_aloam_odom_lm_step(&lm, 2, nullptr, nullptr, 0) == SLIO_EINVAL);
  }
  // argument errors
  {
    slio_aloam_odom_params p;
    slio_aloam_odom_state st;
    slio_aloam_odom_result res;
    const double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
    int32_t corr[3] = {0, 0, 0}, cnt[4];
    double A[21], g[6], cost;
    EXPECT(slio_aloam_odom_params_default(nullptr) == SLIO_EINVAL && slio_aloam_odom_host_init(nullptr) == SLIO_EINVAL);
    EXPECT(slio_aloam_odom_params_default(&p) == SLIO_OK && p.n_scans == 16 && p.skip_frame_num == 2);
    slio_aloam_odom_host_init(&st);
    EXPECT(slio_aloam_odom_host_associate(nullptr, 1, nullptr, 0, nullptr, 0, nullptr, 0, q, t, corr) == SLIO_EINVAL);
    EXPECT(slio_aloam_odom_host_associate(sharp.data(), -1, nullptr, 0, nullptr, 0, nullptr, 0, q, t, corr) ==
           SLIO_EINVAL);
    EXPECT(slio_aloam_odom_host_associate(sharp.data(), 1, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, t, corr) ==
           SLIO_EINVAL);
    EXPECT(slio_aloam_odom_host_associate(sharp.data(), 769, nullptr, 0, nullptr, 0, nullptr, 0, q, t, corr) ==
           SLIO_ECAPACITY);
    corr[0] = 5;
    EXPECT(slio_aloam_odom_host_evaluate(sharp.data(), 1, nullptr, 0, cl.data(), 5, nullptr, 0, corr, q, t, A, g, &cost,
                                         cnt) == SLIO_EINVAL);
    corr[0] = -1;
    corr[1] = 2;
    EXPECT(slio_aloam_odom_host_evaluate(sharp.data(), 1, nullptr, 0, cl.data(), 5, nullptr, 0, corr, q, t, A, g, &cost,
                                         cnt) == SLIO_EINVAL);
    EXPECT(slio_aloam_odom_host_run(nullptr, &st, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, &res) == SLIO_EINVAL);
    p.skip_frame_num = 0;
    EXPECT(slio_aloam_odom_host_run(&p, &st, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, &res) == SLIO_EINVAL);
    p.skip_frame_num = 1;
    p.n_scans = 1;
    EXPECT(slio_aloam_odom_host_run(&p, &st, sharp.data(), 13, nullptr, 0, nullptr, 0, nullptr, 0, &res) ==
           SLIO_ECAPACITY);
    EXPECT(slio_aloam_odom_host_run(&p, &st, sharp.data(), 12, nullptr, 0, nullptr, 0, nullptr, 0, &res) == SLIO_OK);
  }

  std::printf(fails ? "FAILED %d\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
