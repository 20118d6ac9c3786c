// Stand-alone driver of the loop closure's host code -- slio_lmap_detect_loop
// and slio_lmap_loop_correction (csrc/slio_lmap.cpp) and the ICP step shared
// with the device loop (csrc/slio_icp.hpp through slio_icp_step,
// csrc/slio_s2m.cpp) -- for tests/test_lego_loop_cpu.py, which builds it with
// -fsanitize=address,undefined and runs it as a child process.  Exits 0 when
// every call returned what it should; the sanitizers abort it otherwise.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "slio.h"

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

int main() {
  // detection: ten keys on a circle, 5 s apart; the current position beside key 9
  std::vector<float> xyz;
  std::vector<double> tm;
  for (int k = 0; k < 10; ++k) {
    const double a = 2.0 * M_PI * k / 10.0;
    xyz.push_back((float)(3.0 * std::cos(a)));
    xyz.push_back(0.1f * k);
    xyz.push_back((float)(3.0 * std::sin(a)));
    tm.push_back(5.0 * k);
  }
  const float cur[3] = {xyz[27], xyz[28], xyz[29]};
  int32_t id = -2;
  EXPECT(slio_lmap_detect_loop(xyz.data(), tm.data(), 10, cur, 45.0, 5.0f, 30.0, &id) == SLIO_OK);
  EXPECT(id == 0);
  EXPECT(slio_lmap_detect_loop(xyz.data(), tm.data(), 10, cur, 45.0, 1.0f, 30.0, &id) == SLIO_OK);
  EXPECT(id == -1);  // nothing but key 9 itself within 1 m
  EXPECT(slio_lmap_detect_loop(xyz.data(), tm.data(), 10, cur, 20.0, 5.0f, 30.0, &id) == SLIO_OK);
  EXPECT(id == -1);  // nothing 30 s away
  EXPECT(slio_lmap_detect_loop(nullptr, nullptr, 0, cur, 45.0, 5.0f, 30.0, &id) == SLIO_OK);
  EXPECT(id == -1);
  EXPECT(slio_lmap_detect_loop(xyz.data(), tm.data(), 10, cur, 45.0, 5.0f, 30.0, nullptr) == SLIO_EINVAL);
  EXPECT(slio_lmap_detect_loop(nullptr, tm.data(), 10, cur, 45.0, 5.0f, 30.0, &id) == SLIO_EINVAL);
  EXPECT(slio_lmap_detect_loop(xyz.data(), tm.data(), -1, cur, 45.0, 5.0f, 30.0, &id) == SLIO_EINVAL);
  EXPECT(slio_lmap_detect_loop(xyz.data(), tm.data(), 10, cur, 45.0, NAN, 30.0, &id) == SLIO_EINVAL);

  // correction: the identity leaves the latest key where it is
  float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float latest[6] = {0.01f, 0.7f, -0.02f, 1.5f, -0.2f, 2.5f}, closest[6] = {0, 0.1f, 0, 3.f, 0, 0.5f};
  float from[6], to[6], noise = -1;
  EXPECT(slio_lmap_loop_correction(T, latest, closest, 0.125, from, to, &noise) == SLIO_OK);
  EXPECT(noise == 0.125f);
  EXPECT(from[0] == latest[5] && from[1] == latest[3] && from[2] == latest[4]);
  EXPECT(std::fabs(from[3] - latest[2]) < 1e-6f && std::fabs(from[4] - latest[0]) < 1e-6f &&
         std::fabs(from[5] - latest[1]) < 1e-6f);
  EXPECT(to[0] == closest[5] && to[1] == closest[3] && to[2] == closest[4] && to[3] == closest[2] &&
         to[4] == closest[0] && to[5] == closest[1]);
  T[3] = 0.3f, T[7] = -0.1f, T[11] = 0.2f;
  T[0] = T[10] = std::cos(0.03f), T[2] = std::sin(0.03f), T[8] = -T[2];
  EXPECT(slio_lmap_loop_correction(T, latest, closest, DBL_MAX, from, to, &noise) == SLIO_OK);
  for (float v : from) EXPECT(std::isfinite(v));
  EXPECT(std::isinf(noise));  // DBL_MAX rounds to +inf in float, as the reference's assignment does
  EXPECT(slio_lmap_loop_correction(nullptr, latest, closest, 0.1, from, to, &noise) == SLIO_EINVAL);
  EXPECT(slio_lmap_loop_correction(T, latest, closest, 0.1, from, to, nullptr) == SLIO_EINVAL);

  // the shared ICP step: a pure translation, a planar (rank-2) cloud, a
  // rank-1 one, too few correspondences, the iteration limit
  slio_icp_params prm;
  slio_icp_state st;
  EXPECT(slio_icp_params_default(&prm) == SLIO_OK);
  EXPECT(slio_icp_params_default(nullptr) == SLIO_EINVAL);
  for (int shape = 0; shape < 3; ++shape) {
    double sums[16] = {0};
    const int n = 40;
    for (int i = 0; i < n; ++i) {
      const double p[3] = {0.3 * i, shape == 2 ? 0.0 : std::sin(0.7 * i), shape == 0 ? std::cos(1.3 * i) : 0.0};
      const double q[3] = {p[0] + 0.25, p[1] - 0.5, p[2] + 0.125};
      for (int a = 0; a < 3; ++a) {
        sums[a] += p[a];
        sums[3 + a] += q[a];
        for (int b = 0; b < 3; ++b) sums[6 + 3 * a + b] += q[a] * p[b];
      }
      sums[15] += 0.25 * 0.25 + 0.5 * 0.5 + 0.125 * 0.125;
    }
    EXPECT(slio_icp_state_init(&st, nullptr) == SLIO_OK);
    float delta[16];
    int done = -1;
    EXPECT(slio_icp_step(sums, n, &prm, &st, delta, &done) == SLIO_OK);
    EXPECT(done == 0 && st.iterations == 1 && st.convergence_state == SLIO_ICP_NOT_CONVERGED);
    EXPECT(std::fabs(delta[3] - 0.25f) < 1e-5f && std::fabs(delta[7] + 0.5f) < 1e-5f &&
           std::fabs(delta[11] - 0.125f) < 1e-5f);
    // (a line leaves the rotation about itself open: only the others are checked)
    for (int r = 0; r < 3 && shape < 2; ++r)
      for (int c = 0; c < 3; ++c) EXPECT(std::fabs(delta[4 * r + c] - (r == c ? 1.0f : 0.0f)) < 1e-5f);
    for (int i = 0; i < 16; ++i) EXPECT(std::isfinite(delta[i]));
    // the same sums again: the mean squared error did not move
    EXPECT(slio_icp_step(sums, n, &prm, &st, delta, &done) == SLIO_OK);
    EXPECT(done == 1 && st.converged == 1 && st.convergence_state == SLIO_ICP_ABS_MSE);
    EXPECT(slio_icp_state_init(&st, nullptr) == SLIO_OK);
    EXPECT(slio_icp_step(sums, 2, &prm, &st, delta, &done) == SLIO_OK);
    EXPECT(done == 1 && st.converged == 0 && st.convergence_state == SLIO_ICP_NO_CORRESPONDENCES);
    prm.max_iterations = 1;
    EXPECT(slio_icp_state_init(&st, nullptr) == SLIO_OK);
    EXPECT(slio_icp_step(sums, n, &prm, &st, delta, &done) == SLIO_OK);
    EXPECT(done == 1 && st.convergence_state == SLIO_ICP_ITERATIONS);
    prm.max_iterations = 100;
    EXPECT(slio_icp_step(nullptr, n, &prm, &st, delta, &done) == SLIO_EINVAL);
    EXPECT(slio_icp_step(sums, -1, &prm, &st, delta, &done) == SLIO_EINVAL);
  }
  {
    double zero[16] = {0};
    float delta[16];
    int done = -1;
    EXPECT(slio_icp_state_init(&st, nullptr) == SLIO_OK);
    EXPECT(slio_icp_step(zero, 10, &prm, &st, delta, &done) == SLIO_OK);  // A == 0: identity
    for (int i = 0; i < 16; ++i) EXPECT(delta[i] == (i % 5 == 0 ? 1.0f : 0.0f));
  }

  std::printf(fails ? "FAILED %d\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
