// Stand-alone driver of the livox_mapping host code (csrc/slio_livox.cpp and
// the step in csrc/slio_s2m.cpp) for tests/test_livox_map_cpu.py, which builds
// it with -fsanitize=address,undefined and runs it as a child process: the
// same cases the Python tests put through the library.  Exits 0 when every
// call returned what it should; the sanitizers abort it otherwise.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

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
  // cube index: negatives, exact multiples of 50 - 25, and their neighbours
  for (int k = -12; k <= 12; ++k) {
    const float e = 50.0f * k - 25.0f;
    const float ts[3] = {std::nextafterf(e, -INFINITY), e, std::nextafterf(e, INFINITY)};
    for (float t : ts) {
      int32_t c = 0;
      EXPECT(slio_lvx_cube_index(t, 10, &c) == SLIO_OK);
      // truncation then `--` is the floor, except on an exact negative
      // multiple of 50, where the reference lands one cube lower
      const double v = (double)t + 25.0, fl = std::floor(v / 50.0);
      EXPECT(c == (int)fl + 10 - (v < 0 && v == 50.0 * fl ? 1 : 0));
    }
  }
  int32_t c = 0;
  EXPECT(slio_lvx_cube_index(NAN, 10, &c) == SLIO_EINVAL);
  EXPECT(slio_lvx_cube_index(3e9f, 10, &c) == SLIO_EINVAL);
  EXPECT(slio_lvx_cube_index(0.0f, 10, nullptr) == SLIO_EINVAL);

  // selection: identity, rotated, and poses that shift in each direction, twice
  const float poses[9][6] = {{0, 0, 0, 0, 0, 0},          {0.3f, -0.2f, 1.1f, 12.f, -30.f, 24.9f},
                             {-0.7f, 0.4f, -2.f, -80.f, 49.f, 130.f}, {0, 0, 0, 400.f, 0, 0},
                             {0, 0, 0, -400.f, 0, 0},     {0, 0, 0, 0, 160.f, 0},
                             {0, 0, 0, 0, -160.f, 0},     {0, 0, 0, 0, 0, 460.f},
                             {0, 0, 0, -460.f, 0, -400.f}};
  int32_t cen[3] = {10, 5, 10};
  for (const auto& tf : poses) {
    int32_t ctr[3], shift[3], v[125], s[125], nv = -1, ns = -1;
    EXPECT(slio_lvx_select_host(tf, cen, ctr, shift, v, &nv, s, &ns) == SLIO_OK);
    EXPECT(nv >= 0 && nv <= ns && ns <= 125);
    for (int a = 0; a < 3; ++a) EXPECT(ctr[a] >= 3 && ctr[a] < (a == 1 ? 11 : 21) - 3);
    for (int i = 0; i < ns; ++i) EXPECT(s[i] >= 0 && s[i] < SLIO_LVX_CUBES);
  }
  {
    int32_t ctr[3], shift[3], v[125], s[125], nv, ns;
    const float bad[6] = {0, 0, 0, INFINITY, 0, 0};
    EXPECT(slio_lvx_select_host(bad, cen, ctr, shift, v, &nv, s, &ns) == SLIO_EINVAL);
    EXPECT(slio_lvx_select_host(poses[0], nullptr, ctr, shift, v, &nv, s, &ns) == SLIO_EINVAL);
  }

  // the plane system: a tilted plane with a little noise, then a singular set
  float nb[24];
  for (int i = 0; i < 8; ++i) {
    const float x = 3.0f + 0.37f * i, y = -2.0f + 0.11f * i * i;
    nb[3 * i] = x;
    nb[3 * i + 1] = y;
    nb[3 * i + 2] = 1.5f + 0.2f * x - 0.1f * y + 0.001f * (i % 3);
  }
  float x10[3], x8[3];
  EXPECT(slio_lvx_plane_solve(nb, 10, x10) == SLIO_OK);
  EXPECT(slio_lvx_plane_solve(nb, 8, x8) == SLIO_OK);
  EXPECT(std::memcmp(x10, x8, sizeof x8) == 0);
  std::memset(nb, 0, sizeof nb);
  EXPECT(slio_lvx_plane_solve(nb, 10, x10) == 1);
  EXPECT(x10[0] == 0.0f && x10[1] == 0.0f && x10[2] == 0.0f);
  EXPECT(slio_lvx_plane_solve(nb, 9, x10) == SLIO_EINVAL);
  EXPECT(slio_lvx_plane_solve(nullptr, 10, x10) == SLIO_EINVAL);

  // the step: a well-conditioned system, one weak direction, too few rows
  float AtA[36] = {0}, AtB[6], tf[6] = {0}, P[36] = {0};
  for (int i = 0; i < 6; ++i) {
    AtA[6 * i + i] = 200.0f + 10.0f * i;
    AtB[i] = 0.01f * (i + 1);
  }
  AtA[1] = AtA[6] = 3.0f;
  int deg = -1, conv = -1;
  EXPECT(slio_lvx_lm_step(AtA, AtB, 400, 0, tf, &deg, P, &conv) == SLIO_OK);
  EXPECT(deg == 0);
  AtA[35] = 0.5f;  // one eigenvalue below eignThre = 1
  EXPECT(slio_lvx_lm_step(AtA, AtB, 400, 0, tf, &deg, P, &conv) == SLIO_OK);
  EXPECT(deg == 1);
  EXPECT(slio_lvx_lm_step(AtA, AtB, 400, 1, tf, &deg, P, &conv) == SLIO_OK);
  EXPECT(slio_lvx_lm_step(AtA, AtB, 49, 1, tf, &deg, P, &conv) == 1);
  EXPECT(conv == 0);
  EXPECT(slio_lvx_lm_step(nullptr, AtB, 400, 0, tf, &deg, P, &conv) == SLIO_EINVAL);
  EXPECT(slio_s2m_lm_step(AtA, AtB, 400, 0, tf, &deg, P, &conv) == SLIO_OK);
  EXPECT(deg == 1);  // 0.5 is below 100 as well
  for (int i = 0; i < 6; ++i) EXPECT(std::isfinite(tf[i]));

  std::printf(fails ? "FAILED %d\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
