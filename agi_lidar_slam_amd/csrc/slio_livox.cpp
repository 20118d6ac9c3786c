// slio_livox.cpp -- the host formulas of livox_mapping's laserMapping node
// (src/livox_mapping/src/laserMapping.cpp), callable without a GPU: the cube
// index of a coordinate (:482-491, :1162-1168), the centre cube with the six
// shift loops' bookkeeping (:493-713), the field-of-view test that picks the
// valid and the surround cubes (:715-776), and the plane system of the surf
// branch (:962-975).  Float and double exactly where the reference has them;
// sin / cos / sqrt of a float are the double functions.  The step after the
// normal equations (:1102-1150) is slio_lvx_lm_step, beside its two siblings
// in slio_s2m.cpp.
#include <cmath>
#include <cstring>

#include "slio.h"
#include "slio_common.hpp"
#include "slio_cvsolve.hpp"
#include "slio_livox.hpp"

using slio::set_error;

namespace slio {
namespace lvx {

int select_host(const float tf[6], int32_t cen[3], int32_t center[3], int32_t shift[3], int32_t* valid,
                int32_t* nvalid, int32_t* surround, int32_t* nsurround) {
  // :475-480: pointOnYAxis = pointAssociateToMap((0, 10, 0))
  float py[3];
  {
    const float cr = fcos(tf[0]), sr = fsin(tf[0]), cp = fcos(tf[1]), sp = fsin(tf[1]), cy = fcos(tf[2]),
                sy = fsin(tf[2]);
    const float x = 0.0f, y = 10.0f, z = 0.0f;
    const float x1 = cy * x - sy * y;
    const float y1 = sy * x + cy * y;
    const float z1 = z;
    const float x2 = x1;
    const float y2 = cr * y1 - sr * z1;
    const float z2 = sr * y1 + cr * z1;
    py[0] = cp * x2 + sp * z2 + tf[3];
    py[1] = y2 + tf[4];
    py[2] = -sp * x2 + cp * z2 + tf[5];
  }
  const int dim[3] = {kW, kH, kD};
  int c[3];
  for (int a = 0; a < 3; ++a) {
    if (!cube_of(tf[3 + a], cen[a], &c[a])) return 1;
    shift[a] = 0;
    // :493-713: one cube per turn while the centre is within 3 of an edge;
    // the contents move with the centre
    while (c[a] < 3) {
      ++c[a];
      ++cen[a];
      ++shift[a];
    }
    while (c[a] >= dim[a] - 3) {
      --c[a];
      --cen[a];
      --shift[a];
    }
    center[a] = c[a];
  }
  int nv = 0, ns = 0;
  for (int i = c[0] - 2; i <= c[0] + 2; ++i)
    for (int j = c[1] - 2; j <= c[1] + 2; ++j)
      for (int k = c[2] - 2; k <= c[2] + 2; ++k) {
        if (!(i >= 0 && i < kW && j >= 0 && j < kH && k >= 0 && k < kD)) continue;
        const float centerX = (float)(50.0 * (i - cen[0]));
        const float centerY = (float)(50.0 * (j - cen[1]));
        const float centerZ = (float)(50.0 * (k - cen[2]));
        bool in_fov = false;
        for (int ii = -1; ii <= 1; ii += 2)
          for (int jj = -1; jj <= 1; jj += 2)
            for (int kk = -1; kk <= 1; kk += 2) {
              const float cornerX = (float)(centerX + 25.0 * ii);
              const float cornerY = (float)(centerY + 25.0 * jj);
              const float cornerZ = (float)(centerZ + 25.0 * kk);
              const float squaredSide1 = (tf[3] - cornerX) * (tf[3] - cornerX) +
                                         (tf[4] - cornerY) * (tf[4] - cornerY) +
                                         (tf[5] - cornerZ) * (tf[5] - cornerZ);
              const float squaredSide2 = (py[0] - cornerX) * (py[0] - cornerX) +
                                         (py[1] - cornerY) * (py[1] - cornerY) +
                                         (py[2] - cornerZ) * (py[2] - cornerZ);
              const float check1 =
                  (float)(100.0 + squaredSide1 - squaredSide2 - 10.0 * std::sqrt(3.0) * std::sqrt((double)squaredSide1));
              const float check2 =
                  (float)(100.0 + squaredSide1 - squaredSide2 + 10.0 * std::sqrt(3.0) * std::sqrt((double)squaredSide1));
              if (check1 < 0 && check2 > 0) in_fov = true;
            }
        const int ind = i + kW * j + kW * kH * k;
        if (in_fov) valid[nv++] = ind;
        surround[ns++] = ind;
      }
  *nvalid = nv;
  *nsurround = ns;
  return 0;
}

}  // namespace lvx
}  // namespace slio

extern "C" {

int slio_lvx_cube_index(float t, int32_t cen, int32_t* cube) {
  if (!cube) {
    set_error("slio_lvx_cube_index: null argument");
    return SLIO_EINVAL;
  }
  int c;
  if (!slio::lvx::cube_of(t, cen, &c)) {
    set_error("slio_lvx_cube_index: coordinate is not finite or beyond 1e6 m");
    return SLIO_EINVAL;
  }
  *cube = c;
  return SLIO_OK;
}

int slio_lvx_select_host(const float transform[6], int32_t cen[3], int32_t center[3], int32_t shift[3],
                         int32_t* valid, int32_t* nvalid, int32_t* surround, int32_t* nsurround) {
  if (!transform || !cen || !center || !shift || !valid || !nvalid || !surround || !nsurround) {
    set_error("slio_lvx_select_host: null argument");
    return SLIO_EINVAL;
  }
  for (int a = 0; a < 6; ++a)
    if (!std::isfinite(transform[a])) {
      set_error("slio_lvx_select_host: transform is not finite");
      return SLIO_EINVAL;
    }
  int32_t c2[3] = {cen[0], cen[1], cen[2]};
  if (slio::lvx::select_host(transform, c2, center, shift, valid, nvalid, surround, nsurround)) {
    set_error("slio_lvx_select_host: position beyond 1e6 m");
    return SLIO_EINVAL;
  }
  std::memcpy(cen, c2, sizeof c2);
  return SLIO_OK;
}

int slio_lvx_plane_solve(const float* nb_xyz, int m, float x[3]) {
  if (!nb_xyz || !x || (m != 8 && m != 10)) {
    set_error("slio_lvx_plane_solve: need 8 neighbours and m of 8 or 10");
    return SLIO_EINVAL;
  }
  // matA0 is 10 x 3 with rows 8 and 9 never written, matB0 ten times -1
  // (:423-425); m = 8 leaves the two zero rows out
  float A[30] = {0}, b[10];
  for (int i = 0; i < 24; ++i) A[i] = nb_xyz[i];
  for (int i = 0; i < 10; ++i) b[i] = -1.0f;
  const bool ok = m == 10 ? slio::cvs::qr_solve_mn<10, 3>(A, b, x) : slio::cvs::qr_solve_mn<8, 3>(A, b, x);
  if (!ok)
    for (int i = 0; i < 3; ++i) x[i] = 0.0f;
  return ok ? SLIO_OK : 1;
}

}  // extern "C"
