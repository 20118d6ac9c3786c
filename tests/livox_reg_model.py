"""numpy restatement of livox_mapping's scanRegistration
(src/livox_mapping/src/scanRegistration.cpp, laserCloudHandler :152-534), in
the manner of tests/livox_map_model.py: the literal serial loops, one
np.float32 operation per float operation of the reference and one np.float64
operation per double operation, in the reference's order, with the promotions
the reference makes (a float compared against a double literal is widened
first).  It shares no code with the library.  cv::eigen is
tests/lego_map_model.py's restatement of hal::Jacobi.

Conventions, as everywhere in these models: sqrt of a float is the double
function rounded to float, std::atan2 of two floats likewise.  Eigen:
dot / squaredNorm of a Vector3d in the unrolled order a0 + (a1 + a2),
normalize() of 3.3 (a zero vector stays as it is), true division.

The yardstick of tests/test_livox_reg_cpu.py and tests/test_gpu_livox_reg.py.
"""
import math

import numpy as np

import lego_map_model as LM
from lego_odom_model import F, fatan2, fsqrt

D = np.float64
MAX_POINTS = 32000
STATS = ("stride1", "stride4", "left_surf", "right_surf", "set150", "outlier", "break_left", "break_right",
         "set100", "kept100", "reset100", "reset_erased")


def scan_id(y, z):
    """:166-171."""
    theta = D(fatan2(y, z)) / D(math.pi) * D(180) + D(180)
    return int(math.floor(theta / D(9)))


def theta_over_9(y, z):
    return float(D(fatan2(y, z)) / D(math.pi) * D(180) + D(180)) / 9.0


def plane_judge(pts, threshold):
    """:64-120 on a list of (x, y, z) float32."""
    num = len(pts)
    cx = cy = cz = F(0)
    for p in pts:
        cx = cx + p[0]
        cy = cy + p[1]
        cz = cz + p[2]
    cx, cy, cz = cx / F(num), cy / F(num), cz / F(num)
    a11 = a12 = a13 = a22 = a23 = a33 = F(0)
    for p in pts:
        ax, ay, az = p[0] - cx, p[1] - cy, p[2] - cz
        a11 = a11 + ax * ax
        a12 = a12 + ax * ay
        a13 = a13 + ax * az
        a22 = a22 + ay * ay
        a23 = a23 + ay * az
        a33 = a33 + az * az
    n = F(num)
    a11, a12, a13, a22, a23, a33 = a11 / n, a12 / n, a13 / n, a22 / n, a23 / n, a33 / n
    W, _ = LM.jacobi([a11, a12, a13, a12, a22, a23, a13, a23, a33], 3)
    return bool(W[0] > F(threshold) * W[1])


def _dot(a, b):
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])


def _norm(a):
    return np.sqrt(_dot(a, a))


def _normalized(a):
    z = _dot(a, a)
    if z > 0:
        s = np.sqrt(z)
        return (a[0] / s, a[1] / s, a[2] / s)
    return a


def register(cloud):
    """laserCloudHandler.  Returns dict(flags, visited, cloud, corner, surf,
    counts, stats)."""
    with np.errstate(all="ignore"):
        return _register(np.ascontiguousarray(cloud, F).reshape(-1, 4))


def _register(inp):
    # :157-187
    cloudSize = min(len(inp), MAX_POINTS)
    X, Y, Z, I = [], [], [], []
    for i in range(cloudSize):
        x, y, z, inten = inp[i]
        if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
            continue
        X.append(x)
        Y.append(y)
        Z.append(z)
        I.append(F(scan_id(y, z)) + inten / F(10000))
    N = len(X)
    flag = [0] * N
    visited = np.zeros(N, np.uint8)
    st = dict.fromkeys(STATS, 0)

    def vec(a, b):
        """Eigen::Vector3d(p[a].x - p[b].x, ...): float differences, widened."""
        return (D(X[a] - X[b]), D(Y[a] - Y[b]), D(Z[a] - Z[b]))

    def depth_of(i):
        return fsqrt(X[i] * X[i] + Y[i] * Y[i] + Z[i] * Z[i])

    def fan_cos(i, K, w):
        a = (D(0), D(0), D(0))
        for k in range(1, K + 1):
            t = _normalized(vec(i - k, i))
            kw = D(k) / D(w)
            a = (a[0] + kw * t[0], a[1] + kw * t[1], a[2] + kw * t[2])
        b = (D(0), D(0), D(0))
        for k in range(1, K + 1):
            t = _normalized(vec(i + k, i))
            kw = D(k) / D(w)
            b = (b[0] + kw * t[0], b[1] + kw * t[1], b[2] + kw * t[2])
        return abs(_dot(a, b) / (_norm(a) * _norm(b)))

    # loop 1 (:212-325)
    count_num = 1
    i = 5
    while i < N - 5:
        visited[i] = 1
        ld = [C[i - 4] + C[i - 3] - F(4) * C[i - 2] + C[i - 1] + C[i] for C in (X, Y, Z)]
        left_curvature = ld[0] * ld[0] + ld[1] * ld[1] + ld[2] * ld[2]
        if D(left_curvature) < D(0.01):
            if D(left_curvature) < D(0.001):
                flag[i - 2] = 1
                st["left_surf"] += 1
            left_surf_flag = True
        else:
            left_surf_flag = False
        rd = [C[i + 4] + C[i + 3] - F(4) * C[i + 2] + C[i + 1] + C[i] for C in (X, Y, Z)]
        right_curvature = rd[0] * rd[0] + rd[1] * rd[1] + rd[2] * rd[2]
        if D(right_curvature) < D(0.01):
            if D(right_curvature) < D(0.001):
                flag[i + 2] = 1
                st["right_surf"] += 1
            count_num = 4
            right_surf_flag = True
        else:
            count_num = 1
            right_surf_flag = False
        st["stride4" if count_num == 4 else "stride1"] += 1
        if left_surf_flag and right_surf_flag:
            cc = fan_cos(i, 4, 10.0)
            last_dis, current_dis = _norm(vec(i - 4, i)), _norm(vec(i + 4, i))
            if cc < D(0.5) and last_dis > D(0.05) and current_dis > D(0.05):
                flag[i] = 150
                st["set150"] += 1
        i += count_num

    # loop 2 (:327-483)
    for i in range(5, N - 5):
        depth = depth_of(i)
        d1 = (X[i + 1] - X[i], Y[i + 1] - Y[i], Z[i + 1] - Z[i])
        diff_right = fsqrt(d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2])
        d2 = (X[i - 1] - X[i], Y[i - 1] - Y[i], Z[i - 1] - Z[i])
        diff_left = fsqrt(d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2])
        depth_right, depth_left = depth_of(i + 1), depth_of(i - 1)
        if D(diff_right) > D(0.1) * D(depth) and D(diff_left) > D(0.1) * D(depth):
            st["outlier"] += 1
            flag[i] = 250
            continue
        before = flag[i]
        if D(abs(diff_right - diff_left)) > D(0.1):
            left = bool(diff_right > diff_left)
            st["break_left" if left else "break_right"] += 1
            s = -1 if left else 1
            surf_vector = vec(i + 4 * s, i)
            lidar_vector = (D(X[i]), D(Y[i]), D(Z[i]))
            surf_dis = _norm(surf_vector)
            cc = abs(_dot(surf_vector, lidar_vector) / (_norm(surf_vector) * _norm(lidar_vector)))
            lst = []
            min_dis, max_dis = D(10000), D(0)
            for j in range(4):
                lst.append((X[i - j], Y[i - j], Z[i - j]))       # p[i - j] on both sides (:384, :423)
                temp_vector = vec(i + s * j, i + s * (j + 1))
                if j == 3:
                    break
                temp_dis = _norm(temp_vector)
                if temp_dis < min_dis:
                    min_dis = temp_dis
                if temp_dis > max_dis:
                    max_dis = temp_dis
            is_plane = plane_judge(lst, 100)
            if is_plane and max_dis < D(2) * min_dis and surf_dis < D(0.05) * D(depth) and cc < D(0.8):
                if left:
                    if depth_right > depth_left:
                        flag[i] = 100
                    elif depth_right == 0:
                        flag[i] = 100
                else:
                    if depth_right < depth_left:
                        flag[i] = 100
                    elif depth_left == 0:
                        flag[i] = 100
        if flag[i] == 100:
            st["set100"] += 1
            cc = fan_cos(i, 3, 6.0)
            if cc < D(0.8):
                st["kept100"] += 1
            else:
                flag[i] = 0
                st["reset100"] += 1
                if before != 0:
                    st["reset_erased"] += 1

    # :486-508
    full = np.array([X, Y, Z, I], F).T.reshape(-1, 4) if N else np.zeros((0, 4), F)
    fl = np.array(flag, np.int32)
    surf = full[fl == 1]
    corner = full[(fl == 100) | (fl == 150)]
    return dict(flags=fl, visited=visited, cloud=np.ascontiguousarray(full), corner=np.ascontiguousarray(corner),
                surf=np.ascontiguousarray(surf), counts=np.array([N, len(corner), len(surf)], np.int32), stats=st)
