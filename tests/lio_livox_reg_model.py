"""LIO-Livox's ScanRegistration for Use_seg = 0 restated in numpy / Python from
the reference text (src/LIO-Livox/src/lio/LidarFeatureExtractor.cpp:
detectFeaturePoint :93-614, FeatureExtract :1218-1291, FeatureExtract_Mid
:1352-1401; ScanRegistration.cpp lidarCallBackPc2 :61-93), independent of
csrc/: the model of tests/test_lio_livox_reg_cpu.py and
tests/test_gpu_lio_livox_reg.py.

float is numpy.float32 with the reference's association order, double is
numpy.float64; an Eigen::Vector3d dot / squaredNorm is a0 + (a1 + a2), and
normalize() leaves a zero vector as it is (Eigen 3.3), as in
tests/livox_reg_model.py.  The per-point quantities that no other point's result
feeds (depth, the two ray angles, K, curvature, diffR, the two flatness tests of
the line-feature loop) are evaluated for all positions at once; everything that
the reference does in an order (the sorts, the parts, the flag and pick loops,
the strided line-feature loop, the write-back) is a Python loop in that order.
The two insertion sorts (:211-232) swap neighbours on a strict `<`, which is a
stable ascending sort; the model calls Python's stable sort.  A NaN curvature
or diffR (a non-finite intensity in a Pc2 cloud) has no place under `<`; as
include/slio_frontend.h states, NaN sorts as one class after every number.

Where the reference is undefined the model does what include/slio_frontend.h
states: cloudAngle and CloudFeatureFlag start at zero, thNumCurvSize is a
per-line value (so the picking loops use the K of the line's last loop position
m - 6), a line of more than 20000 points raises, the Pc2 path wants n_scans >=
4, an empty message gives empty clouds.  plane_judge's result is dead (:473,
:512) and is not evaluated.
"""
import numpy as np

F = np.float32
D = np.float64
MAX_LINE = 20000
MAX_SCANS = 6

HORIZON = dict(n_scans=6, lidar_type=0, num_curv_size=2, distance_faraway=100.0, num_flat=3, part_num=150,
               flat_threshold=0.02, break_corner_dis=1.0, lidar_nearest_dis=1.0, kdtree_corner_outlier_dis=0.2)
MID360 = dict(n_scans=4, lidar_type=2, num_curv_size=2, distance_faraway=30.0, num_flat=3, part_num=100,
              flat_threshold=0.02, break_corner_dis=1.0, lidar_nearest_dis=1.0, kdtree_corner_outlier_dis=0.2)

STATS = ("lines_k2", "lines_k3", "far_pick_beyond_numflat", "angle_pick", "pick300", "pick300_over_2",
         "skip_marked_by_previous_part", "previous_part_2_to_1", "gap_stopped_mark", "curvature_ties", "set150",
         "set100_left", "set100_right", "set101_cc", "set101_nan", "near_skipped", "stride1", "stride4")


class LineTooLong(Exception):
    pass


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


def _cdiv(a, b):
    """C's int division (truncation towards zero); b > 0."""
    return a // b if a >= 0 else -((-a) // b)


def detect(c, prm, st):
    """detectFeaturePoint on the finite points c (m, 4) of one line.  Returns
    (flags, visited, pointsLessSharp, pointsLessFlat)."""
    m = len(c)
    far, flat = F(prm["distance_faraway"]), F(prm["flat_threshold"])
    brk, near = F(prm["break_corner_dis"]), F(prm["lidar_nearest_dis"])
    num_flat, part_num = int(prm["num_flat"]), int(prm["part_num"])
    flag = [0] * m
    visited = np.zeros(m, np.uint8)
    if m <= 10:
        return np.array(flag, np.int32), visited, [], []
    X, Y, Z, I = (np.ascontiguousarray(c[:, k], F) for k in range(4))
    P64 = c[:, :3].astype(D)
    i = np.arange(5, m - 5)

    # ---- :151-203, all positions at once
    depth_all = np.sqrt(X * X + Y * Y + Z * Z)                       # float
    dis = depth_all[i]

    def ray_cos(a):
        cur = (P64[i, 0], P64[i, 1], P64[i, 2])
        d = (P64[a, 0] - cur[0], P64[a, 1] - cur[1], P64[a, 2] - cur[2])
        return _dot(d, cur) / (_norm(d) * _norm(cur))

    angle_last, angle_next = ray_cos(i - 1), ray_cos(i + 1)
    steep = (np.abs(angle_last) > 0.966) & (np.abs(angle_next) > 0.966)
    K = np.where((dis > far) | steep, 2, 3)
    curv = np.zeros(m, F)
    refl = np.zeros(m, F)
    for k in (2, 3):
        sel = i[K == k]
        d = [np.zeros(len(sel), F) for _ in range(3)]
        dr = F(-2 * k) * I[sel]
        for j in range(1, k + 1):
            for a, C in enumerate((X, Y, Z)):
                d[a] = d[a] + (C[sel - j] + C[sel + j])
            dr = dr + (I[sel - j] + I[sel + j])
        for a, C in enumerate((X, Y, Z)):
            d[a] = d[a] - F(2 * k) * C[sel]
        curv[sel] = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        refl[sel] = dr
    cloudAngle = np.zeros(m, np.int32)
    cloudAngle[i[steep]] = 1
    cloudDepth = np.zeros(m, F)
    cloudDepth[i] = dis
    K_line = int(K[-1])                     # what the serial loop leaves in thNumCurvSize
    st["lines_k2" if K_line == 2 else "lines_k3"] += 1
    flat_thr = flat * cloudDepth * flat * cloudDepth                               # float (:241)
    is_cand = curv < flat_thr
    is_rcand = (curv.astype(D) < D(0.7) * D(flat) * cloudDepth.astype(D) * D(flat) * cloudDepth.astype(D)) & \
        (refl.astype(D) > 20.0)                                                     # double (:290-292)
    is_far = cloudDepth > far
    step2 = np.zeros(m, F)                  # |p[a + 1] - p[a]|^2, float
    dx, dy, dz = X[1:] - X[:-1], Y[1:] - Y[:-1], Z[1:] - Z[:-1]
    step2[:-1] = dx * dx + dy * dy + dz * dz
    is_gap = step2.astype(D) > 0.02

    # ---- :205-297
    scanStartInd, scanEndInd = 5, m - 6
    owner = {}                              # position -> the part whose mark or pick is on it
    for j in range(part_num):
        sp = scanStartInd + _cdiv((scanEndInd - scanStartInd) * j, part_num)
        ep = scanStartInd + _cdiv((scanEndInd - scanStartInd) * (j + 1), part_num) - 1
        if ep < sp:
            continue
        cloudSortInd = sorted(range(sp, ep + 1), key=lambda q: (bool(np.isnan(curv[q])), curv[q]))
        reflectSortInd = sorted(range(sp, ep + 1), key=lambda q: (bool(np.isnan(refl[q])), refl[q]))
        if len(set(float(curv[q]) for q in range(sp, ep + 1))) < ep - sp + 1:
            st["curvature_ties"] += 1
        smallestPickedNum, sharpestPickedNum = 1, 1
        for ind in cloudSortInd:
            if flag[ind] != 0:
                if owner.get(ind, j) < j:
                    st["skip_marked_by_previous_part"] += 1
                continue
            if is_cand[ind]:
                flag[ind] = 3
                owner[ind] = j
                for l in range(1, K_line + 1):
                    if is_gap[ind + l - 1] or is_far[ind]:
                        if is_gap[ind + l - 1] and not is_far[ind]:
                            st["gap_stopped_mark"] += 1
                        break
                    flag[ind + l] = 1
                    owner[ind + l] = j
                for l in range(-1, -K_line - 1, -1):
                    if is_gap[ind + l] or is_far[ind]:
                        if is_gap[ind + l] and not is_far[ind]:
                            st["gap_stopped_mark"] += 1
                        break
                    if flag[ind + l] == 2 and ind + l < sp:
                        st["previous_part_2_to_1"] += 1
                    flag[ind + l] = 1
                    owner[ind + l] = j
        for k in range(ep - sp + 1):
            ind = cloudSortInd[k]
            if (flag[ind] == 3 and smallestPickedNum <= num_flat) or (flag[ind] == 3 and is_far[ind]) or \
                    cloudAngle[ind] == 1:
                if flag[ind] == 3 and smallestPickedNum > num_flat and cloudAngle[ind] != 1:
                    st["far_pick_beyond_numflat"] += 1
                if cloudAngle[ind] == 1 and not (flag[ind] == 3 and (smallestPickedNum <= num_flat or is_far[ind])):
                    st["angle_pick"] += 1
                smallestPickedNum += 1
                flag[ind] = 2
                owner[ind] = j
            idx = reflectSortInd[k]
            if is_rcand[idx] and sharpestPickedNum <= 3:
                sharpestPickedNum += 1
                st["pick300"] += 1
                if flag[idx] == 2:
                    st["pick300_over_2"] += 1
                flag[idx] = 300
                owner[idx] = j

    # ---- :301-403
    def stencil(s):
        out = []
        for C in (X, Y, Z):
            out.append(C[i + 4 * s] + C[i + 3 * s] - F(4) * C[i + 2 * s] + C[i + s] + C[i])
        return out[0] * out[0] + out[1] * out[1] + out[2] * out[2]

    left_flat = np.zeros(m, bool)
    right_flat = np.zeros(m, bool)
    left_flat[i] = stencil(-1) < flat * dis
    right_flat[i] = stencil(+1) < flat * dis

    def vec(a, b):
        """Eigen::Vector3d(p[a].x - p[b].x, ...): float differences, widened."""
        return (D(X[a] - X[b]), D(Y[a] - Y[b]), D(Z[a] - Z[b]))

    def fan(q, sign, K_, w, need_depth):
        acc = (D(0), D(0), D(0))
        for k in range(1, K_ + 1):
            if need_depth and depth_all[q - k] < F(1):         # temp_depth reads q - k in both loops
                continue
            t = _normalized(vec(q + sign * k, q))
            kw = D(k) / D(w)
            acc = (acc[0] + kw * t[0], acc[1] + kw * t[1], acc[2] + kw * t[2])
        return acc

    count_num = 1
    q = 5
    while q < m - 5:
        visited[q] = 1
        count_num = 4 if right_flat[q] else 1
        st["stride4" if count_num == 4 else "stride1"] += 1
        if left_flat[q] and right_flat[q]:
            norm_left, norm_right = fan(q, -1, 4, 10.0, False), fan(q, +1, 4, 10.0, False)
            cc = abs(_dot(norm_left, norm_right) / (_norm(norm_left) * _norm(norm_right)))
            last_dis, current_dis = _norm(vec(q - 4, q)), _norm(vec(q + 4, q))
            if cc < D(0.5) and last_dis > D(0.05) and current_dis > D(0.05):
                flag[q] = 150
                st["set150"] += 1
        q += count_num

    # ---- :407-578
    diff_right = np.sqrt(step2[i])                                  # |p[i + 1] - p[i]|, float
    diff_left = np.sqrt(step2[i - 1])                               # (p[i-1] - p[i])^2 = (p[i] - p[i-1])^2
    breaks = i[np.abs(diff_right - diff_left) > brk]
    for q in breaks:
        dr_, dl_ = np.sqrt(step2[q]), np.sqrt(step2[q - 1])
        depth_right, depth_left = depth_all[q + 1], depth_all[q - 1]
        left = bool(dr_ > dl_)
        surf_vector = vec(q - 1, q) if left else vec(q + 1, q)
        lidar_vector = (D(X[q]), D(Y[q]), D(Z[q]))
        cc = abs(_dot(surf_vector, lidar_vector) / (_norm(surf_vector) * _norm(lidar_vector)))
        if cc < D(0.95):
            if left:
                if depth_right > depth_left or depth_right == 0:
                    flag[q] = 100
            else:
                if depth_right < depth_left or depth_left == 0:
                    flag[q] = 100
        if flag[q] == 100:
            norm_front, norm_back = fan(q, -1, 3, 6.0, True), fan(q, +1, 3, 6.0, True)
            cc = abs(_dot(norm_front, norm_back) / (_norm(norm_front) * _norm(norm_back)))
            if cc < D(0.95):
                st["set100_left" if left else "set100_right"] += 1
            else:
                flag[q] = 101
                st["set101_nan" if np.isnan(cc) else "set101_cc"] += 1

    # ---- :591-613
    corner, surf = [], []
    d2 = X * X + Y * Y + Z * Z
    for q in range(5, m - 5):
        if flag[q] not in (2, 100, 150):
            continue
        if d2[q] < near * near:
            st["near_skipped"] += 1
            continue
        (surf if flag[q] == 2 else corner).append(q)
    return np.array(flag, np.int32), visited, corner, surf


def _x_kept(x, lidar_type):
    """:1243-1247 and ScanRegistration.cpp:72-76; NaN passes both tests."""
    x = np.asarray(x, F).astype(D)
    return ~(x < 0.01) if lidar_type in (0, 1) else ~(np.abs(x) < 0.01)


def _to_sec(t):
    """ros::Time().fromNSec(t).toSec(): sec + 1e-9 * nsec, double."""
    t = np.asarray(t, np.uint32).astype(np.int64)
    return (t // 1000000000).astype(D) + D(1e-9) * (t % 1000000000).astype(D)


def _finish(cloud, line_of, prm):
    """From the ingested cloud on (:1257-1290 / :1367-1400)."""
    n = len(line_of)
    vlines = [[] for _ in range(MAX_SCANS)]
    for ci in range(n):
        vlines[line_of[ci]].append(ci)
    if max(len(v) for v in vlines) > MAX_LINE:
        raise LineTooLong()
    st = dict.fromkeys(STATS, 0)
    flags, visited, lines = [], [], []
    for vl in vlines:
        pts = cloud[vl, :4] if vl else np.zeros((0, 4), F)
        c = pts[np.isfinite(pts[:, :3]).all(1)]
        f, v, corner, surf = detect(c, prm, st)
        # idx counts the line's finite points, vlines[l] all of them (:1276, :1280)
        for idx in corner:
            cloud[vl[idx], 6] = F(1.0)
        for idx in surf:
            cloud[vl[idx], 6] = F(2.0)
        flags.append(f)
        visited.append(v)
        lines.append(np.ascontiguousarray(c, F))
    lab = cloud[:, 6].astype(D) if n else np.zeros(0)
    corner_cloud = cloud[np.abs(lab - 1.0) < 1e-5]
    surf_cloud = cloud[np.abs(lab - 2.0) < 1e-5]
    return dict(cloud=cloud, corner=corner_cloud, surf=surf_cloud,
                counts=[n, len(corner_cloud), len(surf_cloud)],
                line_size=[len(v) for v in vlines], finite_size=[len(c) for c in lines],
                flags=flags, visited=visited, lines=lines, stats=st)


def feature_extract(prm, xyz, reflectivity, line, offset_time):
    """FeatureExtract (:1218-1291) on a CustomMsg as arrays."""
    with np.errstate(all="ignore"):
        xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
        line = np.asarray(line, np.uint8).astype(np.int32)
        n = len(xyz)
        if n == 0:
            return _finish(np.zeros((0, 8), F), [], prm)
        timeSpan = _to_sec(offset_time[-1])
        keep = np.nonzero(~(line > prm["n_scans"] - 1) & _x_kept(xyz[:, 0], prm["lidar_type"]))[0]
        cloud = np.zeros((len(keep), 8), F)
        cloud[:, :3] = xyz[keep]
        cloud[:, 3] = np.asarray(reflectivity, np.uint8)[keep].astype(F)
        cloud[:, 4] = (_to_sec(np.asarray(offset_time)[keep]) / timeSpan).astype(F)
        cloud[:, 5] = line[keep].astype(np.int32).view(F)                         # _int_as_float
        return _finish(cloud, [int(v) for v in line[keep]], prm)


def feature_extract_mid(prm, xyzi):
    """lidarCallBackPc2 (ScanRegistration.cpp:61-93) with FeatureExtract_Mid
    (:1352-1401)."""
    if prm["n_scans"] < 4:
        raise ValueError("line = i % 4 needs n_scans >= 4")
    with np.errstate(all="ignore"):
        xyzi = np.ascontiguousarray(xyzi, F).reshape(-1, 4)
        n = len(xyzi)
        k = np.arange(n)
        keep = np.nonzero(_x_kept(xyzi[:, 0], prm["lidar_type"]))[0]
        cloud = np.zeros((len(keep), 8), F)
        cloud[:, :4] = xyzi[keep]
        cloud[:, 4] = k[keep].astype(F) / F(max(n, 1))
        cloud[:, 5] = (k[keep] % 4).astype(F)
        return _finish(cloud, [int(v) for v in k[keep] % 4], prm)
