"""numpy float32 restatement of LeGO-LOAM's loop closure as include/slio.h
specifies it (slio_lmap_detect_loop, slio_lmap_loop_clouds,
slio_lmap_loop_correction, the recent-keyframe list of
extractSurroundingKeyFrames).  No device, no library: the transform is
lego_map_model.to_map, the VoxelGrid the oracle's, the ICP icp_model's.
path:line are in src/LeGO-LOAM/LeGO-LOAM/src/mapOptmization.cpp."""
from collections import deque

import numpy as np

import lego_map_model as M
from lego_odom_model import F, fasin, fatan2, fcos, fsin


# ------------------------------------------------------------------ detectLoopClosure's search (:863-887)
def detect_loop(key_xyz, key_time, cur, t, radius=5.0, time_diff=30.0):
    """The radius search's hits in ascending float squared distance (stable:
    equal distances by lower key); the first more than time_diff away wins."""
    p = np.ascontiguousarray(key_xyz, F).reshape(-1, 3)
    if p.shape[0] == 0:
        return -1
    d = p - np.asarray(cur, F).reshape(3)
    sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert sq.dtype == F
    order = np.argsort(sq, kind="stable")
    order = order[sq[order] < F(radius) * F(radius)]
    for k in order:
        if abs(float(key_time[k]) - float(t)) > time_diff:
            return int(k)
    return -1


# ------------------------------------------------------------------ the recent-keyframe list (:1044-1089)
class RecentList:
    """recent*CloudKeyFrames as a deque of key numbers, and latestFrameID
    (0 at construction, :390)."""

    def __init__(self, search_num=50):
        self.q = deque()
        self.latest_frame_id = 0
        self.search_num = search_num

    def update(self, num_poses):
        """One call of extractSurroundingKeyFrames with num_poses keys."""
        if len(self.q) < self.search_num:
            self.q.clear()
            for i in range(num_poses - 1, -1, -1):
                self.q.appendleft(i)
                if len(self.q) >= self.search_num:
                    break
        elif self.latest_frame_id != num_poses - 1:
            self.q.popleft()
            self.latest_frame_id = num_poses - 1
            self.q.append(self.latest_frame_id)
        return list(self.q)

    def correct_poses(self):
        self.q.clear()


def local_maps(voxel_grid, kfs, poses, keys, leaf_corner=0.2, leaf_surf=0.4):
    """:1091-1097 and the two VoxelGrids: kfs[k] = (corner, surf, outlier) of
    key k.  Returns (corner concatenation, surf concatenation, corner map,
    surf map)."""
    cc = np.concatenate([M.to_map(poses[k], kfs[k][0]) for k in keys] or [np.zeros((0, 3), F)])
    sc = np.concatenate([np.concatenate([M.to_map(poses[k], kfs[k][1]), M.to_map(poses[k], kfs[k][2])])
                         for k in keys] or [np.zeros((0, 3), F)])
    return cc, sc, voxel_grid(cc, leaf_corner), voxel_grid(sc, leaf_surf)


# ------------------------------------------------------------------ detectLoopClosure's clouds (:889-931)
def loop_clouds(voxel_grid, kfs, poses, latest, closest, search_num, leaf=0.4):
    """(source, target concatenation, target): the source is key `latest`'s
    corner then surf cloud at its pose, not downsampled; the target the keys
    closest - search_num .. closest + search_num inside [0, latest], corner
    then surf of each, through the VoxelGrid."""
    src = np.concatenate([M.to_map(poses[latest], kfs[latest][0]), M.to_map(poses[latest], kfs[latest][1])])
    parts = []
    for j in range(-search_num, search_num + 1):
        k = closest + j
        if k < 0 or k > latest:
            continue
        parts += [M.to_map(poses[k], kfs[k][0]), M.to_map(poses[k], kfs[k][1])]
    cat = np.concatenate(parts)
    return src, cat, voxel_grid(cat, leaf)


# ------------------------------------------------------------------ the correction (:992-1012)
def get_transformation(x, y, z, roll, pitch, yaw):
    """pcl::getTransformation in float32, rows 0..2."""
    A, B, C, D, E, Fs = fcos(yaw), fsin(yaw), fcos(pitch), fsin(pitch), fcos(roll), fsin(roll)
    DE, DF = D * E, D * Fs
    t = np.array([[A * C, A * DF - B * E, B * Fs + A * DE, x],
                  [B * C, A * E + B * DF, B * DE - A * Fs, y],
                  [-D, C * Fs, C * E, z]], F)
    assert all(isinstance(v, F) for v in (DE, DF, A * C))
    return t


def translation_and_euler(t):
    """pcl::getTranslationAndEulerAngles: x, y, z, roll, pitch, yaw."""
    return (F(t[0, 3]), F(t[1, 3]), F(t[2, 3]), fatan2(t[2, 1], t[2, 2]), fasin(-t[2, 0]), fatan2(t[1, 0], t[0, 0]))


def affine_product(a, b):
    """Eigen's Affine3f product: linear = La Lb, translation = La tb + ta,
    every sum in index order, float32."""
    out = np.zeros((3, 4), F)
    for r in range(3):
        for c in range(3):
            out[r, c] = F(F(a[r, 0] * b[0, c] + a[r, 1] * b[1, c]) + a[r, 2] * b[2, c])
        out[r, 3] = F(F(F(a[r, 0] * b[0, 3] + a[r, 1] * b[1, 3]) + a[r, 2] * b[2, 3]) + a[r, 3])
    return out


def loop_correction(final_T, latest_pose6, closest_pose6, fitness):
    """(pose_from, pose_to, noise), all float32."""
    T = np.asarray(final_T, F).reshape(4, 4)
    x, y, z, roll, pitch, yaw = translation_and_euler(T)
    corr = get_transformation(z, x, y, yaw, roll, pitch)
    p = np.asarray(latest_pose6, F)
    wrong = get_transformation(p[5], p[3], p[4], p[2], p[0], p[1])
    ok = affine_product(corr, wrong)
    pose_from = np.array(translation_and_euler(ok), F)
    q = np.asarray(closest_pose6, F)
    pose_to = np.array([q[5], q[3], q[4], q[2], q[0], q[1]], F)
    return pose_from, pose_to, F(fitness)


def table_pose(pose_from):
    """A GTSAM pose {x, y, z, roll, pitch, yaw} as the key-pose table holds it
    (:1775-1794): {rx, ry, rz, tx, ty, tz} = {pitch, yaw, roll, y, z, x}."""
    g = np.asarray(pose_from, F)
    return np.array([g[4], g[5], g[3], g[1], g[2], g[0]], F)
