"""The voxel map's definition (include/imls_gpu.h "voxel map") restated in numpy: the
reference every device result is compared with bit for bit.

update(): candidates = the old map's rows in stored order, then the scan's surviving rows in scan
order; the voxel index floor(double(c) / double(voxel_size)) per axis from the stored floats; the
range test against the pose's translation; a stable argsort by key (older rows first within a key);
the rank inside a key from np.maximum.accumulate over the segment heads; the first max_per_voxel stay.

drive_voxel(): model_restatement.drive with this map in place of the posed FIFO.
"""
import numpy as np

import oracle_ctypes as oc
from model_restatement import inv_pose, pose_cloud, register_from, soa6, xyzn

INFO_KEYS = ("points", "voxels", "scan_inserted", "scan_nonfinite", "scan_out_of_grid", "scan_out_of_range", "scan_full",
             "map_out_of_grid", "map_out_of_range", "map_trimmed")
GRID_LO, GRID_HI = -float(2 ** 20), float(2 ** 20 - 1)
DEFAULTS = dict(voxel_size=0.5, max_per_voxel=20, max_range=100.0)


def enter_map_frame(scan, pose):
    """Step 1 for every row (non-finite rows left as given): an identity pose keeps the bits."""
    a = xyzn(scan).reshape(-1, 6)
    T = np.asarray(pose, dtype=np.float64).reshape(4, 4)
    if np.array_equal(T, np.eye(4)):
        return a.copy()
    return pose_cloud(a, T)


def voxel_index(pts, voxel_size):
    """(n, 3) float64 indices i_a = floor(double(c_a) / double(voxel_size)); NaN / inf pass through."""
    with np.errstate(all="ignore"):
        return np.floor(pts[:, :3].astype(np.float64) / np.float64(np.float32(voxel_size)))


def keys_of(idx):
    i = idx.astype(np.int64) + (1 << 20)
    return (i[:, 2] << 42) | (i[:, 1] << 21) | i[:, 0]


def update(old_map, scan, pose=None, voxel_size=0.5, max_per_voxel=20, max_range=100.0, classes=False):
    """(new map (m, 6) float32, info dict).  old_map: (n_old, 6) float32 rows in stored order.
    classes=True also returns, per candidate (old rows then ALL scan rows), the name of the class that
    dropped it, or "kept"."""
    T = np.eye(4) if pose is None else np.asarray(pose, dtype=np.float64).reshape(4, 4)
    old = np.asarray(old_map, dtype=np.float32).reshape(-1, 6)
    new = enter_map_frame(scan, T)
    n_old, n = len(old), len(new)
    cand = np.concatenate([old, new])
    is_old = np.arange(n_old + n) < n_old
    cls = np.full(n_old + n, "kept", dtype=object)
    # step 1 tests the scan row AS GIVEN: a finite row whose map-frame float overflows (or is NaN, from
    # inf − inf under an extreme pose) is a stored non-finite float, which fails the grid test below
    given = xyzn(scan).reshape(-1, 6)
    cls[n_old:][~np.isfinite(given[:, :3]).all(axis=1)] = "scan_nonfinite"
    idx = voxel_index(cand, voxel_size)
    with np.errstate(invalid="ignore"):
        in_grid = ((idx >= GRID_LO) & (idx <= GRID_HI)).all(axis=1)
    alive = cls == "kept"
    drop = alive & ~in_grid
    cls[drop & is_old], cls[drop & ~is_old] = "map_out_of_grid", "scan_out_of_grid"
    alive &= in_grid
    t = T[:3, 3]
    with np.errstate(all="ignore"):
        d = cand[:, :3].astype(np.float64) - t
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        r = np.float64(np.float32(max_range))
        in_range = d2 <= r * r
    drop = alive & ~in_range
    cls[drop & is_old], cls[drop & ~is_old] = "map_out_of_range", "scan_out_of_range"
    alive &= in_range
    surv = np.flatnonzero(alive)
    key = keys_of(idx[surv])
    order = np.argsort(key, kind="stable")
    sk, ss = key[order], surv[order]
    m = len(sk)
    head = np.ones(m, bool)
    head[1:] = sk[1:] != sk[:-1]
    pos = np.arange(m)
    rank = pos - np.maximum.accumulate(np.where(head, pos, 0)) if m else pos
    keep = rank < int(max_per_voxel)
    full = ss[~keep]
    cls[full[full < n_old]] = "map_trimmed"
    cls[full[full >= n_old]] = "scan_full"
    out = cand[ss[keep]].copy()
    info = {k: 0 for k in INFO_KEYS}
    for k in INFO_KEYS[3:]:
        info[k] = int((cls == k).sum())
    info["points"], info["voxels"] = len(out), int(head.sum())
    info["scan_inserted"] = int((cls[n_old:] == "kept").sum())
    return (out, info, cls) if classes else (out, info)


class VoxelMap:
    """The map as a context holds it: update / rebase / clear."""

    def __init__(self, **params):
        self.params = dict(DEFAULTS, **params)
        self.rows = np.zeros((0, 6), np.float32)
        self.info = {k: 0 for k in INFO_KEYS}

    def update(self, scan, pose=None):
        self.rows, self.info = update(self.rows, scan, pose, **self.params)
        return len(self.rows)

    def rebase(self, pose):
        if len(self.rows) and not np.array_equal(np.asarray(pose, dtype=np.float64).reshape(4, 4), np.eye(4)):
            self.rows = pose_cloud(self.rows, pose)

    def clear(self):
        self.rows = np.zeros((0, 6), np.float32)


def drive_voxel(frames, p, prior="none", rebase_distance=100.0, poses=None, **params):
    """LaserOdometry(map_model="voxel", motion_prior=prior, rebase_distance=…, voxel_map=params) on the
    oracle's steps: ([(rPose, iterations, status, nowPose)] per registered frame, [map rows after each
    frame's update], [info of each update]).  poses (optional): the map-frame pose T_A' to use for
    frame k in place of the oracle's own registration result (the device's, to compare maps bit for
    bit whatever the last-digit differences of the registrations)."""
    vm = VoxelMap(**params)
    prev, out, maps, infos = np.eye(4), [], [], []
    T_A, last = np.eye(4), np.eye(4)
    rs = oc.rand_state(p.ransac_seed)
    for k, (filtered, flat) in enumerate(frames):
        if k != 0:
            if poses is not None:
                T_new, iters, status = poses[k - 1], -1, -1
            else:
                init = oc.chain_pose(T_A, last) if prior == "constant_velocity" else T_A
                r = register_from(soa6(xyzn(flat)), soa6(vm.rows), p, init=init, rand_state=rs)
                T_new, iters, status = r["pose"], r["iters"], r["status"]
            rp = oc.chain_pose(inv_pose(T_A), T_new)
            T_A = np.array(T_new, dtype=np.float64)
            last = rp
            prev = oc.chain_pose(prev, rp)
            out.append((rp, iters, status, prev))
        vm.update(filtered, T_A)
        infos.append(dict(vm.info))
        if np.linalg.norm(T_A[:3, 3]) > rebase_distance:
            vm.rebase(inv_pose(T_A))
            T_A = np.eye(4)
        maps.append(vm.rows.copy())
    return out, maps, infos
