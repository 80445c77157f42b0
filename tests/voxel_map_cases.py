"""The voxel map's test cases, shared by test_voxel_map_model.py (their premises, proved on the
restatement) and test_gpu_voxel_map.py (the device against the restatement, bit for bit).

A case is (name, params, steps); a step is ("update", scan (n, 6) float32, pose 4×4 or None) or
("rebase", pose).  Normals are random unit vectors: they only have to travel with their points.
"""
import math

import numpy as np

from model_restatement import make_pose

INF = float("inf")
F = np.float32


def with_normals(xyz, seed=0):
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    rng = np.random.default_rng(1000 + seed)
    nrm = rng.normal(size=(len(xyz), 3))
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-12)
    return np.concatenate([xyz, nrm.astype(np.float32)], axis=1)


def cloud(n, seed, half=20.0):
    rng = np.random.default_rng(seed)
    return with_normals(rng.uniform(-half, half, size=(n, 3)), seed)


POSE_A = make_pose(yaw=0.3, pitch=-0.05, roll=0.02, t=(1.25, -0.75, 0.1))
POSE_B = make_pose(yaw=-1.1, pitch=0.2, roll=-0.3, t=(-3.5, 2.0, 0.4))
POSE_FAR = make_pose(t=(1000.5, -2000.25, 30.0))          # pure translation, exactly representable
REBASE = make_pose(yaw=math.radians(10.0), t=(0.13, -0.07, 0.02))


def in_voxel(index, n, voxel, seed):
    """n points strictly inside the voxel with integer index (ix, iy, iz)."""
    rng = np.random.default_rng(seed)
    return (np.asarray(index, dtype=np.float64) + rng.uniform(0.1, 0.9, size=(n, 3))) * voxel


# ---- sizes and cap ------------------------------------------------------------------------------
def size_cases():
    out = []
    for n in (0, 1, 255, 256, 257, 4097):
        out.append((f"size_{n}", dict(), [("update", cloud(n, n + 1), None), ("update", cloud(300, n + 2), POSE_A),
                                          ("update", cloud(n, n + 3), POSE_B)]))
    bad = cloud(300, 7)
    bad[0::3, 0] = np.nan
    bad[1::3, 1] = np.inf
    bad[2::3, 2] = -np.inf
    out.append(("all_nan_first", dict(), [("update", bad, None), ("update", cloud(100, 8), POSE_A)]))
    out.append(("all_nan_second", dict(), [("update", cloud(500, 9), None), ("update", bad, POSE_A)]))
    mixed = cloud(1000, 10)
    mixed[5::7, 1] = np.nan
    out.append(("some_nan", dict(), [("update", mixed, POSE_A), ("update", mixed, POSE_B)]))
    # the sensor moves 5 km: every old row is out of range and the scan brings nothing
    far = make_pose(t=(5000.0, 0.0, 0.0))
    out.append(("emptied_by_range", dict(max_range=50.0),
                [("update", cloud(400, 11), None), ("update", cloud(0, 0), far), ("update", cloud(50, 12), far)]))
    out.append(("cap_1", dict(max_per_voxel=1, voxel_size=1.0), [("update", cloud(3000, 13), None), ("update", cloud(3000, 14), POSE_A)]))
    return out


CAP_EDGE_CAP = 5
CAP_EDGE_VOXELS = {(3, -2, 1): (2, 2), (-4, 0, 0): (3, 2), (0, 5, -1): (4, 2)}   # voxel: rows of update 1, of update 2


def cap_edge_case():
    """Three voxels reaching cap − 1, cap and cap + 1 across two updates."""
    a = np.concatenate([in_voxel(v, c[0], 0.5, 20 + k) for k, (v, c) in enumerate(CAP_EDGE_VOXELS.items())])
    b = np.concatenate([in_voxel(v, c[1], 0.5, 30 + k) for k, (v, c) in enumerate(CAP_EDGE_VOXELS.items())])
    return ("cap_edge", dict(max_per_voxel=CAP_EDGE_CAP), [("update", with_normals(a, 1), None), ("update", with_normals(b, 2), None)])


# ---- segments and compaction --------------------------------------------------------------------
SEGMENT_START, SEGMENT_ROWS = 200, 700


def segment_scan():
    """200 lone rows with smaller keys, 700 rows in voxel (0, 0, 0), 100 lone rows after, shuffled."""
    lo = np.concatenate([in_voxel((-1 - k, 0, 0), 1, 0.5, 100 + k) for k in range(SEGMENT_START)])
    mid = in_voxel((0, 0, 0), SEGMENT_ROWS, 0.5, 40)
    hi = np.concatenate([in_voxel((1 + k, 0, 0), 1, 0.5, 400 + k) for k in range(100)])
    rows = np.concatenate([lo, mid, hi])
    return with_normals(rows[np.random.default_rng(41).permutation(len(rows))], 3)


def segment_cases():
    scan, more = segment_scan(), with_normals(in_voxel((0, 0, 0), 10, 0.5, 42), 4)
    out = [(f"segment_cap_{cap}", dict(max_per_voxel=cap), [("update", scan, None), ("update", more, None)])
           for cap in (1, 20, 699, 700, 701)]
    big = with_normals(in_voxel((2, 3, -4), 10000, 0.5, 43), 5)
    out.append(("one_voxel_10000_cap_20", dict(max_per_voxel=20), [("update", big, None), ("update", big[:100], None)]))
    out.append(("one_voxel_10000_cap_9999", dict(max_per_voxel=9999), [("update", big, None), ("update", big[:100], None)]))
    # two rows per voxel, cap 1: kept and dropped rows alternate along the whole sorted order
    pairs = np.concatenate([in_voxel((k % 60 - 30, k // 60 - 25, 0), 2, 0.5, 500 + k) for k in range(3000)])
    out.append(("alternating", dict(max_per_voxel=1), [("update", with_normals(pairs, 6), None), ("update", with_normals(pairs[::-1], 7), None)]))
    return out


# ---- voxel boundaries ---------------------------------------------------------------------------
BOUNDARY_VOXELS = (0.5, 0.3, 0.1)
BOUNDARY_K = (-7, -3, -1, 1, 2, 9)


def boundary_triples(voxel):
    """[(label, sentinel coordinate float32, k)]: for the boundary k·voxel, the float nearest to it and
    one float ulp either side; around zero: −0.0, +0.0 and tiny values of both signs (k = 0)."""
    v = np.float64(np.float32(voxel))
    out = []
    for k in BOUNDARY_K:
        b = np.float32(k * v)
        out += [(f"{k}v-ulp", np.nextafter(b, F(-np.inf)), k), (f"{k}v", b, k), (f"{k}v+ulp", np.nextafter(b, F(np.inf)), k)]
    tiny = np.nextafter(F(0), F(1))                       # the smallest denormal
    out += [("-0.0", F(-0.0), 0), ("+0.0", F(0.0), 0), ("-tiny", -tiny, 0), ("+tiny", tiny, 0), ("-1e-30", F(-1e-30), 0),
            ("+1e-30", F(1e-30), 0)]
    return out


def boundary_rows(voxel, axis):
    """Every sentinel alone at its own place along another axis, each with a companion in the middle of
    the voxel below the boundary (index k − 1): (rows (2m, 3): sentinel, companion, …; labels)."""
    rows, labels = [], []
    for j, (label, c, k) in enumerate(boundary_triples(voxel)):
        other = [(10 * j + 0.5) * voxel, 0.5 * voxel]     # a row of its own along the next axis
        for value in (np.float64(c), (k - 0.5) * np.float64(np.float32(voxel))):
            p = [0.0, 0.0, 0.0]
            p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = value, other[0], other[1]
            rows.append(p)
        labels.append(label)
    return np.asarray(rows, dtype=np.float32), labels


def boundary_cases():
    out = []
    for voxel in BOUNDARY_VOXELS:
        for axis in range(3):
            rows, _ = boundary_rows(voxel, axis)
            out.append((f"boundary_v{voxel}_axis{axis}", dict(voxel_size=voxel, max_per_voxel=1),
                        [("update", with_normals(rows, 8), None), ("update", with_normals(rows, 9), None)]))
    return out


GRID_EDGE = [(-524288.0, True), (-524288.5, False), (524287.5, True), (524288.0, False)]   # voxel 0.5: index −2²⁰, −2²⁰−1, 2²⁰−1, 2²⁰


def grid_edge_case():
    rows = []
    for axis in range(3):
        for c, _ in GRID_EDGE:
            p = [1.25, 1.25, 1.25]
            p[axis] = c
            rows.append(p)
    scan = with_normals(rows, 10)
    # second step: a rebase pushes the edge rows of the old map over the edge (map_out_of_grid)
    return ("grid_edge", dict(voxel_size=0.5, max_range=INF),
            [("update", scan, None), ("rebase", make_pose(t=(-1.0, -1.0, -1.0))), ("update", scan, None)])


# ---- range --------------------------------------------------------------------------------------
RANGE_TRIPLES = [((3.0, 4.0, 12.0), 13.0), ((2.0, 3.0, 6.0), 7.0), ((-8.0, 9.0, -12.0), 17.0)]


def range_scan(limit, pose):
    """Per triple of that limit: the point at exactly the limit and the one whose STORED z is a float
    ulp farther from the sensor.  pose is None or a pure translation t with t + p exact in float, so
    the scan row is the stored point minus t, also exact."""
    t = np.zeros(3) if pose is None else np.asarray(pose, dtype=np.float64)[:3, 3]
    rows = []
    for p, r in RANGE_TRIPLES:
        if r != limit:
            continue
        rows.append(p)
        stored_z = np.nextafter(F(t[2] + p[2]), F(np.copysign(np.inf, p[2])))
        z = F(np.float64(stored_z) - t[2])
        assert np.float64(z) + t[2] == np.float64(stored_z) and F(np.float64(z) + t[2]) == stored_z
        rows.append((p[0], p[1], z))
    return with_normals(rows, 11)


def range_cases():
    out = []
    for _, r in RANGE_TRIPLES:
        for name, pose in (("origin", None), ("far", POSE_FAR)):
            out.append((f"range_{int(r)}_{name}", dict(max_range=r, voxel_size=0.5),
                        [("update", range_scan(r, pose), pose), ("update", cloud(200, 50, 30.0), pose)]))
    wide = cloud(2000, 51, 5.0e4)
    out.append(("range_inf", dict(max_range=INF), [("update", wide, None), ("update", wide[:500], POSE_FAR)]))
    # the sensor moves: old rows fall out of range behind it
    steps = [("update", cloud(1500, 60 + k, 25.0), make_pose(yaw=0.1 * k, t=(12.0 * k, -3.0 * k, 0.5 * k))) for k in range(4)]
    out.append(("moving_sensor", dict(max_range=30.0), steps))
    return out


# ---- rebase -------------------------------------------------------------------------------------
def rebase_case():
    """A dense map at cap, re-expressed off the grid: voxels of the new frame hold more than cap rows, so
    the next update trims old rows (map_trimmed)."""
    dense = cloud(6000, 70, 3.0)
    return ("rebase_trims", dict(max_per_voxel=5, voxel_size=0.5),
            [("update", dense, POSE_A), ("update", cloud(2000, 71, 3.0), POSE_B), ("rebase", REBASE),
             ("update", cloud(500, 72, 3.0), POSE_A), ("rebase", np.eye(4)), ("update", cloud(10, 73, 3.0), None)])


def overflow_case():
    """Finite scan rows whose map-frame float is not finite: +inf by overflow under a finite translation,
    NaN from inf − inf under an extreme (finite) pose.  The non-finite test is on the row as given, so
    these are stored-float failures of the grid test (scan_out_of_grid), not scan_nonfinite."""
    far = float(F(3.0e38))                                # a float, so that −far + far is exactly 0
    big = make_pose(t=(far, 0.0, 0.0))
    scan = with_normals([[far, 0.0, 0.0], [-far, 1.0, 1.0], [1.0, 2.0, 3.0], [np.nan, 0.0, 0.0]], 12)
    wild = np.eye(4)
    wild[0, 0], wild[0, 1] = 1.0e300, -1.0e300
    scan2 = with_normals([[1.0e30, 1.0e30, 0.0], [0.0, 0.0, 0.5], [np.inf, 0.0, 0.0]], 13)
    return ("overflow", dict(max_range=INF), [("update", scan, big), ("update", scan2, wild)])


def all_cases():
    return (size_cases() + [cap_edge_case()] + segment_cases() + boundary_cases() + [grid_edge_case()] + range_cases() +
            [rebase_case(), overflow_case()])


def run_on_restatement(case):
    """[(map rows, info, classes) after each update step] of a case on the numpy restatement."""
    import voxel_map_np as vnp
    _, params, steps = case
    vm = vnp.VoxelMap(**params)
    out = []
    for step in steps:
        if step[0] == "rebase":
            vm.rebase(step[1])
            continue
        rows, info, cls = vnp.update(vm.rows, step[1], step[2], classes=True, **vm.params)
        vm.rows, vm.info = rows, info
        out.append((rows, info, cls, len(step[1])))
    return out
