"""CPU: the voxel map's definition on its numpy restatement (voxel_map_np.py), and the premises of the
cases test_gpu_voxel_map.py runs on the device — a case that does not reach the edge it is named for
would pin nothing there."""
import numpy as np
import pytest

import voxel_map_cases as vc
import voxel_map_np as vnp
from model_restatement import pose_cloud

CASES = vc.all_cases()


def rows_set(a):
    """The multiset of (n, 6) float32 rows as sorted raw bytes."""
    return sorted(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).reshape(len(a), 6).tolist())


def test_saturation():
    """One scan pushed k times holds Σ_v min(cap, k·c_v) rows, then stops growing."""
    scan = vc.cloud(4000, 1, 4.0)
    cap, voxel = 4, 0.25
    idx = vnp.voxel_index(scan, voxel)
    _, counts = np.unique(vnp.keys_of(idx), return_counts=True)
    vm = vnp.VoxelMap(voxel_size=voxel, max_per_voxel=cap, max_range=float("inf"))
    sizes = []
    for k in range(1, 8):
        vm.update(scan)
        assert len(vm.rows) == int(np.minimum(cap, k * counts).sum())
        sizes.append(len(vm.rows))
    assert sizes[0] < sizes[1] and sizes[-1] == sizes[-2] == len(counts) * cap
    assert vm.info["scan_inserted"] == 0 and vm.info["scan_full"] == len(scan)


def test_multiset_identity():
    """cap ≥ n and max_range = inf: the map is the multiset of the posed clouds."""
    scans = [(vc.cloud(700, 2), None), (vc.cloud(900, 3), vc.POSE_A), (vc.cloud(500, 4), vc.POSE_B)]
    vm = vnp.VoxelMap(max_per_voxel=10 ** 6, max_range=float("inf"))
    want = []
    for scan, pose in scans:
        vm.update(scan, pose)
        want.append(scan if pose is None else pose_cloud(scan, pose))
    assert rows_set(vm.rows) == rows_set(np.concatenate(want))
    key = vnp.keys_of(vnp.voxel_index(vm.rows, 0.5))
    assert np.all(np.diff(key) >= 0)


def test_identity_pose_keeps_the_bits():
    scan = vc.with_normals([[-0.0, 0.0, -0.0], [1.0, -0.0, 2.0]], 1)
    scan[:, 3:] = np.float32(-0.0)
    out, _ = vnp.update(np.zeros((0, 6), np.float32), scan, np.eye(4), max_range=float("inf"))
    assert rows_set(out) == rows_set(scan)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_one_class_per_dropped_row(case):
    """Every candidate of every step is kept or falls in exactly one class; the counters add up."""
    n_old = 0
    for rows, info, cls, n in vc.run_on_restatement(case):
        assert len(cls) == n_old + n
        names = set(cls.tolist())
        assert names <= {"kept"} | set(vnp.INFO_KEYS[3:])
        assert set(cls[:n_old].tolist()) <= {"kept", "map_out_of_grid", "map_out_of_range", "map_trimmed"}
        assert set(cls[n_old:].tolist()) <= {"kept", "scan_nonfinite", "scan_out_of_grid", "scan_out_of_range", "scan_full"}
        assert sum(info[k] for k in ("scan_inserted", "scan_nonfinite", "scan_out_of_grid", "scan_out_of_range", "scan_full")) == n
        assert info["points"] == n_old - info["map_out_of_grid"] - info["map_out_of_range"] - info["map_trimmed"] + info["scan_inserted"]
        assert info["points"] == len(rows) == int((cls == "kept").sum())
        assert np.isfinite(rows[:, :3]).all()
        n_old = len(rows)
        if case[0].startswith("rebase") or case[0] == "grid_edge":
            continue
        assert info["map_trimmed"] == 0          # without a rebase the old map never exceeds the cap


def case_named(name):
    return next(c for c in CASES if c[0] == name)


def test_cap_edge_premise():
    (_, i1, _, _), (rows, i2, _, _) = vc.run_on_restatement(case_named("cap_edge"))
    assert i1["scan_full"] == 0 and i2["scan_full"] == 1 and i2["voxels"] == 3
    _, counts = np.unique(vnp.keys_of(vnp.voxel_index(rows, 0.5)), return_counts=True)
    cap = vc.CAP_EDGE_CAP
    assert sorted(counts.tolist()) == [cap - 1, cap, cap]
    assert sorted(a + b for a, b in vc.CAP_EDGE_VOXELS.values()) == [cap - 1, cap, cap + 1]


def test_segment_premise():
    """The 700-row voxel's sorted segment starts at 200: it crosses positions 256 and 512."""
    scan = vc.segment_scan()
    key = np.sort(vnp.keys_of(vnp.voxel_index(scan, 0.5)))
    big = vnp.keys_of(np.zeros((1, 3)))[0]
    pos = np.flatnonzero(key == big)
    assert pos[0] == vc.SEGMENT_START and len(pos) == vc.SEGMENT_ROWS and pos[-1] == pos[0] + len(pos) - 1
    for cap in (1, 20, 699, 700, 701):
        (_, i1, _, _), (_, i2, _, _) = vc.run_on_restatement(case_named(f"segment_cap_{cap}"))
        assert i1["scan_full"] == max(0, 700 - cap)
        assert i2["scan_inserted"] == max(0, min(10, cap - 700))


def test_alternating_premise():
    (rows, info, cls, n), _ = vc.run_on_restatement(case_named("alternating"))
    assert info["points"] == info["voxels"] == 3000 and info["scan_full"] == 3000


@pytest.mark.parametrize("voxel", vc.BOUNDARY_VOXELS)
def test_lone_occupants(voxel):
    """A sentinel is alone in its voxel above the boundary and joins its companion below it: moving
    it across the boundary changes `voxels`."""
    rows, labels = vc.boundary_rows(voxel, 0)
    got = {}
    for j, label in enumerate(labels):
        _, info = vnp.update(np.zeros((0, 6), np.float32), vc.with_normals(rows[2 * j:2 * j + 2]), None, voxel_size=voxel,
                             max_per_voxel=8, max_range=float("inf"))
        got[label] = info["voxels"]
    for k in vc.BOUNDARY_K:
        assert got[f"{k}v-ulp"] == 1 and got[f"{k}v+ulp"] == 2, (k, got)
        assert got[f"{k}v"] in (1, 2)
        if voxel == 0.5:
            assert got[f"{k}v"] == 2                    # k·2⁻¹ is exact: the boundary belongs to the voxel above
    # floor, not truncation: −0.0 is in voxel 0, every negative however small in voxel −1
    assert got["-0.0"] == got["+0.0"] == got["+tiny"] == got["+1e-30"] == 2
    assert got["-tiny"] == got["-1e-30"] == 1


def test_grid_edge_premise():
    steps = vc.run_on_restatement(case_named("grid_edge"))
    (rows, info, cls, n) = steps[0]
    want = ["kept" if ok else "scan_out_of_grid" for _ in range(3) for _, ok in vc.GRID_EDGE]
    assert cls.tolist() == want
    idx = vnp.voxel_index(rows, 0.5)
    assert idx.min() == -2 ** 20 and idx.max() == 2 ** 20 - 1
    assert steps[1][1]["map_out_of_grid"] == 3       # the rebase pushed the three low-edge rows out


@pytest.mark.parametrize("name", ["origin", "far"])
def test_range_premise(name):
    for _, r in vc.RANGE_TRIPLES:
        (rows, info, cls, n), second = vc.run_on_restatement(case_named(f"range_{int(r)}_{name}"))
        assert cls.tolist() == ["kept", "scan_out_of_range"]
        t = np.zeros(3) if name == "origin" else vc.POSE_FAR[:3, 3]
        d = rows[0, :3].astype(np.float64) - t
        assert d @ d == r * r                           # the kept row is at exactly max_range
    (rows, info, cls, n), _ = vc.run_on_restatement(case_named("range_inf"))
    assert info["scan_inserted"] == n and np.abs(rows[:, :3]).max() > 4.0e4
    steps = vc.run_on_restatement(case_named("moving_sensor"))
    assert all(s[1]["map_out_of_range"] > 0 for s in steps[1:])
    assert vc.run_on_restatement(case_named("emptied_by_range"))[1][1]["points"] == 0


def test_overflow_premise():
    """The non-finite test is on the scan row as given; a finite row whose stored float would be ±inf or
    NaN fails the grid test instead."""
    (rows, info, cls, n), (rows2, info2, cls2, n2) = vc.run_on_restatement(case_named("overflow"))
    assert cls.tolist() == ["scan_out_of_grid", "kept", "scan_out_of_grid", "scan_nonfinite"]
    case = case_named("overflow")
    posed = vnp.enter_map_frame(case[2][0][1], case[2][0][2])
    assert np.isposinf(posed[0, 0]) and np.isfinite(posed[2, 0])
    posed2 = vnp.enter_map_frame(case[2][1][1], case[2][1][2])
    assert np.isnan(posed2[0, 0])
    assert cls2.tolist() == ["kept", "scan_out_of_grid", "kept", "scan_nonfinite"]


def test_rebase_premise():
    steps = vc.run_on_restatement(case_named("rebase_trims"))
    assert steps[2][1]["map_trimmed"] > 0 and steps[3][1]["map_trimmed"] == 0
    assert steps[0][1]["scan_full"] > 0


def test_driver_refuses_a_pipelined_voxel_map():
    from planetary_lidar_odometry_amd import imls_icp
    with pytest.raises(ValueError, match="never pipelined"):
        imls_icp.LaserOdometry(map_model="voxel", pipelined=True)
    with pytest.raises(ValueError, match="map_model"):
        imls_icp.LaserOdometry(map_model="octree")


def test_parameter_defaults():
    from planetary_lidar_odometry_amd import _abi
    p = _abi.default_voxel_map_params()
    assert (p.voxel_size, p.max_per_voxel, p.max_range) == (0.5, 20, 100.0)
    q = _abi.ImlsVoxelMapParams()                      # the library's own defaults (no context, no GPU)
    _abi.load_library().imls_default_voxel_map_params(q)
    assert (q.voxel_size, q.max_per_voxel, q.max_range) == (p.voxel_size, p.max_per_voxel, p.max_range)
    assert vnp.DEFAULTS == dict(voxel_size=0.5, max_per_voxel=20, max_range=100.0)
