"""LaserOdometry(map_model="voxel"): scan-to-model odometry on the voxel map, against the same driver
restated on the CPU oracle's step functions with the numpy map (voxel_map_np.drive_voxel), as
test_gpu_model_odometry.py does for the posed FIFO: iterations and statuses equal, rPose and the
trajectory within that file's tolerances (1e-6 LS, 1e-5 through RANSAC→DRPM), pose-file lines as the
oracle formats them.  The MAP is compared bit for bit: each frame's device map and counters equal the
restatement fed the device's own poses.

Trajectory RMSE against ground truth on this fixture (8 VLP-16 frames), from the CPU restatement and
printed by test_voxel_ls: voxel map 0.00201 m (0.5 m / 20 / 100 m) beside the posed FIFO's 0.00216 m
at queue 3."""
import numpy as np
import pytest

import model_restatement as mr
import oracle_ctypes as oc
import voxel_map_np as vnp
from deskew_cases import front_params, moving_sweep
from planetary_lidar_odometry_amd import _abi, config, imls_icp, producer

pytestmark = pytest.mark.gpu


def _params(ls=True, queue=3):
    p = config.params_from_config(config.load())
    if ls:
        p.solve_method = _abi.IMLS_SOLVE_LS
    p.max_queue_size = queue
    return p


@pytest.fixture(scope="module")
def model():
    """The frames, the ground truth and the oracle side of every configuration, computed once."""
    frames, truth = mr.vlp16_stream(8)
    src = mr.soa6(mr.xyzn(frames[1][1]))
    tgt = mr.soa6(mr.xyzn(frames[0][0]))
    for ls in (True, False):                  # the restated loop is the oracle's, from I
        mr.assert_pinned_to_oracle(src, tgt, _params(ls, 1))
    want = {
        "plain": vnp.drive_voxel(frames, _params()),
        "cv": vnp.drive_voxel(frames, _params(), prior="constant_velocity"),
        "rebase": vnp.drive_voxel(frames, _params(), rebase_distance=2.5),
        "ransac": vnp.drive_voxel(frames[:5], _params(ls=False)),
    }
    return frames, truth, want


def _run(frames, p, tmp_path, name, **kw):
    """The driver over the frames; after every frame its map, counters and map-frame pose."""
    pose_file = tmp_path / f"{name}.txt"
    maps, map_poses = [], []
    with imls_icp.LaserOdometry(p, device=0, pose_file=str(pose_file), map_model="voxel", **kw) as lo:
        assert not lo.pipelined
        for k, (filtered, flat) in enumerate(frames):
            r = lo.process(filtered, flat, timestamp=f"{1317384506.0 + 0.1 * k:f}")
            if k:
                map_poses.append(r["map_pose"])
            maps.append(lo.ctx.voxel_map_download().T.copy())
        return dict(results=list(lo.results), poses=list(lo.poses), lines=pose_file.read_text().splitlines(keepends=True),
                    rebases=lo.rebases, maps=maps, map_poses=map_poses, infos=list(lo.map_infos))


def _check(gpu, want, tol):
    want = want[0]
    results, poses, lines = gpu["results"], gpu["poses"], gpu["lines"]
    assert len(results) == len(want) == len(poses) == len(lines)
    err, prev = [], np.eye(4)
    for (ts, rp, it, st), (ts2, now), (wrp, wit, wst, wnow), line in zip(results, poses, want, lines):
        d = np.abs(rp - wrp).max()
        print(f"{ts}: iters {it}/{wit} status {st}/{wst} |ΔrPose| {d:.3e}")
        assert (it, st) == (wit, wst), (ts, it, st, wit, wst)
        assert d < tol, (ts, d)
        assert np.array_equal(now, oc.chain_pose(prev, rp))
        prev = now
        err.append(np.linalg.norm(now[:3, 3] - wnow[:3, 3]))
        assert line == oc.format_pose(now, ts2)
    rmse = float(np.sqrt(np.mean(np.square(err))))
    print(f"trajectory RMSE vs the restatement {rmse:.3e}")
    assert rmse <= tol, rmse


def _check_maps(frames, p, gpu, **kw):
    """Each frame's device map and counters equal the restatement fed the device's poses, bit for bit."""
    _, maps, infos = vnp.drive_voxel(frames, p, poses=gpu["map_poses"], **kw)
    assert len(maps) == len(gpu["maps"]) == len(frames) == len(gpu["infos"])
    for k, (got, want) in enumerate(zip(gpu["maps"], maps)):
        assert got.shape == want.shape, (k, got.shape, want.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
        assert gpu["infos"][k] == infos[k], (k, gpu["infos"][k], infos[k])
    print("map sizes", [len(m) for m in maps])


def test_voxel_ls(model, tmp_path):
    frames, truth, want = model
    gpu = _run(frames, _params(), tmp_path, "voxel")
    assert gpu["rebases"] == 0
    _check(gpu, want["plain"], 1e-6)
    _check_maps(frames, _params(), gpu)
    rmse = mr.rmse_to([now for _, now in gpu["poses"]], truth)
    oracle = mr.rmse_to([w[3] for w in want["plain"][0]], truth)
    print(f"trajectory RMSE vs ground truth: voxel map {rmse:.5f} m (the restatement's {oracle:.5f} m)")
    assert abs(rmse - oracle) <= 1e-6
    assert max(len(m) for m in gpu["maps"]) > 80000          # the map grows over the stream: ~90k rows


def test_voxel_ignores_max_queue_size(model, tmp_path):
    frames, _, want = model
    gpu = _run(frames[:4], _params(queue=1), tmp_path, "q1")
    _check(gpu, (want["plain"][0][:3],), 1e-6)
    _check_maps(frames[:4], _params(queue=1), gpu)


def test_voxel_constant_velocity(model, tmp_path):
    frames, _, want = model
    gpu = _run(frames, _params(), tmp_path, "cv", motion_prior="constant_velocity")
    _check(gpu, want["cv"], 1e-6)
    _check_maps(frames, _params(), gpu, prior="constant_velocity")


def test_voxel_with_rebases(model, tmp_path):
    """rebase_distance 2.5 m on a 1 m-per-frame trajectory: the map is re-expressed in the newest scan's
    frame twice within the 8 frames, and the update after each rebase trims the re-partitioned voxels."""
    frames, _, want = model
    gpu = _run(frames, _params(), tmp_path, "rebase", rebase_distance=2.5)
    assert gpu["rebases"] == 2
    _check(gpu, want["rebase"], 1e-6)
    _check_maps(frames, _params(), gpu, rebase_distance=2.5)
    assert sum(i["map_trimmed"] for i in gpu["infos"]) > 0


def test_voxel_ransac_drpm(model, tmp_path):
    frames, _, want = model
    gpu = _run(frames[:5], _params(ls=False), tmp_path, "ransac")
    _check(gpu, want["ransac"], 1e-5)
    _check_maps(frames[:5], _params(ls=False), gpu)


def test_standing_still_saturates(model):
    """The same scan over and over: the FIFO would hold max_queue_size copies; the voxel map stops
    growing once every voxel is full, and equals the restatement at every push."""
    frames, _, _ = model
    filtered, flat = frames[0]
    params = dict(voxel_size=0.25, max_per_voxel=4)
    # at one pose: Σ_v min(cap, k·c_v) rows after k pushes, constant once every voxel is full
    scan = mr.xyzn(filtered)
    _, counts = np.unique(vnp.keys_of(vnp.voxel_index(scan, 0.25)), return_counts=True)
    vm, sizes = vnp.VoxelMap(**params), []
    with imls_icp.ImlsContext(_params()) as c:
        c.set_voxel_map_params(**params)
        for k in range(1, 8):
            sizes.append(c.voxel_map_update(filtered))
            vm.update(filtered)
            assert sizes[-1] == len(vm.rows) == int(np.minimum(4, k * counts).sum())
        assert np.array_equal(c.voxel_map_download().T.view(np.uint32), vm.rows.view(np.uint32))
        assert c.voxel_map_info() == vm.info and vm.info["scan_inserted"] == 0
    print("standing still at one pose, map sizes", sizes)
    assert sizes[0] < sizes[1] < sizes[2] and sizes[-1] == sizes[-2] == sizes[-3] == 4 * len(counts)
    # through the driver, which registers every scan against the map and pushes it at the pose it found
    # (I to within the registration's noise): the map equals the restatement at the device's poses
    vm, sizes = vnp.VoxelMap(**params), []
    with imls_icp.LaserOdometry(_params(), map_model="voxel", voxel_map=_abi.ImlsVoxelMapParams(0.25, 4, 100.0)) as lo:
        for k in range(5):
            lo.process(filtered, flat, str(k))
            vm.update(filtered, lo.anchor_pose)
            got = lo.ctx.voxel_map_download().T
            assert np.array_equal(got.view(np.uint32), vm.rows.view(np.uint32)), k
            assert lo.map_infos[-1] == vm.info
            sizes.append(got.shape[0])
            # bounded by the occupied volume, not by the number of pushes
            assert sizes[-1] == lo.map_infos[-1]["points"] <= 4 * lo.map_infos[-1]["voxels"]
    print("standing still through the driver, map sizes", sizes)


def test_process_sweep_equals_process_on_the_downloaded_clouds():
    sweeps = [moving_sweep(k)[0] for k in range(4)]
    p, fp = _params(), front_params()
    vmp = _abi.ImlsVoxelMapParams(0.5, 10, 80.0)
    with imls_icp.LaserOdometry(p, map_model="voxel", voxel_map=vmp,
                                producer=producer.ScanRegistration(shuffle_seed=4, rand_seed=2)) as a, \
            imls_icp.LaserOdometry(p, map_model="voxel", voxel_map=vmp) as b:
        host = producer.ScanRegistration(shuffle_seed=4, rand_seed=2)
        try:
            for k, raw in enumerate(sweeps):
                ra = a.process_sweep(raw, str(k), fp)
                rb = b.process(*host.process_raw(raw, fp), str(k))
                assert (ra is None) == (rb is None) == (k == 0)
                assert a.ctx.voxel_map_download().tobytes() == b.ctx.voxel_map_download().tobytes()
        finally:
            host.close()
            a.producer.close()
        assert len(a.poses) == 3 and all(r[2] > 0 for r in a.results)
        for (ta, pa), (tb, pb) in zip(a.poses, b.poses):
            assert ta == tb and pa.tobytes() == pb.tobytes()
        assert a.map_infos == b.map_infos and a.map_infos[-1]["points"] > a.map_infos[0]["points"]
