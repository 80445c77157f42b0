"""GPU: the voxel map (imls_voxel_map_*) against its numpy restatement (voxel_map_np.py), bit for bit —
the stored rows in their order and every counter, after every update of every case of
voxel_map_cases.py (whose premises test_voxel_map_model.py proves), through the host and the device
form; argument and state errors; and the cross-checks against the machinery the map feeds: a
registration against the map equals one against set_target(download()), kNN distances equal those of
a posed FIFO of the same scans, and contexts that never use the map are untouched by one that does."""
import numpy as np
import pytest

import gpu_mem
import model_restatement as mr
import voxel_map_cases as vc
import voxel_map_np as vnp
from planetary_lidar_odometry_amd import _abi, config, imls_icp

pytestmark = pytest.mark.gpu

CASES = vc.all_cases()
INF = float("inf")


@pytest.fixture(scope="module")
def ctx():
    with imls_icp.ImlsContext(config.bench_params(3)) as c:
        yield c


def _update(c, form, scan, pose):
    if form == "host":
        return c.voxel_map_update(scan, pose)
    if len(scan) == 0:
        return c.voxel_map_update_device(0, 0, pose)
    d = gpu_mem.DevSoa(np.ascontiguousarray(scan.T))
    try:
        return c.voxel_map_update_device(d.ptr, len(scan), pose)      # the call waits: the scan has been read
    finally:
        d.free()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_map(c, vm, key):
    got = c.voxel_map_download()
    assert got.shape == (6, len(vm.rows)), (key, got.shape, len(vm.rows))
    assert np.array_equal(_bits(got.T), _bits(vm.rows)), key
    assert c.voxel_map_info() == vm.info, (key, c.voxel_map_info(), vm.info)
    assert c.map_size() == ((1, len(vm.rows)) if len(vm.rows) else (0, 0))


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_map_order_and_counters_equal_the_restatement(ctx, case, form):
    name, params, steps = case
    ctx.map_clear()
    ctx.set_voxel_map_params(**params)
    vm = vnp.VoxelMap(**params)
    for k, step in enumerate(steps):
        if step[0] == "rebase":
            ctx.map_rebase(step[1])
            vm.rebase(step[1])
            got = ctx.voxel_map_download()
            assert np.array_equal(_bits(got.T), _bits(vm.rows)), (name, k, "rebase")
            continue
        n_map = _update(ctx, form, step[1], step[2])
        vm.update(step[1], step[2])
        assert n_map == len(vm.rows) == ctx.n_target, (name, k)
        _assert_map(ctx, vm, (name, form, k))


def test_first_info_is_zero_and_defaults():
    with imls_icp.ImlsContext(config.bench_params(3)) as c:
        assert c.voxel_map_info() == {k: 0 for k in vnp.INFO_KEYS}
        assert c.voxel_map_download().shape == (6, 0)
        p = _abi.ImlsVoxelMapParams()
        c.lib.imls_default_voxel_map_params(p)
        assert (p.voxel_size, p.max_per_voxel, p.max_range) == (0.5, 20, 100.0)
        # the defaults are in force without a set_params call
        scan = vc.cloud(5000, 1, 120.0)
        c.voxel_map_update(scan)
        vm = vnp.VoxelMap()
        vm.update(scan)
        assert vm.info["scan_out_of_range"] > 0
        _assert_map(c, vm, "defaults")


# ---- argument and state errors ------------------------------------------------------------------
def _raises(status, call):
    with pytest.raises(_abi.ImlsError) as e:
        call()
    assert e.value.status == status, e.value


def test_argument_errors():
    scan = vc.cloud(100, 2)
    with imls_icp.ImlsContext(config.bench_params(3)) as c:
        for bad in (dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(voxel_size=float("nan")), dict(voxel_size=INF),
                    dict(max_per_voxel=0), dict(max_per_voxel=-3), dict(max_range=0.0), dict(max_range=-2.0),
                    dict(max_range=float("nan")), dict(max_range=-INF)):
            _raises(_abi.IMLS_ERR_ARG, lambda: c.set_voxel_map_params(**bad))
        c.set_voxel_map_params(max_range=INF, max_per_voxel=1, voxel_size=0.01)
        d = gpu_mem.DevSoa(np.ascontiguousarray(scan.T))
        try:
            for k in range(12):                              # every entry of rows 0-2, then one of the last row
                pose = np.eye(4)
                pose.reshape(16)[k] = np.nan if k % 2 else np.inf
                _raises(_abi.IMLS_ERR_ARG, lambda: c.voxel_map_update(scan, pose))
                _raises(_abi.IMLS_ERR_ARG, lambda: c.voxel_map_update_device(d.ptr, len(scan), pose))
            pose = np.eye(4)
            pose[3, 1] = np.nan
            _raises(_abi.IMLS_ERR_ARG, lambda: c.voxel_map_update(scan, pose))
        finally:
            d.free()
        assert c.voxel_map_download().shape == (6, 0) and c.voxel_map_info()["points"] == 0


def test_state_errors_and_map_kinds():
    scan, other = vc.cloud(3000, 3, 10.0), vc.cloud(2000, 4, 10.0)
    src = np.ascontiguousarray(scan[::3])
    p = config.bench_params(3)
    p.max_queue_size = 3
    with imls_icp.ImlsContext(p) as c:
        c.voxel_map_update(scan)
        # a FIFO push on a context holding a voxel map, in every form
        _raises(_abi.IMLS_ERR_STATE, lambda: c.map_push(other))
        _raises(_abi.IMLS_ERR_STATE, lambda: c.map_push(other, pose=vc.POSE_A))
        before = c.voxel_map_download()
        # an update while a registration is pending
        c.set_source(src)
        c.register_frame_async()
        _raises(_abi.IMLS_ERR_STATE, lambda: c.voxel_map_update(other))
        _raises(_abi.IMLS_ERR_STATE, lambda: c.map_rebase(vc.POSE_A))
        c.register_frame_result()
        assert np.array_equal(_bits(c.voxel_map_download()), _bits(before))
        # set_target replaces the index without touching the map
        c.set_target(other)
        assert np.array_equal(_bits(c.voxel_map_download()), _bits(before))
        c.voxel_map_update(other, vc.POSE_A)
        vm = vnp.VoxelMap()
        vm.update(scan)
        vm.update(other, vc.POSE_A)
        _assert_map(c, vm, "after set_target")
        # map_clear empties whichever map is held; then the FIFO may be used, and bars the voxel map
        c.map_clear()
        assert c.map_size() == (0, 0) and c.voxel_map_download().shape == (6, 0)
        c.map_push(other)
        assert c.map_size() == (1, len(other))
        _raises(_abi.IMLS_ERR_STATE, lambda: c.voxel_map_update(scan))
        c.map_clear()
        c.map_push(np.zeros((0, 6), np.float32))             # a FIFO of empty scans holds no points: no bar
        assert c.voxel_map_update(scan) == len(vnp.update(np.zeros((0, 6), np.float32), scan)[0])


def test_an_empty_map_is_no_target(stream):
    frames, _ = stream
    scan = frames[0][0]
    with imls_icp.ImlsContext(config.bench_params(3)) as c:
        c.set_voxel_map_params(max_range=200.0)
        n0 = c.voxel_map_update(scan)
        c.set_source(frames[1][1])
        assert c.register_frame()["iters"] > 0
        assert c.voxel_map_update(np.zeros((0, 6), np.float32), mr.make_pose(t=(5000.0, 0.0, 0.0))) == 0
        assert c.voxel_map_info()["map_out_of_range"] == n0 > 0
        _raises(_abi.IMLS_ERR_STATE, lambda: c.register_frame())
        c.map_rebase(vc.POSE_A)                              # an empty map: nothing to do
        assert c.voxel_map_update(scan) > 0
        assert c.register_frame()["iters"] > 0


# ---- cross-checks against existing machinery ------------------------------------------------------
@pytest.fixture(scope="module")
def stream():
    frames, truth = mr.vlp16_stream(4)
    return [(mr.xyzn(f), mr.xyzn(s)) for f, s in frames], truth


def _same(a, b, key):
    assert (a["iters"], a["status"]) == (b["iters"], b["status"]), key
    assert len(a["trace"]) == len(b["trace"])
    for ta, tb in zip(a["trace"], b["trace"]):
        assert ta.n_valid == tb.n_valid and list(ta.reject) == list(tb.reject), key
        assert list(ta.pose) == list(tb.pose), key
    assert np.array_equal(a["pose"], b["pose"]), (key, np.abs(a["pose"] - b["pose"]).max())


@pytest.mark.parametrize("ls", [True, False], ids=["ls", "ransac_drpm"])
def test_registration_against_the_map_equals_set_target_of_its_rows(stream, ls):
    frames, truth = stream
    p = config.params_from_config(config.load())
    if ls:
        p.solve_method = _abi.IMLS_SOLVE_LS
    with imls_icp.ImlsContext(p) as a, imls_icp.ImlsContext(p) as b:
        for k in range(3):
            a.voxel_map_update(frames[k][0], truth[k])
        rows = a.voxel_map_download()
        assert rows.shape[1] > len(frames[0][0])
        assert b.set_target(np.ascontiguousarray(rows.T)) == rows.shape[1]
        for c in (a, b):
            c.set_initial_pose(truth[2])
            c.set_source(frames[3][1])
        ra, rb = a.register_frame(), b.register_frame()
        assert ra["trace"][0].n_valid > len(frames[3][1]) // 10
        _same(ra, rb, ls)
        assert np.array_equal(a.rng_state(), b.rng_state())


def test_knn_distances_equal_a_posed_fifo_of_the_same_scans(stream):
    frames, truth = stream
    p = config.bench_params(3)
    p.max_queue_size = 3
    q = mr.pose_cloud(frames[3][1], truth[3])[:800, :3]
    with imls_icp.ImlsContext(p) as a, imls_icp.ImlsContext(p) as b:
        a.set_voxel_map_params(max_per_voxel=10 ** 6, max_range=INF)
        for k in range(3):
            na = a.voxel_map_update(frames[k][0], truth[k])
            nb = b.map_push(frames[k][0], pose=truth[k])
            assert na == nb
        ia, da, fa = a.knn(q, 20, 3.0, True)
        ib, db, fb = b.knn(q, 20, 3.0, True)
    assert (fa > 0).sum() > 400
    assert np.array_equal(da, db) and np.array_equal(fa, fb)
    assert not np.array_equal(ia, ib)                        # another order: the indices differ


def test_contexts_that_never_use_the_map_are_untouched(stream):
    frames, truth = stream
    p = config.params_from_config(config.load())            # RANSAC → DRPM: the rand() stream is part of the state

    def plain():
        with imls_icp.ImlsContext(p) as c:
            c.set_target(frames[0][0])
            c.set_source(frames[1][1])
            r = c.register_frame()
            return r, c.rng_state()

    before, state_before = plain()
    with imls_icp.ImlsContext(p) as v:
        v.set_voxel_map_params(max_per_voxel=3)
        for k in range(2):
            v.voxel_map_update(frames[k][0], truth[k])
        v.map_rebase(mr.inv_pose(truth[1]))
        v.set_source(frames[2][1])
        v.register_frame()
        after, state_after = plain()                         # while the map's context is alive
    _same(before, after, "plain")
    assert np.array_equal(state_before, state_after)
