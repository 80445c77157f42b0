"""imls_map_push_posed[_device] and imls_map_rebase: a map FIFO kept in one fixed map frame.

The posed push stores a kept point as float(((T0·x + T1·y) + T2·z) + T3) per row (double, in that
order, no contraction) and its normal rotated the same way; the NaN / Inf filter tests the point as
given.  The other side of every check is set_target on the numpy restatement of that arithmetic
(model_restatement.pose_cloud) of the host-concatenated FIFO — the equality
test_gpu_stream.py::test_device_fifo_equals_host_concatenation asserts for the plain push: bit-equal
registrations as the FIFO rolls over — in all three FIFO modes (queue 1: the scan's transformed copy;
queue 3: the incremental index, the transform inside the filter's scatter pass; queue 32: the
concatenation path), host and device forms, with NaN / Inf rows in one scan.  Neighbour lists against
the posed map are exact against oc.knn on the restated map.  Fixtures: 6 VLP-16 scans (~13k points)."""
import numpy as np
import pytest

import gpu_mem
import model_restatement as mr
import oracle_ctypes as oc
from planetary_lidar_odometry_amd import _abi, config, imls_icp, synth

pytestmark = pytest.mark.gpu

# map ← scan poses with yaw, pitch, roll and translation (the last two far from the origin)
POSES = [mr.make_pose(0.0, 0.0, 0.0, (0.0, 0.0, 0.0)),
         mr.make_pose(0.03, -0.01, 0.02, (1.1, -0.2, 0.05)),
         mr.make_pose(-0.4, 0.05, -0.03, (2.3, 0.7, -0.1)),
         mr.make_pose(1.3, -0.08, 0.06, (-3.9, 4.2, 0.3)),
         mr.make_pose(2.9, 0.11, -0.09, (57.0, -31.0, 2.5)),
         mr.make_pose(-2.2, 0.02, 0.15, (-120.5, 88.25, -4.0))]


@pytest.fixture(scope="module")
def scans():
    """(N, 6) float32 scans; scan 2 carries NaN / Inf rows (coordinates and a normal)."""
    sm = synth.vlp16()
    scene = synth.make_scene(2)
    traj = synth.trajectory(11, 2002)
    out = [mr.xyzn(synth.scan(scene, sm, traj[5 + k], seed=5000 + k)) for k in range(6)]
    bad = out[2].copy()
    bad[5, 0] = np.nan
    bad[77, 1] = np.inf
    bad[78, 2] = -np.inf
    bad[4001, :3] = np.nan
    bad[len(bad) - 1, 2] = np.nan
    bad[9, 4] = np.nan                    # a normal: not filtered (the filter tests xyz)
    out[2] = bad
    return out


def _params(queue, iters=4):
    p = config.bench_params(iters)
    p.max_queue_size = queue
    return p


def _same(a, b, key):
    assert (a["iters"], a["status"]) == (b["iters"], b["status"]), key
    for ta, tb in zip(a["trace"], b["trace"]):
        assert ta.n_valid == tb.n_valid and list(ta.reject) == list(tb.reject), key
    assert np.array_equal(a["pose"], b["pose"]), (key, np.abs(a["pose"] - b["pose"]).max())


def _finite(a6):
    return a6[np.isfinite(a6[:, :3]).all(axis=1)]


def _src(full, k):
    """A ~1450-point source in scan k's sensor frame (every 9th point of it)."""
    return np.ascontiguousarray(_finite(full[k])[::9])


class _Pusher:
    """map_push(pose=…) in the host or the device form (device buffers kept alive until close)."""

    def __init__(self, ctx, form):
        self.ctx, self.form, self.bufs = ctx, form, []

    def push(self, a6, pose, count=True):
        if self.form == "host":
            return self.ctx.map_push(a6, count=count, pose=pose)
        d = gpu_mem.DevSoa(np.ascontiguousarray(a6.T))
        self.bufs.append(d)
        return self.ctx.map_push_device(d.ptr, len(a6), count=count, pose=pose)

    def close(self):
        self.ctx.synchronize()
        for d in self.bufs:
            d.free()


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("queue", [1, 3, 32])
def test_posed_fifo_equals_restated_concatenation(scans, queue, form):
    full = scans
    p = _params(queue)
    with imls_icp.ImlsContext(p) as a, imls_icp.ImlsContext(p) as b:
        push = _Pusher(a, form)
        try:
            fifo = []
            for k in range(5):
                T = POSES[k + 1]
                n_map = push.push(full[k], T)
                fifo.append(mr.pose_cloud(full[k], T))
                if len(fifo) > queue:
                    fifo.pop(0)
                want_map = np.concatenate(fifo)
                assert a.map_size() == (len(fifo), len(want_map))
                assert n_map == len(_finite(want_map))
                # the registration's source sits in the newest scan's frame: start it there
                for c in (a, b):
                    c.set_initial_pose(T)
                b.set_target(want_map)
                src = _src(full, k + 1)                     # the next scan, ~1 m on
                a.set_source(src)
                b.set_source(src)
                ra, rb = a.register_frame(), b.register_frame()
                # not vacuous: a tenth of the source has a correspondence at the very first iteration
                assert ra["trace"][0].n_valid > len(src) // 10, (k, ra["trace"][0].n_valid)
                _same(ra, rb, (queue, form, k))
        finally:
            push.close()


@pytest.mark.parametrize("queue", [1, 3, 32])
def test_knn_against_the_posed_map_is_exact(scans, queue):
    full = scans
    p = _params(queue)
    fifo = []
    with imls_icp.ImlsContext(p) as c:
        for k in range(2, 5):                              # scan 2 has the NaN / Inf rows
            c.map_push(full[k], count=False, pose=POSES[k])
            fifo.append(mr.pose_cloud(full[k], POSES[k]))
            if len(fifo) > queue:
                fifo.pop(0)
        q = mr.pose_cloud(_src(full, 5), POSES[4])[:600, :3]
        idx, d2, found = c.knn(q, 20, 3.0, True)
    tgt = mr.soa6(_finite(np.concatenate(fifo)))
    wd2, widx = oc.knn(tgt, np.ascontiguousarray(q.T), 20, 3.0, True)
    assert (found > 0).sum() > 300
    assert np.array_equal(idx, widx) and np.array_equal(d2, wd2)


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("queue", [1, 3, 32])
def test_identity_pose_is_the_plain_push(scans, queue, form):
    full = scans
    p = _params(queue)
    src = _src(full, 4)
    q = src[:500, :3]
    with imls_icp.ImlsContext(p) as a, imls_icp.ImlsContext(p) as b:
        pa, pb = _Pusher(a, form), _Pusher(b, form)
        try:
            for k in (2, 3):
                na = pa.push(full[k], np.eye(4))
                nb = pb.push(full[k], None)
                assert na == nb
            for c in (a, b):
                c.set_source(src)
            _same(a.register_frame(), b.register_frame(), (queue, form))
            ka, kb = a.knn(q, 20, 3.0, True), b.knn(q, 20, 3.0, True)
            assert all(np.array_equal(x, y) for x, y in zip(ka, kb))
        finally:
            pa.close()
            pb.close()


@pytest.mark.parametrize("queue", [1, 3, 32])
def test_rebase_equals_the_restated_double_rounding(scans, queue):
    """map_rebase(B): every stored float re-expressed under B (the second rounding), then a further
    posed push in the new frame still matches."""
    full = scans
    p = _params(queue)
    B = mr.inv_pose(POSES[3])
    src = _src(full, 4)
    with imls_icp.ImlsContext(p) as a, imls_icp.ImlsContext(p) as b:
        fifo = []
        for k in (1, 2, 3):
            a.map_push(full[k], count=False, pose=POSES[k])
            fifo.append(mr.pose_cloud(full[k], POSES[k]))
            if len(fifo) > queue:
                fifo.pop(0)
        a.set_source(src)
        a.set_initial_pose(POSES[3])
        a.register_frame()                                  # the index exists before the rebase
        a.map_rebase(B)
        fifo = [mr.pose_cloud(f, B) for f in fifo]
        a.set_initial_pose(None)                            # scan 3's frame is the map frame now
        b.set_target(np.concatenate(fifo))
        b.set_source(src)
        ra, rb = a.register_frame(), b.register_frame()
        assert ra["trace"][0].n_valid > len(src) // 10
        _same(ra, rb, (queue, "rebased"))
        T = mr.make_pose(0.02, 0.01, -0.01, (0.9, 0.1, 0.0))
        n_map = a.map_push(full[4], pose=T)
        fifo.append(mr.pose_cloud(full[4], T))
        if len(fifo) > queue:
            fifo.pop(0)
        assert n_map == len(_finite(np.concatenate(fifo)))
        b.set_target(np.concatenate(fifo))
        for c in (a, b):
            c.set_initial_pose(T)
            c.set_source(src)
        _same(a.register_frame(), b.register_frame(), (queue, "pushed after the rebase"))


def test_argument_and_state_errors(scans):
    full = scans
    bad = np.eye(4)
    bad[0, 3] = np.nan
    with imls_icp.ImlsContext(_params(3)) as c:
        for call in (lambda: c.map_push(full[0], pose=bad), lambda: c.map_rebase(bad)):
            with pytest.raises(_abi.ImlsError) as e:
                call()
            assert e.value.status == _abi.IMLS_ERR_ARG
        assert c.map_size() == (0, 0)
        c.map_rebase(POSES[1])                              # an empty FIFO: nothing to do
    with imls_icp.ImlsContext(_params(1)) as c:             # a scan indexed in place is the caller's
        d = gpu_mem.DevSoa(np.ascontiguousarray(full[0].T))
        try:
            c.map_push_device(d.ptr, len(full[0]))
            with pytest.raises(_abi.ImlsError) as e:
                c.map_rebase(POSES[1])
            assert e.value.status == _abi.IMLS_ERR_STATE
            c.synchronize()
        finally:
            d.free()
