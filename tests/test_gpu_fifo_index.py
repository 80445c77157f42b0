"""The incremental index of the map FIFO (fifo_index.hip fifo_*, api_map.hip fifo_build): each scan pushed
into the FIFO (accumulateTargetCloud, /root/reference/src/laser_odometry.cpp:116-136) is NaN-filtered
and Morton-sorted ONCE under a quantisation frame fixed for the FIFO; a registration compacts the
previous merged order (the evicted scans' entries out) and merges the newest run into it, instead of
re-sorting the concatenation that setTargetPointCloud indexes (imls_icp.cpp:80-103).

The merged order is the stable sort of the concatenation by key, and every record carries its
concatenated filtered index (libnabo's tie order), so the correspondences are exactly a full
build's: against a fresh context's set_target of the same concatenation, every registration has
the same iterations, statuses, per-iteration valid counts and reject counters, and the same pose bit
for bit; against the CPU oracle on the concatenation (oracle/imls_oracle.cpp), iterations, statuses,
valid counts and reject counters exact and the pose within 1e-6.  Covered: a 10-scan FIFO rolling
over, a scan far outside the FIFO's frame (clamped keys → the next build re-frames), and more
pushes between two registrations than there are run ids."""
import numpy as np
import pytest

import oracle_ctypes as oc
from planetary_lidar_odometry_amd import config, imls_icp, synth

pytestmark = pytest.mark.gpu
QUEUE = 10


@pytest.fixture(scope="module")
def scans():
    """15 consecutive VLP-16 scans of one trajectory, each in its own sensor frame (the reference
    pushes the raw filtered scans), plus each one's 2000-point FPS subsample as a small source."""
    sm = synth.vlp16()
    scene = synth.make_scene(4)
    poses = synth.trajectory(20, 2004)
    full = [synth.scan(scene, sm, poses[5 + k], seed=4000 + k) for k in range(15)]
    return full, [synth.fps_subsample(s, 2000, seed=k) for k, s in enumerate(full)]


def _params(iters=6):
    p = config.bench_params(iters)
    p.max_queue_size = QUEUE
    return p


def _same(a, b, key):
    assert (a["iters"], a["status"]) == (b["iters"], b["status"]), key
    for ta, tb in zip(a["trace"], b["trace"]):
        assert ta.n_valid == tb.n_valid and list(ta.reject) == list(tb.reject), key
    assert np.array_equal(a["pose"], b["pose"]), (key, np.abs(a["pose"] - b["pose"]).max())


def _full(p, queue, src):
    with imls_icp.ImlsContext(p) as c:
        c.set_target(np.concatenate(queue))
        c.set_source(src)
        return c.register_frame()


def test_fifo_rolling_equals_full_build_and_oracle(scans):
    full, small = scans
    p = _params()
    queue, checked = [], 0
    with imls_icp.ImlsContext(p) as c:
        for k in range(len(full) - 1):
            n_map = c.map_push(full[k])
            queue.append(full[k])
            if len(queue) > QUEUE:
                queue.pop(0)
            assert n_map == sum(len(q) for q in queue)
            for src in (small[k + 1], full[k + 1]):
                c.set_source(src)
                got = c.register_frame()
                _same(got, _full(p, queue, src), (k, len(src)))
            if k in (3, QUEUE - 1, len(full) - 2):      # growing, full, rolled over
                want = oc.register_frame(synth.soa(small[k + 1]), synth.soa(np.concatenate(queue)), p)
                c.set_source(small[k + 1])
                got = c.register_frame()
                assert (got["iters"], got["status"]) == (want["iters"], want["status"])
                for tg, tw in zip(got["trace"], want["trace"]):
                    assert tg.n_valid == tw.n_valid and list(tg.reject) == list(tw.reject)
                assert np.abs(got["pose"] - want["pose"]).max() < 1e-6
                checked += 1
    assert checked == 3


def test_fifo_reframe_after_far_scan(scans):
    """A scan 500 m outside the frame set by the first scans: its keys clamp at the frame's faces
    (still exact: the tree's boxes come from the points), the next build re-frames every run."""
    full, small = scans
    p = _params()
    far = full[2].copy()
    far["x"] += 500.0
    seq = [full[0], full[1], far, full[3], full[4]]
    queue = []
    with imls_icp.ImlsContext(p) as c:
        for k, sc in enumerate(seq):
            c.map_push(sc, count=False)
            queue.append(sc)
            c.set_source(small[5])
            _same(c.register_frame(), _full(p, queue, small[5]), k)


def test_fifo_many_pushes_between_registrations(scans):
    """40 count-less pushes without a registration (run ids wrap around) then one registration:
    the FIFO's last QUEUE scans, as a full build of them."""
    full, small = scans
    p = _params()
    order = [k % 14 for k in range(40)]
    with imls_icp.ImlsContext(p) as c:
        c.map_push(full[0])
        c.set_source(small[14])
        c.register_frame()                                   # a merged order exists
        for k in order:
            c.map_push(small[k], count=False)
        c.set_source(small[14])
        got = c.register_frame()
    _same(got, _full(p, [small[k] for k in order[-QUEUE:]], small[14]), "wrap")


def test_fifo_tensors_refused(scans):
    full, _ = scans
    p = _params()
    with imls_icp.ImlsContext(p) as c:
        c.map_push(full[0])
        c.map_push(full[1])
        with pytest.raises(Exception):
            c.set_target_tensors(np.zeros((len(full[0]) + len(full[1]), 6), np.float32))
