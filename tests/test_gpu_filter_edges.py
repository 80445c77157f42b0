"""GPU: the NaN filter (csrc/filter.hip) at its edges — the clouds of filter_edge_cases.py: non-finite
rows first, last, on both sides of a 256-row block boundary and of the batched scan's 1,024-block
chunk boundary, one whole block dropped, a NaN normal on a kept row.

Lone path (k_flag_finite → scan → k_compact): set_source returns the input index of every kept row,
which must equal numpy's isfinite mask on xyz exactly.  Batched path (k_filter_count_b →
k_filter_scan_b → k_filter_scatter_b): the same clouds through deferred loads and register_frames, a
posed map push among them; every result must equal — bit for bit — the registration of that frame
alone in a fresh context.  (A cloud without one kept row is no frame: the lone path alone takes the
one-row cloud whose row is non-finite.)"""
import numpy as np
import pytest

import filter_edge_cases as fc
import gpu_mem
import model_restatement as mr
from planetary_lidar_odometry_amd import config, imls_icp, synth

pytestmark = pytest.mark.gpu

POSE = mr.make_pose(0.03, -0.02, 0.05, (0.4, -0.2, 0.1))


@pytest.fixture(scope="module")
def bases():
    """Finite (m, 6) rows of a scan pair: (source, target)."""
    pair = synth.make_pair("vlp16", map_scans=1, start=5)
    rows = [np.ascontiguousarray(synth.soa(c).T) for c in (pair.source, pair.target)]
    return [r[np.isfinite(r).all(axis=1)] for r in rows]


def _params(queue=1):
    p = config.bench_params(3)
    p.max_queue_size = queue
    return p


def _one_finite_row(base):
    a = base[:1].copy()
    a[0, 3:] = np.nan
    return a


def test_lone_filter_keeps_exactly_the_finite_rows(bases):
    src = bases[0]
    clouds = [fc.edge_cloud(src, n) for n in fc.SIZES + (fc.SIZE_SECOND_CHUNK,)] + [_one_finite_row(src)]
    with imls_icp.ImlsContext(_params()) as c, imls_icp.ImlsContext(_params(queue=2)) as f:
        for a in clouds:
            want = fc.kept_rows(a)
            kept = c.set_source(a)
            assert kept.dtype == np.uint32 and np.array_equal(kept, want), (len(a), len(kept), len(want))
            assert c.n_source == len(want)
            # the posed scatter (k_compact_posed: the incremental FIFO's push) keeps the same rows
            f.map_clear()
            assert f.map_push(a, pose=POSE) == len(want), len(a)


def _same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_batched_filter_equals_lone_registrations(bases):
    s, t = bases
    S = {n: fc.edge_cloud(s, n) for n in fc.SIZES[1:]}
    T = {n: fc.edge_cloud(t, n) for n in fc.SIZES[1:] + (fc.SIZE_SECOND_CHUNK,)}
    big = fc.SIZES[-1]
    frames = [                                            # (source, target, pose of the push)
        (S[255], T[big], None),
        (S[big], T[257], None),
        (S[256], T[fc.SIZE_SECOND_CHUNK], POSE),
        (S[257], T[255], None),
        (_one_finite_row(s), T[256], POSE),
        (S[255], _one_finite_row(t), None),
    ]
    p = _params()
    ref = []
    for src, tgt, pose in frames:                         # each frame alone, filters at the call
        with imls_icp.ImlsContext(p) as c:
            assert c.map_push(tgt, pose=pose) == len(fc.kept_rows(tgt))
            assert len(c.set_source(src)) == len(fc.kept_rows(src))
            ref.append(c.register_frame())
    assert all(r["trace"][0].n_valid > 100 for r in ref[:4])      # frames that really register
    dev = [(gpu_mem.DevSoa(src.T), gpu_mem.DevSoa(tgt.T)) for src, tgt, _ in frames]
    ctxs = [imls_icp.ImlsContext(p) for _ in frames]
    try:
        for c, (sd, td), (_, _, pose) in zip(ctxs, dev, frames):
            c.set_defer(True)
            c.map_push_device(td.ptr, td.n, count=False, pose=pose)
            c.set_source_device(sd.ptr, sd.n, count=False)
        poses, iters, status, traces = imls_icp.register_frames(ctxs)
        for k, r in enumerate(ref):
            assert _same_bits(r["pose"], poses[k]), k
            assert (r["iters"], r["status"]) == (iters[k], status[k]), k
            assert len(r["trace"]) == len(traces[k]), k
            assert all(bytes(a) == bytes(b) for a, b in zip(r["trace"], traces[k])), k   # 8-byte fields, no padding
    finally:
        for c in ctxs:
            c.close()
        for a, b in dev:
            a.free()
            b.free()
