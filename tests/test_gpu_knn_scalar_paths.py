"""The packet traversal's sparse trip, insertion step and node step at their edges (k_knn_wave).

Packets are forced as in tests/test_gpu_knn_steps.py, and every case is compared with the CPU oracle
under that file's contract: validity masks, reject counters, indices, x and n bit-exact, y within
1e-5 (registrations: iterations, status, per-iteration counts, pose within 1e-6).

(a) 1, 2, 3, 20 and 21 queries within centimetres of one map point: that point's leaf is wanted by
    exactly that many lanes — odd and even numbers of sparse trips, kSparseLanes (20, project_common.h)
    and one past it (the broadcast scan).
(b) maps of 65, 127, 200 and 257 points at leaf 64: a last leaf of 1 and of 63 points, and
    P = 2, 4, 8 leaves, so the node step descends 1, 2 and 3 levels; K = 8 and the map's own points
    jittered by 1 cm as the source, so every leaf is wanted.
(c) a 6-iteration registration from a start off by about half the map's neighbour spacing: prefilled
    lanes meet leaves where some lanes have new candidates and some have none (both branches after
    the sparse trips; the debug build's counts are in profiles/r08_knn_scalar/README.md).
(d) a packet of 32 queries around one map point and 32 around another in a different child of the
    root step: the vote ties.  The projection is checked here; which child the tie chose is checked
    by the per-wave records of the debug build (profiles/r08_knn_scalar/README.md).
"""
import numpy as np
import pytest

import oracle_ctypes as oc
from planetary_lidar_odometry_amd import _abi, config, imls_icp, synth

pytestmark = pytest.mark.gpu
Y_TOL = 1e-5       # tests/test_gpu_parity.py
POSE_TOL = 1e-6    # test_register_frame_matches_golden
MAP_N, SRC_N = 5003, 333
ITERS = 6


def _packets(p):
    c = imls_icp.ImlsContext(p)
    c.set_option("traversal", _abi.IMLS_TRAVERSAL_PACKETS)
    return c


def _check_projection(got, want):
    x, y, n, idx, rej = got
    wx, wy, wn, widx, wrej = want
    assert np.array_equal(rej, wrej), (rej, wrej)
    assert np.array_equal(idx, widx)
    assert np.array_equal(x, wx)
    assert np.array_equal(n, wn)
    if len(widx):
        dy = np.abs(y.astype(np.float64) - wy.astype(np.float64)).max()
        assert dy <= Y_TOL, dy


def _jittered(points, sigma, seed):
    out = points.copy()
    j = np.random.default_rng(seed).normal(0.0, sigma, (out.size, 3)).astype(np.float32)
    out["x"] += j[:, 0]
    out["y"] += j[:, 1]
    out["z"] += j[:, 2]
    return out


def build_clouds():
    """The inputs of this file (the 5003-point map is that of tests/test_gpu_knn_steps.py)."""
    pair = synth.make_pair("vlp16", map_scans=1, start=5)
    rng = np.random.default_rng(7)
    tgt = pair.target[np.sort(rng.choice(pair.target.size, MAP_N, replace=False))]
    # (a) n queries within centimetres of one map point
    lone = {n: _jittered(np.repeat(tgt[MAP_N // 2][None], n), 0.02, 100 + n) for n in (1, 2, 3, 20, 21)}
    # (b) small maps: consecutive points of the map, each queried by its own points moved by 1 cm
    small = {m: tgt[1000:1000 + m].copy() for m in (65, 127, 200, 257)}
    small_src = {m: _jittered(small[m], 0.01, 200 + m) for m in small}
    # (c) the scan off its true pose by about half a neighbour spacing of the map
    off = pair.true_pose @ synth.pose_xyyaw(0.075, -0.05, 0.0015)
    half = synth.fps_subsample(synth.transform_cloud(pair.source, off), SRC_N, seed=2)
    # (d) 32 queries around each of two map points at opposite ends of the map: the two points differ
    # in the top bit of their Morton keys' x, so they lie under different children of the root step
    ca, cb = tgt[int(np.argmin(tgt["x"]))], tgt[int(np.argmax(tgt["x"]))]
    tie = np.concatenate([_jittered(np.repeat(ca[None], 32), 0.02, 301), _jittered(np.repeat(cb[None], 32), 0.02, 302)])
    assert tgt.size == MAP_N and half.size == SRC_N and tie.size == 64
    return dict(tgt=tgt, lone=lone, small=small, small_src=small_src, half=half, tie=tie)


@pytest.fixture(scope="module")
def clouds():
    return build_clouds()


@pytest.fixture(scope="module")
def oracle_half(clouds):
    return oc.register_frame(synth.soa(clouds["half"]), synth.soa(clouds["tgt"]), config.bench_params(ITERS))


@pytest.mark.parametrize("nq", [1, 2, 3, 20, 21])
def test_lone_wanting_lanes(clouds, nq):
    """(a) a leaf wanted by exactly nq lanes."""
    p = config.bench_params(ITERS)
    src = clouds["lone"][nq]
    want = oc.project(synth.soa(src), synth.soa(clouds["tgt"]), np.eye(4), p)
    with _packets(p) as c:
        c.set_target(clouds["tgt"])
        c.set_source(src)
        _check_projection(c.project(np.eye(4)), want)


@pytest.mark.parametrize("m", [65, 127, 200, 257])
def test_partial_leaves_and_shallow_trees(clouds, m):
    """(b) 2, 2, 4 and 5 leaves of 64 (P = 2, 2, 4, 8): the last one holds 1, 63, 8 and 1 points."""
    p = config.bench_params(ITERS)
    p.search_number = 8
    tgt, src = clouds["small"][m], clouds["small_src"][m]
    want = oc.project(synth.soa(src), synth.soa(tgt), np.eye(4), p)
    with _packets(p) as c:
        c.set_option("leaf_size", 64)
        c.set_target(tgt)
        c.set_source(src)
        _check_projection(c.project(np.eye(4)), want)


@pytest.mark.parametrize("leaf", [64, 16])
def test_listed_and_new_points_in_one_visit(clouds, oracle_half, leaf):
    """(c) prefilled lists meet leaves that hold new points for some lanes and none for others."""
    o = oracle_half
    with _packets(config.bench_params(ITERS)) as c:
        c.set_option("leaf_size", leaf)
        c.set_target(clouds["tgt"])
        c.set_source(clouds["half"])
        r = c.register_frame()
    assert r["iters"] == o["iters"] and r["status"] == o["status"], (r["iters"], o["iters"], r["status"], o["status"])
    assert [int(t.n_valid) for t in r["trace"]] == [int(t.n_valid) for t in o["trace"]]
    assert [list(t.reject) for t in r["trace"]] == [list(t.reject) for t in o["trace"]]
    d = np.abs(r["pose"] - o["pose"]).max()
    assert d < POSE_TOL, d


def test_vote_tie(clouds):
    """(d) one 64-query packet, half of it under each of two children of the root step."""
    p = config.bench_params(ITERS)
    want = oc.project(synth.soa(clouds["tie"]), synth.soa(clouds["tgt"]), np.eye(4), p)
    with _packets(p) as c:
        c.set_option("first_packet", 64)
        c.set_target(clouds["tgt"])
        c.set_source(clouds["tie"])
        _check_projection(c.project(np.eye(4)), want)
