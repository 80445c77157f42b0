"""The packet traversal's leaf and node steps (k_knn_wave / k_knn_wave_b) on small frames.

Small frames take the wave-per-query kernels by default, so every context here forces packets
(IMLS_OPT_TRAVERSAL = IMLS_TRAVERSAL_PACKETS).  Each case is compared with the CPU oracle under the
contract of tests/test_gpu_parity.py: validity masks, reject counters, indices, x and n bit-exact,
y within 1e-5; every query is compared.

Sizes: a map of 5003 points and sources of 333 / 301 queries — neither a multiple of 64, so the last
leaf and the last packet are partial — and a few ICP iterations: each case runs in about a second.

Which leaf path runs follows from the queries' layout (kSparseLanes = 20 in project_common.h): queries
spread over the whole map leave ≤ 20 lanes of a packet wanting any one leaf (the sparse scan);
a whole packet of queries within a few centimetres of one map point all want that point's leaf
(the broadcast scan).  The debug-trace build's counts of sparse and broadcast leaf visits for these
inputs at each leaf size are recorded in profiles/r07_knn_issue/README.md (tools/leaf_visit_trace.py).
"""
import numpy as np
import pytest

import oracle_ctypes as oc
from planetary_lidar_odometry_amd import _abi, config, imls_icp, synth

pytestmark = pytest.mark.gpu
Y_TOL = 1e-5       # tests/test_gpu_parity.py
POSE_TOL = 1e-6    # test_register_frame_matches_golden
MAP_N, SRC_N, SRC2_N = 5003, 333, 301
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


def build_clouds():
    """The inputs of this file (also counted by tools/leaf_visit_trace.py, which imports this)."""
    pair = synth.make_pair("vlp16", map_scans=1, start=5)
    rng = np.random.default_rng(7)
    tgt = pair.target[np.sort(rng.choice(pair.target.size, MAP_N, replace=False))]
    # spread: a farthest-point subsample of the scan, moved onto the map by the true motion
    moved = synth.transform_cloud(pair.source, pair.true_pose)
    spread = synth.fps_subsample(moved, SRC_N, seed=1)
    # clustered: every query within centimetres of one map point (inside one leaf's extent)
    c = tgt[MAP_N // 2]
    clustered = np.repeat(c[None], SRC_N)
    j = rng.normal(0.0, 0.02, (SRC_N, 3)).astype(np.float32)
    clustered["x"] += j[:, 0]
    clustered["y"] += j[:, 1]
    clustered["z"] += j[:, 2]
    # registration: the scan off its true pose by about one neighbour spacing of the map
    off = pair.true_pose @ synth.pose_xyyaw(0.15, -0.1, 0.003)
    reg = synth.fps_subsample(synth.transform_cloud(pair.source, off), SRC_N, seed=2)
    reg2 = synth.fps_subsample(synth.transform_cloud(pair.source, off), SRC2_N, seed=3)
    assert tgt.size == MAP_N and spread.size == SRC_N and reg.size == SRC_N and reg2.size == SRC2_N
    return dict(tgt=tgt, spread=spread, clustered=clustered, reg=reg, reg2=reg2)


@pytest.fixture(scope="module")
def clouds():
    return build_clouds()


@pytest.fixture(scope="module")
def oracle_proj(clouds):
    p = config.bench_params(ITERS)
    return {k: oc.project(synth.soa(clouds[k]), synth.soa(clouds["tgt"]), np.eye(4), p) for k in ("spread", "clustered")}


@pytest.fixture(scope="module")
def oracle_reg(clouds):
    p = config.bench_params(ITERS)
    return {k: oc.register_frame(synth.soa(clouds[k]), synth.soa(clouds["tgt"]), p) for k in ("reg", "reg2")}


def _check_frame(r, o):
    assert r["iters"] == o["iters"] and r["status"] == o["status"], (r["iters"], o["iters"], r["status"], o["status"])
    assert [int(t.n_valid) for t in r["trace"]] == [int(t.n_valid) for t in o["trace"]]
    assert [list(t.reject) for t in r["trace"]] == [list(t.reject) for t in o["trace"]]
    d = np.abs(r["pose"] - o["pose"]).max()
    assert d < POSE_TOL, d


@pytest.mark.parametrize("queries", ["spread", "clustered"])
@pytest.mark.parametrize("leaf", [64, 16, 4])
def test_leaf_sizes(clouds, oracle_proj, leaf, queries):
    """Leaf sizes 64, 16 and 4 (cnt < 64 in both leaf scans) with spread queries (sparse scan) and a
    packet of queries inside one leaf (broadcast scan)."""
    with _packets(config.bench_params(ITERS)) as c:
        c.set_option("leaf_size", leaf)
        c.set_target(clouds["tgt"])
        c.set_source(clouds[queries])
        _check_projection(c.project(np.eye(4)), oracle_proj[queries])


def test_multi_iteration_registration(clouds, oracle_reg):
    """≥ 5 ICP iterations from a pose off by about one neighbour spacing: the prefilled lists meet
    leaves holding both listed and new points.  List reuse and temporal seeding on and off give the
    same frame, the oracle's."""
    o = oracle_reg["reg"]
    assert o["iters"] >= 5
    poses = []
    for reuse in (1, 0):
        for seed in (1, 0):
            with _packets(config.bench_params(ITERS)) as c:
                c.set_options(list_reuse=reuse, temporal_seed=seed)
                c.set_target(clouds["tgt"])
                c.set_source(clouds["reg"])
                r = c.register_frame()
            _check_frame(r, o)
            poses.append(r["pose"])
    for q in poses[1:]:
        assert np.array_equal(q, poses[0])


@pytest.mark.parametrize("K", [8, 20, 32])
def test_ties_and_duplicates(clouds, K):
    """Exact duplicate map points and queries that coincide with map points: many equal keys, tying
    after the slot-id truncation.  K = 8, 20, 32 run the KL = 12, 22 and 36 instantiations."""
    NDUP = 300
    tgt = np.concatenate([clouds["tgt"], clouds["tgt"][:NDUP]])
    src = tgt[:SRC_N].copy()                  # on the duplicated points (and 33 single ones)
    p = config.bench_params(ITERS)
    p.search_number = K
    # the case is what it claims: most queries hold both copies of some point (two equal keys) among
    # their K nearest, by the oracle's own neighbour search
    _, nn = oc.knn(synth.soa(tgt), synth.soa(src)[:3], K, float(p.r), 1)
    both = sum(1 for row in nn if any(i < NDUP and i + MAP_N in row for i in row))
    assert both >= NDUP * 9 // 10, both
    want = oc.project(synth.soa(src), synth.soa(tgt), np.eye(4), p)
    with _packets(p) as c:
        c.set_target(tgt)
        c.set_source(src)
        _check_projection(c.project(np.eye(4)), want)


_RUNG_ORACLE = {}


def _rung_oracle(clouds, K, src):
    """The oracle's projection of clouds[src] at the identity with search_number K, once per (K, src)."""
    if (K, src) not in _RUNG_ORACLE:
        p = config.bench_params(ITERS)
        p.search_number = K
        _RUNG_ORACLE[K, src] = oc.project(synth.soa(clouds[src]), synth.soa(clouds["tgt"]), np.eye(4), p)
    return _RUNG_ORACLE[K, src]


@pytest.mark.parametrize("path", ["packets", "wave_per_query", "fused", "lane"])
@pytest.mark.parametrize("K", [8, 16, 20, 32])
def test_list_size_rungs_alone(clouds, K, path):
    """Every rung of the K → (list length, heap capacity) table (K ≤ 8, ≤ 16, ≤ 20, > 20) on every
    launch path of a frame alone: packets + k_finish, one wave per query + k_finish (the map itself as
    the source: 5003 queries, above the fused kernel's 4096), the fused kernel (333 queries), and
    every query through the exact per-lane kernel.  What this pins is the launch plumbing and the list
    block's addresses on each path for each instantiation; it does not pin the table's values (a list
    too short only sends more queries to the exact fallback, which still answers right)."""
    mode = {"packets": _abi.IMLS_TRAVERSAL_PACKETS, "wave_per_query": _abi.IMLS_TRAVERSAL_WAVE_PER_QUERY,
            "fused": _abi.IMLS_TRAVERSAL_WAVE_PER_QUERY, "lane": _abi.IMLS_TRAVERSAL_LANE}[path]
    src = "tgt" if path == "wave_per_query" else "spread"
    p = config.bench_params(ITERS)
    p.search_number = K
    with imls_icp.ImlsContext(p) as c:
        c.set_option("traversal", mode)
        c.set_target(clouds["tgt"])
        c.set_source(clouds[src])
        _check_projection(c.project(np.eye(4)), _rung_oracle(clouds, K, src))


@pytest.mark.parametrize("trav", ["packets", "wave_per_query"])
@pytest.mark.parametrize("K", [8, 16, 20, 32])
def test_list_size_rungs_batched(clouds, K, trav):
    """The same rungs through the batched kernels: two frames in one call, each the oracle's frame."""
    p = config.bench_params(ITERS)
    p.search_number = K
    if K not in _RUNG_ORACLE:   # the oracle's two registrations, once per K
        _RUNG_ORACLE[K] = [oc.register_frame(synth.soa(clouds[k]), synth.soa(clouds["tgt"]), p) for k in ("reg", "reg2")]
    want = _RUNG_ORACLE[K]
    ctxs = [imls_icp.ImlsContext(p) for _ in range(2)]
    try:
        for c, k in zip(ctxs, ("reg", "reg2")):
            c.set_option("traversal", {"packets": _abi.IMLS_TRAVERSAL_PACKETS,
                                       "wave_per_query": _abi.IMLS_TRAVERSAL_WAVE_PER_QUERY}[trav])
            c.set_target(clouds["tgt"])
            c.set_source(clouds[k])
        poses, iters, status, traces = imls_icp.register_frames(ctxs)
    finally:
        for c in ctxs:
            c.close()
    for f, o in enumerate(want):
        _check_frame(dict(pose=poses[f], iters=iters[f], status=status[f], trace=traces[f]), o)


@pytest.mark.parametrize("packet", [16, 32])
def test_first_packet_sizes(clouds, oracle_reg, packet):
    """Packets of 16 and 32 queries per wave in every iteration."""
    with _packets(config.bench_params(ITERS)) as c:
        c.set_options(first_packet=packet, first_packet_iters=ITERS)
        c.set_target(clouds["tgt"])
        c.set_source(clouds["reg"])
        _check_frame(c.register_frame(), oracle_reg["reg"])


def test_batched_entry_point(clouds, oracle_reg):
    """Two frames in one call (k_knn_wave_b): each bit-equal to the frame registered alone."""
    p = config.bench_params(ITERS)
    alone = []
    for k in ("reg", "reg2"):
        with _packets(p) as c:
            c.set_target(clouds["tgt"])
            c.set_source(clouds[k])
            alone.append(c.register_frame())
        _check_frame(alone[-1], oracle_reg[k])
    ctxs = [_packets(p) for _ in range(2)]
    try:
        for c, k in zip(ctxs, ("reg", "reg2")):
            c.set_target(clouds["tgt"])
            c.set_source(clouds[k])
        poses, iters, status, traces = imls_icp.register_frames(ctxs)
    finally:
        for c in ctxs:
            c.close()
    for f, a in enumerate(alone):
        assert iters[f] == a["iters"] and status[f] == a["status"]
        assert np.array_equal(poses[f], a["pose"])
        assert len(traces[f]) == len(a["trace"])
        for t, u in zip(traces[f], a["trace"]):
            assert list(t.delta) == list(u.delta) and list(t.pose) == list(u.pose)
            assert list(t.reject) == list(u.reject) and t.n_valid == u.n_valid and t.n_kept == u.n_kept
