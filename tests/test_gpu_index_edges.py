"""Every index builder at its edges, through the public exact kNN (ImlsContext.knn) against the brute
force of index_edge_cases.py — test_index_edge_cases.py proves that each case reaches its edge.

For every index state reached, exactly (np.array_equal on idx and d², found = filled slots):
  (a) n_map / set_target's count / index_stats' points = the number of finite rows;
  (b) the census: every map point asks k = 1, self-match allowed, r = +inf and must get d² = 0 and the
      lowest index among its exact duplicates — complete by construction: an index that lost or
      replaced any single entry fails it, which kNN probes alone cannot promise;
  (c) 500 probes (half jittered map points, half uniform in and just outside the bbox), k = 20 within
      r = 3.0 without self-match and k = 32 within +inf with self-match, as the brute force answers;
  (d) where the map came from the FIFO, a fresh context's set_target of the concatenation gives the
      same rows.
Contexts are module-level and references are cached per map (shared by the leaf sizes and traversals)."""
import pathlib

import numpy as np
import pytest

import gpu_mem
import index_edge_cases as ec
import model_restatement as mr
import oracle_ctypes as oc
from planetary_lidar_odometry_amd import _abi, config, imls_icp, synth
from test_gpu_fifo_index import _same

pytestmark = pytest.mark.gpu
TRAVERSALS = {"auto": _abi.IMLS_TRAVERSAL_AUTO, "packets": _abi.IMLS_TRAVERSAL_PACKETS, "lane": _abi.IMLS_TRAVERSAL_LANE}
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
Y_TOL = 1e-5                 # the projection's parity contract

_CTX, _REF = {}, {}


def params(queue=1, iters=6):
    p = config.bench_params(iters)
    p.max_queue_size = queue
    return p


def ctx_for(leaf, queue=1, tag=""):
    key = (leaf, queue, tag)
    if key not in _CTX:
        c = imls_icp.ImlsContext(params(queue))
        c.set_option("leaf_size", leaf)
        _CTX[key] = c
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()
    _REF.clear()


def reference(key, P, nprobe=500, census_sample=None):
    """(census queries, census rows, probes, their rows per PROBE_CONFIGS) of map P, computed once."""
    if key not in _REF:
        cidx, cd2 = ec.census(P)
        sel = np.arange(len(P))
        if census_sample is not None and census_sample < len(P):
            sel = np.sort(np.random.default_rng(9).choice(len(P), census_sample, replace=False))
        q = ec.probes(P, nprobe)
        _REF[key] = (P.tobytes(), np.ascontiguousarray(P[sel]), (cidx[sel], cd2[sel]), q, ec.brute_knn_multi(P, q, ec.PROBE_CONFIGS))
    assert _REF[key][0] == P.tobytes(), key                 # one key, one map
    return _REF[key][1:]


def exact(got, want, label):
    idx, d2, found = got
    widx, wd2 = want
    assert idx.dtype == np.int32 and d2.dtype == np.float64 and found.dtype == np.int32
    bad = np.nonzero((idx != widx).any(axis=1) | (d2 != wd2).any(axis=1))[0]
    assert bad.size == 0, (label, len(bad), bad[:5], idx[bad[:2]], widx[bad[:2]], d2[bad[:2]], wd2[bad[:2]])
    assert np.array_equal(idx, widx) and np.array_equal(d2, wd2), label
    assert np.array_equal(found, (idx >= 0).sum(axis=1)), label


def check_state(c, P, key, count=None, solo=None, raw=None, nprobe=500, census_sample=None):
    """(a) – (c) on context c holding map P; (d) against `solo` loaded with the raw concatenation."""
    cq, census, q, rows = reference(key, P, nprobe, census_sample)
    if count is not None:
        assert count == len(P), key
    assert c.index_stats()["points"] == len(P), key
    exact(c.knn(cq, 1, np.inf, True), census, (key, "census"))
    for (k, r, self_ok), want in zip(ec.PROBE_CONFIGS, rows):
        exact(c.knn(q, k, r, self_ok), want, (key, k, r))
    if solo is not None:
        assert solo.set_target(raw) == len(P), key
        exact(solo.knn(cq, 1, np.inf, True), census, (key, "solo census"))
        for (k, r, self_ok), want in zip(ec.PROBE_CONFIGS, rows):
            exact(solo.knn(q, k, r, self_ok), want, (key, "solo", k, r))


def check_shape(c, M, leaf):
    L, P, levels, _ = ec.tree_shape(M, leaf)
    st = c.index_stats()
    assert (st["points"], st["leaves"], st["leaf_slots"], st["levels"], st["bucket"]) == (M, L, P, levels, leaf)


def no_target(c):
    with pytest.raises(_abi.ImlsError) as e:
        c.knn(np.zeros((3, 3), np.float32), 1)
    assert e.value.status == _abi.IMLS_ERR_STATE


# ---- full build ----------------------------------------------------------------------------------------
def _full_build(c, P, key, leaf, traversals, **kw):
    try:
        for trav in traversals:
            c.set_option("traversal", TRAVERSALS[trav])
            n = c.set_target(ec.rows6(P))
            check_shape(c, len(P), leaf)
            check_state(c, P, key, n, **kw)
    finally:
        c.set_option("traversal", _abi.IMLS_TRAVERSAL_AUTO)


@pytest.mark.parametrize("leaf", ec.LEAVES)
@pytest.mark.parametrize("name", list(ec.GEOMETRY))
def test_full_build_degenerate_geometry(name, leaf):
    """index.hip morton_perm (k_bbox_final's ext floor, k_morton's clamp), k_gather, k_leaf_boxes,
    k_subtree; more than 32 points on one position need every leaf at the k-th distance visited."""
    _full_build(ctx_for(leaf), ec.geometry(name), name, leaf, ("auto", "packets", "lane"))


@pytest.mark.parametrize("leaf,M", [(leaf, M) for leaf in ec.LEAVES for M in ec.SIZE_EDGES[leaf]])
def test_full_build_size_edges(leaf, M):
    """Padded leaf counts on the k_subtree round edges (subtree_rounds).  The two 262k maps: 300 probes
    and the census on a 20,000-point sample, under auto and packets; everywhere else all of it."""
    big = M > ec.BIG
    kw = dict(nprobe=300, census_sample=20000) if big else {}
    _full_build(ctx_for(leaf), ec.uniform_cloud(M), f"uniform{M}", leaf, ("auto", "packets") if big else ("auto", "packets", "lane"), **kw)


# ---- batched build -------------------------------------------------------------------------------------
BATCH_SIZES = {4: (1024, 1025), 64: (16385,)}


@pytest.mark.parametrize("leaf", ec.LEAVES)
def test_batched_build(leaf):
    """Count-less targets and sources of several contexts, built together by one register_frames call:
    api_frames.hip batch_builds takes index.hip build_batch for every member whose target is pending
    (a count-less load) unless a member has per-launch timing on.  No public observable tells the two
    paths apart (both record one index-build interval per member), so the path is the code's reading;
    the members' rows must equal the brute force and the same map built alone."""
    maps = [(n, ec.geometry(n)) for n in ec.GEOMETRY] + [(f"uniform{M}", ec.uniform_cloud(M)) for M in BATCH_SIZES[leaf] + (1,)]
    ctxs = []
    try:
        for _, P in maps:
            c = imls_icp.ImlsContext(params())
            ctxs.append(c)
            c.set_option("leaf_size", leaf)
            c.set_target(ec.rows6(P), count=False)
            c.set_source(ec.rows6(P[:: max(len(P) // 48, 1)] + np.float32(0.01)), count=False)
        imls_icp.register_frames(ctxs)              # whatever statuses the degenerate frames end with
        solo = ctx_for(leaf)
        for c, (name, P) in zip(ctxs, maps):
            check_shape(c, len(P), leaf)
            check_state(c, P, name, solo=solo, raw=ec.rows6(P))
    finally:
        for c in ctxs:
            c.close()


# ---- FIFO incremental build ------------------------------------------------------------------------------
class Pusher:
    def __init__(self, c):
        self.c, self.bufs = c, []

    def push(self, scan, kind, count=True):
        if kind == "host":
            return self.c.map_push(scan, count=count)
        if len(scan) == 0:
            return self.c.map_push_device(0, 0, count=count)
        d = gpu_mem.DevSoa(np.ascontiguousarray(scan.T))
        self.bufs.append(d)
        return self.c.map_push_device(d.ptr, len(scan), count=count)

    def close(self):
        self.c.synchronize()
        for d in self.bufs:
            d.free()


def run_sequence(seq, queue, leaf, key, unchecked=(), count=True, checked=None, ref_key=None, ctx=None):
    """Push `seq` into `ctx` (default: the module's (leaf, queue) context) from an empty FIFO; checks
    after every push (in `checked`, where given) except the count-less `unchecked` ones."""
    c, solo = ctx if ctx is not None else ctx_for(leaf, queue), ctx_for(leaf, 1, "solo")
    c.map_clear()
    push, fifo = Pusher(c), []
    try:
        for j, (scan, kind) in enumerate(seq):
            cnt = count and j not in unchecked
            n = push.push(scan, kind, cnt)
            fifo.append(scan)
            if len(fifo) > queue:
                fifo.pop(0)
            assert c.map_size() == (len(fifo), sum(len(s) for s in fifo))
            if j in unchecked or (checked is not None and j not in checked):
                continue
            P = ec.filtered_map(fifo)
            if len(P) == 0:
                assert n == 0
                no_target(c)
                continue
            check_state(c, P, ref_key(j, fifo) if ref_key else f"{key}/{j}", n if cnt else None, solo=solo, raw=np.concatenate(fifo))
    finally:
        push.close()


@pytest.mark.parametrize("leaf", ec.LEAVES)
def test_fifo_ties_above_a_tile(leaf):
    """k_merge_tile / merge_split_at with equal keys from two runs across tile and thread diagonals
    (pushes 2, 3), then k_keep_* over tied runs (pushes 4, 5); leaf 4: k_fifo_gather's segmented boxes."""
    run_sequence(ec.ties_sequence(), 3, leaf, "ties")


def _copies_key(j, fifo):
    return f"stationary/x{len(fifo)}"


@pytest.mark.parametrize("leaf", ec.LEAVES)
@pytest.mark.parametrize("queue,lo,hi", [(2, 0, 4), (3, 0, 5), (31, 0, 11), (31, 11, 22), (31, 22, 33)])
def test_fifo_stationary_sensor(queue, lo, hi, leaf):
    """The same scan pushed queue + 2 times: every key of every run tied.  (Queue 31 in three spans of
    checked pushes; the pushes before a span build too.)"""
    run_sequence(ec.stationary_sequence(queue), queue, leaf, "stationary", checked=range(lo, hi), ref_key=_copies_key)


@pytest.mark.parametrize("leaf", ec.LEAVES)
def test_fifo_id_wrap(leaf):
    """70 count-less pushes of one scan, queue 31, checked every 7th: the run ids wrap (api_map.hip
    map_push: the merged order restarts) and every key is tied."""
    run_sequence(ec.id_wrap_sequence(), 31, leaf, "idwrap", count=False, checked=range(6, 70, 7), ref_key=_copies_key)


@pytest.mark.parametrize("leaf", ec.LEAVES)
@pytest.mark.parametrize("first", ["host", "device"])
def test_fifo_size_sequence(first, leaf):
    """Merged totals on k·2048 (±1), compaction inputs and outputs on k·4096 (±1), a one-point run, an
    empty old order, grow_keep across a reallocation.  Host and device pushes alternate, starting with
    either: every edge is reached through both filters.  A context of its own, created here: its order
    buffers start empty (imls_map_clear keeps them), which fifo_trace's reallocation premise assumes."""
    with imls_icp.ImlsContext(params(3)) as c:
        c.set_option("leaf_size", leaf)
        run_sequence(ec.size_sequence(first), 3, leaf, "sizes", ctx=c)


@pytest.mark.parametrize("leaf", ec.LEAVES)
@pytest.mark.parametrize("name", list(ec.empties_sequences()))
def test_fifo_empty_entries(name, leaf):
    """fifo_build's branches for n = 0 and nk = 0 entries: first (no target: knn answers
    IMLS_ERR_STATE, n_map = 0), first when the frame is computed, in the middle, evicted; NaN rows
    interleaved (the concatenated indices renumber across runs)."""
    run_sequence(ec.empties_sequences()[name], 3, leaf, f"empties-{name}")


@pytest.mark.parametrize("leaf", ec.LEAVES)
@pytest.mark.parametrize("variant", ["single", "paired"])
def test_fifo_clamped_keys(variant, leaf):
    """k_morton_fq's clamp on all three axes, positive and negative faces: checked at the build that
    runs with clamped keys and at the next, re-framed one (fifo_build, h_fifo_clamp).  paired: the two
    far scans meet in one build, two whole runs on one key."""
    run_sequence(ec.clamping_sequence(), 3, leaf, f"clamp-{variant}", unchecked=ec.CLAMP_PAIRED_UNCHECKED if variant == "paired" else ())


@pytest.mark.parametrize("leaf", ec.LEAVES)
def test_fifo_degenerate_first_frame(leaf):
    """k_fifo_frame's 1e-6 extent floor: after a first scan on one point everything clamps."""
    run_sequence(ec.degenerate_frame_sequence(), 3, leaf, "degenerate")


STATE_POSE = mr.make_pose(0.7, -0.05, 0.1, (12.5, -3.25, 0.75))


@pytest.mark.parametrize("leaf", ec.LEAVES)
def test_fifo_state_changes_with_tied_runs(leaf):
    """map_clear, map_rebase and set_target with tied runs in the FIFO."""
    c, solo = ctx_for(leaf, 3), ctx_for(leaf, 1, "solo")
    S = [s for s, _ in ec.ties_sequence()]
    c.map_clear()
    for s in S[:3]:
        c.map_push(s)
    # map_clear, then a push: that scan alone
    c.map_clear()
    n = c.map_push(S[3])
    check_state(c, ec.filtered_map([S[3]]), "state/clear", n, solo=solo, raw=S[3])
    c.map_push(S[4])
    c.map_push(S[0])
    # map_rebase: every entry re-expressed (test_gpu_posed_map.py's arithmetic); duplicates stay duplicates
    c.map_rebase(STATE_POSE)
    fifo = [mr.pose_cloud(s, STATE_POSE) for s in (S[3], S[4], S[0])]
    P = ec.filtered_map(fifo)
    assert len(np.unique(P, axis=0)) == len(np.unique(ec.filtered_map([S[3], S[4], S[0]]), axis=0))
    check_state(c, P, "state/rebase", solo=solo, raw=np.concatenate(fifo))
    # set_target replaces the index without touching the FIFO: the next push gives the FIFO's map again
    other = ec.rows6(ec.geometry("duplicate_groups"))
    n = c.set_target(other)
    check_state(c, ec.geometry("duplicate_groups"), "duplicate_groups", n)
    assert c.map_size()[0] == 3
    n = c.map_push(S[1])
    fifo = fifo[1:] + [S[1]]
    check_state(c, ec.filtered_map(fifo), "state/after-set-target", n, solo=solo, raw=np.concatenate(fifo))


@pytest.mark.parametrize("leaf", ec.LEAVES)
def test_fifo_registration_equals_full_build(leaf):
    """One registration against a 3-scan FIFO, bit-equal to the full build's (pose, iterations, status,
    trace): the leaf-4 boxes of k_fifo_gather serve the whole path, not only knn."""
    sm, scene, poses = synth.vlp16(), synth.make_scene(4), synth.trajectory(12, 2004)
    rng = np.random.default_rng(0)
    scans = []
    for k in range(4):
        s = synth.scan(scene, sm, poses[5 + k], seed=4000 + k)
        scans.append(s[np.sort(rng.choice(len(s), 2500, replace=False))].copy())
    p = params(3)
    out = []
    for fifo in (True, False):
        with imls_icp.ImlsContext(p) as c:
            c.set_option("leaf_size", leaf)
            if fifo:
                for s in scans[:3]:
                    c.map_push(s)
            else:
                c.set_target(np.concatenate(scans[:3]))
            c.set_source(scans[3])
            out.append(c.register_frame())
    _same(out[0], out[1], leaf)


# ---- small source order ------------------------------------------------------------------------------------
@pytest.mark.parametrize("trav", ["auto", "packets"])
@pytest.mark.parametrize("n", [ec.SMALL_ORDER_N - 1, ec.SMALL_ORDER_N, ec.SMALL_ORDER_N + 1])
def test_small_source_order_with_massive_ties(n, trav):
    """k_small_order (≤ 2,048 points) and the radix path (2,049) on a source of which 1,500 points are
    one point: project() against the oracle — masks, counters, x and idx exact, y within 1e-5."""
    g = np.load(GOLDEN / "vlp16_pair.npz")
    p = params()
    tgt_rows = np.ascontiguousarray(g["tgt"].T)
    src = ec.small_source(np.ascontiguousarray(np.concatenate([g["src"].T, g["tgt"].T[::40]])), n)
    want = oc.project(np.ascontiguousarray(src.T), np.ascontiguousarray(g["tgt"], np.float32), g["pose1"], p)
    c = ctx_for(64, 1, "project")
    try:
        c.set_option("traversal", TRAVERSALS[trav])
        c.set_target(tgt_rows)
        kept = c.set_source(src)
        assert len(kept) == n
        x, y, nn, idx, rej = c.project(g["pose1"])
    finally:
        c.set_option("traversal", _abi.IMLS_TRAVERSAL_AUTO)
    wx, wy, wn, widx, wrej = want
    assert np.array_equal(rej, wrej) and np.array_equal(idx, widx)
    assert np.array_equal(x, wx) and np.array_equal(nn, wn)
    assert len(idx) > 0 and np.abs(y.astype(np.float64) - wy).max() <= Y_TOL
