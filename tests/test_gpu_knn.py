"""The public kNN query (imls_knn / imls_knn_device; ImlsContext.knn / knn_device) against the CPU
oracle's restatement of libnabo NNSearchD::knn (oracle_ctypes.knn: epsilon 0, SORT_RESULTS).

The comparison is exact: the indices (positions in the NaN-filtered target) and the fp64 d² — the
same expression ((dx²+dy²)+dz²) on the same floats, so there is nothing to tolerate — with
np.array_equal, and found == filled slots.  Covered: radius (inclusive, unbounded), self-match rule,
tie order on exact duplicates, unfound slots, targets smaller than k, non-finite queries and target
points, every traversal mode, the forced fallback, leaf sizes, the map FIFO, launch-shape
boundaries, buffer regrowth, the device form, the error codes, and that a query between the steps of
a registration changes nothing the registration computes."""
import ctypes as C
import functools
import pathlib

import numpy as np
import pytest

import index_edge_cases
import oracle_ctypes as oc
from planetary_lidar_odometry_amd import _abi, config, imls_icp, synth

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
TRAVERSALS = {"auto": _abi.IMLS_TRAVERSAL_AUTO, "packets": _abi.IMLS_TRAVERSAL_PACKETS,
              "wave_per_query": _abi.IMLS_TRAVERSAL_WAVE_PER_QUERY, "lane": _abi.IMLS_TRAVERSAL_LANE}


def rows(soa6):
    return np.ascontiguousarray(np.asarray(soa6, np.float32).T)


def soa6_of(xyz):
    """(6, M) float32 target from (M, 3) points, normals +z."""
    xyz = np.asarray(xyz, np.float32)
    out = np.zeros((6, len(xyz)), np.float32)
    out[:3] = xyz.T
    out[5] = 1.0
    return out


@functools.lru_cache(maxsize=None)
def golden_pair(name="vlp16_pair"):
    g = np.load(GOLDEN / f"{name}.npz")
    tgt = np.ascontiguousarray(g["tgt"], np.float32)
    q = np.ascontiguousarray(g["src"][:3].T, np.float32)
    return tgt, q


_ORACLE = {}


def oracle(key, tgt6, q, k, r, self_ok):
    """oracle_ctypes.knn on (target, queries) named `key`, computed once per argument set."""
    full = (key, k, float(r), bool(self_ok))
    if full not in _ORACLE:
        d2, idx = oc.knn(tgt6, np.ascontiguousarray(q[:, :3].T), k, float(r), self_ok)
        _ORACLE[full] = (idx, d2)
    return _ORACLE[full]


def check(got, want, label=""):
    idx, d2, found = got
    widx, wd2 = want
    assert idx.dtype == np.int32 and d2.dtype == np.float64 and found.dtype == np.int32
    bad = np.nonzero((idx != widx).any(axis=1) | (d2 != wd2).any(axis=1))[0]
    assert bad.size == 0, (label, bad[:5], idx[bad[:2]], widx[bad[:2]], d2[bad[:2]], wd2[bad[:2]])
    assert np.array_equal(idx, widx) and np.array_equal(d2, wd2), label
    assert np.array_equal(found, (idx >= 0).sum(axis=1)), label


def params():
    p = config.bench_params(6)
    return p


@pytest.fixture(scope="module")
def ctx():
    c = imls_icp.ImlsContext(params())
    yield c
    c.close()


@pytest.fixture(params=list(TRAVERSALS), scope="module")
def tctx(request, ctx):
    """The module's context under each traversal option (auto, packets, one wave per query, lane)."""
    ctx.set_option("traversal", TRAVERSALS[request.param])
    yield ctx
    ctx.set_option("traversal", _abi.IMLS_TRAVERSAL_AUTO)


# 1 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_ok", [0, 1])
@pytest.mark.parametrize("r", [0.5, 3.0, np.inf])
@pytest.mark.parametrize("k", [1, 6, 20, 32])
def test_golden_pair(tctx, k, r, self_ok):
    tgt, q = golden_pair()
    tctx.set_target(rows(tgt))
    check(tctx.knn(q, k, r, bool(self_ok)), oracle("golden", tgt, q, k, r, self_ok), (k, r, self_ok))


# 2 -------------------------------------------------------------------------------------------
def lattice():
    g = np.arange(8, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    tgt = np.concatenate([pts, pts])                       # every point stored twice
    q = np.concatenate([pts, pts[(pts < 7).all(axis=1)] + 0.5]).astype(np.float32)
    return soa6_of(tgt), q


def brute(tgt6, q, k, r, self_ok):
    """The shared brute force (index_edge_cases.brute_knn) on an SoA target."""
    return index_edge_cases.brute_knn(tgt6[:3].T, q, k, r, self_ok)


@pytest.mark.parametrize("self_ok", [0, 1])
@pytest.mark.parametrize("r", [1.0, 1.5, np.inf])
def test_ties_and_duplicates(tctx, r, self_ok):
    tgt, q = lattice()
    tctx.set_target(rows(tgt))
    got = tctx.knn(q, 20, r, bool(self_ok))
    check(got, oracle("lattice", tgt, q, 20, r, self_ok), (r, self_ok))
    check(got, brute(tgt, q, 20, r, self_ok), ("brute", r, self_ok))


# 3 -------------------------------------------------------------------------------------------
def test_heavy_self_duplication(tctx):
    """A query on 40 copies of itself, self-match off, k = 8: the list of 12 holds only copies, all
    dropped — the certificate counts accepted entries, so the exact search answers (not a short row)."""
    rng = np.random.default_rng(5)
    p0 = np.array([[1.25, -2.5, 0.75]], np.float32)
    others = (p0 + rng.uniform(-2, 2, (30, 3))).astype(np.float32)
    xyz = np.concatenate([np.repeat(p0, 40, axis=0), others])
    xyz = xyz[rng.permutation(len(xyz))]
    tgt = soa6_of(xyz)
    tctx.set_target(rows(tgt))
    idx, d2, found = tctx.knn(p0, 8, np.inf, False)
    widx, wd2 = oc.knn(tgt, np.ascontiguousarray(p0.T), 8, np.inf, False)[::-1]
    assert found[0] == 8
    assert np.array_equal(idx, widx) and np.array_equal(d2, wd2)
    assert (d2 > 0).all() and not np.isin(idx[0], np.nonzero((xyz == p0).all(axis=1))[0]).any()
    # and with a radius that holds only 3 of the distinct points
    r = float(np.sqrt(np.sort(wd2[0])[2]))
    check(tctx.knn(p0, 8, r, False), oc.knn(tgt, np.ascontiguousarray(p0.T), 8, r, False)[::-1])


# 4 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,k", [(1, 8), (5, 8), (64, 32), (65, 32)])
def test_small_targets(tctx, M, k):
    rng = np.random.default_rng(M)
    xyz = rng.uniform(-3, 3, (M, 3)).astype(np.float32)
    q = np.concatenate([xyz, rng.uniform(-4, 4, (40, 3)).astype(np.float32)])
    tgt = soa6_of(xyz)
    tctx.set_target(rows(tgt))
    for r, self_ok in ((np.inf, True), (np.inf, False), (2.0, True)):
        got = tctx.knn(q, k, r, self_ok)
        check(got, oc.knn(tgt, np.ascontiguousarray(q.T), k, r, self_ok)[::-1], (M, k, r, self_ok))
        if M < k:
            assert (got[0][:, M:] == -1).all() and np.isinf(got[1][:, M:]).all()


# 5 -------------------------------------------------------------------------------------------
def test_nothing_in_range(tctx):
    tgt, q = golden_pair()
    tctx.set_target(rows(tgt))
    far = (q[:300] + np.float32(500.0)).astype(np.float32)
    idx, d2, found = tctx.knn(far, 20, 3.0, True)
    assert (idx == -1).all() and np.isinf(d2).all() and (found == 0).all()


# 6 -------------------------------------------------------------------------------------------
def test_non_finite_queries(tctx):
    tgt, q = golden_pair()
    q = q[:700].copy()
    badrows = np.array([0, 1, 63, 64, 65, 130, 255, 256, 400, 699])
    vals = [np.nan, np.inf, -np.inf]
    for n, i in enumerate(badrows):
        q[i, n % 3] = vals[n % 3]
    q[130] = np.nan
    tctx.set_target(rows(tgt))
    idx, d2, found = tctx.knn(q, 20, 3.0, True)
    assert (idx[badrows] == -1).all() and np.isinf(d2[badrows]).all() and (found[badrows] == 0).all()
    ok = np.setdiff1d(np.arange(len(q)), badrows)
    widx, wd2 = oc.knn(tgt, np.ascontiguousarray(q[ok].T), 20, 3.0, True)[::-1]
    check((idx[ok], d2[ok], found[ok]), (widx, wd2))


def test_target_with_nan_points(tctx):
    tgt, q = golden_pair()
    tgt = tgt.copy()
    rng = np.random.default_rng(3)
    bad = rng.choice(tgt.shape[1], 500, replace=False)
    tgt[rng.integers(0, 3, 500), bad] = np.nan
    tgt[0, bad[:50]] = np.inf
    n = tctx.set_target(rows(tgt))
    assert n == int(np.isfinite(tgt[:3]).all(axis=0).sum()) <= tgt.shape[1] - 500
    got = tctx.knn(q[:600], 20, 3.0, False)
    check(got, oc.knn(tgt, np.ascontiguousarray(q[:600].T), 20, 3.0, False)[::-1])
    assert got[0].max() < n


# 7 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_launch_shape_boundaries(tctx, nq):
    tgt, q = golden_pair()
    tctx.set_target(rows(tgt))
    idx, d2, found = tctx.knn(q[:nq], 20, 3.0, True)
    assert idx.shape == (nq, 20) and d2.shape == (nq, 20) and found.shape == (nq,)
    widx, wd2 = oracle("golden", tgt, q, 20, 3.0, 1)
    check((idx, d2, found), (widx[:nq], wd2[:nq]), nq)


def test_odd_k_rows(ctx):
    """k = 5 and 7: rows that are not 16-byte aligned take the element-store path."""
    tgt, q = golden_pair()
    ctx.set_target(rows(tgt))
    for k in (5, 7, 18):
        check(ctx.knn(q[:500], k, 3.0, False), oracle("golden500", tgt, q[:500], k, 3.0, 0), k)


@pytest.mark.parametrize("k", [9, 16])
def test_list_size_rung_8_to_16(tctx, k):
    """8 < k ≤ 16: the list-size rung (list length 20, heap capacity 16) between the ones k = 6 and
    k = 20 take, at its two ends, in every traversal mode; the map and queries of
    tests/test_gpu_knn_steps.py (5003 points, 333 queries), against the shared brute force."""
    import test_gpu_knn_steps as steps
    cl = steps.build_clouds()
    tgt6 = synth.soa(cl["tgt"])
    q = np.ascontiguousarray(synth.soa(cl["spread"])[:3].T, np.float32)
    tctx.set_target(cl["tgt"])
    for r, self_ok in ((3.0, True), (np.inf, False)):
        check(tctx.knn(q, k, r, self_ok), brute(tgt6, q, k, r, self_ok), (k, r, self_ok))


def test_strided_queries(ctx):
    """Queries taken from a wider array (stride 6 floats)."""
    tgt, q = golden_pair()
    ctx.set_target(rows(tgt))
    wide = np.ascontiguousarray(np.concatenate([q[:500], np.full((500, 3), np.nan, np.float32)], axis=1))
    check(ctx.knn(wide, 6, 3.0, True), oracle("golden500", tgt, q[:500], 6, 3.0, 1))


# 8 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("trav", ["auto", "packets"])
def test_forced_fallback(every, trav):
    tgt, q = golden_pair()
    with imls_icp.ImlsContext(params()) as c:
        c.set_option("traversal", TRAVERSALS[trav])
        c.set_target(rows(tgt))
        want = c.knn(q, 20, 3.0, False)
        check(want, oracle("golden", tgt, q, 20, 3.0, 0))
        c.set_option("force_fallback", every)
        for k, r, self_ok in ((20, 3.0, False), (32, np.inf, True), (6, 0.5, True)):
            check(c.knn(q, k, r, self_ok), oracle("golden", tgt, q, k, r, int(self_ok)), (every, k, r))


# 9 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", [4, 64])
@pytest.mark.parametrize("trav", ["auto", "packets", "lane"])
def test_leaf_size(leaf, trav):
    tgt, q = golden_pair()
    with imls_icp.ImlsContext(params()) as c:
        c.set_option("leaf_size", leaf)
        c.set_option("traversal", TRAVERSALS[trav])
        c.set_target(rows(tgt))
        check(c.knn(q, 20, 3.0, True), oracle("golden", tgt, q, 20, 3.0, 1), (leaf, trav))
        check(c.knn(q, 6, np.inf, False), oracle("golden", tgt, q, 6, np.inf, 0), (leaf, trav))


# 10 ------------------------------------------------------------------------------------------
def test_fifo_map():
    sm = synth.vlp16()
    scene = synth.make_scene(4)
    poses = synth.trajectory(12, 2004)
    rng = np.random.default_rng(0)
    scans = []
    for k in range(4):
        s = synth.scan(scene, sm, poses[5 + k], seed=4000 + k)
        s = s[np.sort(rng.choice(len(s), 2500, replace=False))].copy()
        s["x"][rng.choice(len(s), 20, replace=False)] = np.nan       # the filter renumbers the map
        scans.append(s)
    q = np.stack([scans[3][f] for f in "xyz"], 1).astype(np.float32)[:800]
    q = q[np.isfinite(q).all(axis=1)]
    p = params()
    p.max_queue_size = 3
    with imls_icp.ImlsContext(p) as c:
        for k in range(3):
            c.map_push(scans[k])
        cat = synth.soa(np.concatenate(scans[:3]))
        check(c.knn(q, 20, 3.0, True), oc.knn(cat, np.ascontiguousarray(q.T), 20, 3.0, True)[::-1], "fifo 0-2")
        c.map_push(scans[3], count=False)                # a deferred build: completed by the query
        cat = synth.soa(np.concatenate(scans[1:4]))
        check(c.knn(q, 20, 3.0, False), oc.knn(cat, np.ascontiguousarray(q.T), 20, 3.0, False)[::-1], "fifo 1-3")


# 11 ------------------------------------------------------------------------------------------
def test_packets_at_scale():
    pair = synth.make_pair("hdl64", map_scans=1)
    tgt = synth.soa(pair.target)
    src = np.stack([pair.source[f] for f in "xyz"], 1).astype(np.float32)
    rng = np.random.default_rng(1)
    q = src[np.sort(rng.choice(len(src), 20000, replace=False))]
    assert len(q) > 16384                                 # above the auto threshold: the packet kernel
    with imls_icp.ImlsContext(params()) as c:
        M = c.set_target(pair.target)
        idx, d2, found = c.knn(q, 20, 3.0, True)
    sub = np.sort(rng.choice(len(q), 2000, replace=False))
    widx, wd2 = oc.knn(tgt, np.ascontiguousarray(q[sub].T), 20, 3.0, True)[::-1]
    check((idx[sub], d2[sub], found[sub]), (widx, wd2))
    filled = idx >= 0
    assert np.array_equal(found, filled.sum(axis=1))
    assert (filled[:, :-1] >= filled[:, 1:]).all()        # filled slots first
    assert (idx[filled] < M).all() and (d2[filled] <= 9.0).all() and np.isinf(d2[~filled]).all()
    with np.errstate(invalid="ignore"):                   # inf − inf between unfound slots
        step = np.diff(d2, axis=1)
    assert (step[filled[:, 1:]] >= 0).all()
    tie = (step == 0) & filled[:, 1:]
    assert (np.diff(idx, axis=1)[tie] > 0).all()


# 12 ------------------------------------------------------------------------------------------
def _frame_key(r):
    return (r["pose"].tobytes(), r["iters"], r["status"], tuple(bytes(t) for t in r["trace"]))


def _registration(p, with_knn):
    g = np.load(GOLDEN / "vlp16_pair.npz")
    tgt, src = rows(g["tgt"]), rows(g["src"])
    q = np.ascontiguousarray(tgt[::4, :3])
    out = []
    with imls_icp.ImlsContext(p) as c:
        def probe():
            if with_knn:
                c.knn(q, 20, 3.0, True)
                c.knn(q[:100], 7, np.inf, False)
        c.set_target(tgt)
        probe()
        c.set_source(src)
        probe()
        out.append(_frame_key(c.register_frame()))
        probe()
        out.append(_frame_key(c.register_frame()))
        probe()
        x, y, n, idx, rej = c.project(g["pose1"])
        out.append(tuple(a.tobytes() for a in (x, y, n, idx, rej)))
        probe()
        out.append(_frame_key(c.register_frame()))
        out.append(c.rng_state().tobytes())
    return out


@pytest.mark.parametrize("solver", ["LS", "RANSAC_DRPM"])
def test_no_interference_with_registration(solver):
    if solver == "LS":
        p = config.bench_params(8)
    else:
        p = config.params_from_config(config.load())     # RANSAC → DRPM: the rand() stream runs on
        p.iterations = 6
        assert p.solve_method == _abi.IMLS_SOLVE_RANSAC and p.ransac_final_method == _abi.IMLS_FINAL_DRPM
    assert _registration(p, False) == _registration(p, True)


# 13 ------------------------------------------------------------------------------------------
def test_device_form(ctx):
    import gpu_mem
    hip = gpu_mem.product_hip()
    tgt, q = golden_pair()
    nq, k = 1500, 20
    ctx.set_option("traversal", _abi.IMLS_TRAVERSAL_AUTO)
    ctx.set_target(rows(tgt))
    want = ctx.knn(q[:nq], k, 3.0, False)
    dq = gpu_mem.DevSoa(np.ascontiguousarray(q[:nq].T))                 # SoA float32[3][nq]
    didx = gpu_mem.DevSoa(np.zeros(nq * k, np.float32))
    dd2 = gpu_mem.DevSoa(np.zeros(2 * nq * k, np.float32))
    dfound = gpu_mem.DevSoa(np.zeros(nq, np.float32))
    try:
        ctx.knn_device(dq.ptr, nq, k, 3.0, False, didx.ptr, dd2.ptr, dfound.ptr)
        ctx.synchronize()
        dq.overwrite(np.full((3, nq), np.nan, np.float32))              # the queries are free again
        idx = np.zeros((nq, k), np.int32); d2 = np.zeros((nq, k)); found = np.zeros(nq, np.int32)
        for host, dev in ((idx, didx), (d2, dd2), (found, dfound)):
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(dev.ptr), host.nbytes, 2) == 0
        check((idx, d2, found), want[:2])
        assert np.array_equal(found, want[2])
        # without the count array
        ctx.knn_device(dq.ptr, nq, k, 3.0, False, didx.ptr, dd2.ptr)
        ctx.synchronize()
        assert hip.hipMemcpy(idx.ctypes.data_as(C.c_void_p), C.c_void_p(didx.ptr), idx.nbytes, 2) == 0
        assert (idx == -1).all()                                        # the overwritten (NaN) queries
    finally:
        for b in (dq, didx, dd2, dfound):
            b.free()


# 14 ------------------------------------------------------------------------------------------
def _status(fn):
    with pytest.raises(_abi.ImlsError) as e:
        fn()
    return e.value.status


def test_errors():
    tgt, q = golden_pair()
    q = q[:50]
    with imls_icp.ImlsContext(params()) as c:
        assert _status(lambda: c.knn(q, 4)) == _abi.IMLS_ERR_STATE                  # no target
        c.set_target(rows(tgt))
        assert _status(lambda: c.knn(q, 0)) == _abi.IMLS_ERR_UNSUPPORTED
        assert _status(lambda: c.knn(q, 33)) == _abi.IMLS_ERR_UNSUPPORTED
        for r in (0.0, -1.0, np.nan):
            assert _status(lambda: c.knn(q, 4, r)) == _abi.IMLS_ERR_ARG
        idx = np.zeros((50, 4), np.int32); d2 = np.zeros((50, 4))
        rc = c.lib.imls_knn(c.ctx, q.ctypes.data_as(C.c_void_p), 3, 50, 4, 1.0, 6,
                            idx.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p), None)
        assert rc == _abi.IMLS_ERR_ARG                                              # unknown flag bits
        for bad in (np.zeros((5, 2), np.float32), np.zeros(9, np.float32), np.zeros((2, 3, 3), np.float32)):
            with pytest.raises(ValueError):
                c.knn(bad, 4)
        c.set_source(rows(np.load(GOLDEN / "vlp16_pair.npz")["src"]))
        c.register_frame_async()
        assert _status(lambda: c.knn(q, 4)) == _abi.IMLS_ERR_STATE                  # frame pending
        c.register_frame_result()
        check(c.knn(q, 4, 3.0), oc.knn(tgt, np.ascontiguousarray(q.T), 4, 3.0, True)[::-1])


# 15 ------------------------------------------------------------------------------------------
def test_grow():
    tgt, q = golden_pair()
    small = q[:40]
    big = np.concatenate([q, (q + np.float32(0.05)).astype(np.float32)])[: 50 * 40]
    with imls_icp.ImlsContext(params()) as c:
        c.set_target(rows(tgt))
        for name, qq in (("small", small), ("big", big), ("small", small)):
            check(c.knn(qq, 20, 3.0, True), oracle("grow-" + name, tgt, qq, 20, 3.0, 1), name)


# 16 ------------------------------------------------------------------------------------------
def test_chunked_query_sets(ctx):
    """More than one chunk (262144 queries per launch sequence, include/imls_gpu.h): the host form and
    the device form (whose later chunks start inside the caller's SoA arrays) equal the oracle."""
    import gpu_mem
    hip = gpu_mem.product_hip()
    tgt, q0 = golden_pair()
    nq, k = 262144 + 777, 6
    rng = np.random.default_rng(11)
    q = (q0[rng.integers(0, len(q0), nq)] + rng.uniform(-0.5, 0.5, (nq, 3))).astype(np.float32)
    ctx.set_option("traversal", _abi.IMLS_TRAVERSAL_AUTO)
    ctx.set_target(rows(tgt))
    want = oc.knn(tgt, np.ascontiguousarray(q.T), k, 1.0, True)[::-1]
    got = ctx.knn(q, k, 1.0, True)
    check(got, want, "host form")
    dq = gpu_mem.DevSoa(np.ascontiguousarray(q.T))
    didx = gpu_mem.DevSoa(np.zeros(nq * k, np.float32))
    dd2 = gpu_mem.DevSoa(np.zeros(2 * nq * k, np.float32))
    dfound = gpu_mem.DevSoa(np.zeros(nq, np.float32))
    try:
        ctx.knn_device(dq.ptr, nq, k, 1.0, True, didx.ptr, dd2.ptr, dfound.ptr)
        ctx.synchronize()
        idx = np.zeros((nq, k), np.int32); d2 = np.zeros((nq, k)); found = np.zeros(nq, np.int32)
        for host, dev in ((idx, didx), (d2, dd2), (found, dfound)):
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(dev.ptr), host.nbytes, 2) == 0
        check((idx, d2, found), want, "device form")
    finally:
        for b in (dq, didx, dd2, dfound):
            b.free()
