"""Tensor-voting normals (csrc/tv.hip) at their edges, device against the CPU oracle — tv_cases.py builds
the cases, test_tv_cases.py proves on the CPU that each reaches its edge, that every query's voted normal
is visible (valid, or counted in reject[no_normal]), and that a kernel wrong in one of eight named ways
would move a subject query by more than 100 × the tolerance used here.

Per projection, against oracle_ctypes.project at the same pose: the six reject counters, idx and x equal;
y within 1e-5 m (the projection's parity contract); n within 2⁻²⁴ + B_q per component, B_q from the
restated vote of that query (tv_cases.vote: the sum's sensitivity to an exp() an ulp off and the Jacobi's
backward error over the eigenvalue gap; test_tv_cases.py).  Rows whose B_q exceeds 1e-7, whose |λ| pick
is not stable or whose n_z is within 100 ulp of 0 are left out of the n comparison: at most 5 % of a
projection's valid rows, asserted (none so far).

Frames: the device's own pose of every iteration is projected by the oracle, so every captured row is
compared (a pose of the oracle's own run would differ in the last bits and move x by an ulp); the final
pose is compared with the oracle's register_frame within 1e-6.

Measured on an MI355X: 48 projections, 14,644 rows compared; largest |Δn| / (2⁻²⁴ + B_q) 0 (the device's n
is the oracle's float on every row); largest |Δy| 2.4e-7; no row left out of the n comparison in any case;
slowest test 1.1 s (test_big_frame), the file 5.1 s.  No defect found.

Device tensors live in a buffer of the HIP runtime the library uses (gpu_mem.DevSoa): a second runtime —
torch's — cannot open the device in the same process.
"""
import ctypes as C

import numpy as np
import pytest

import gpu_mem
import oracle_ctypes as oc
import tv_cases as tc
from planetary_lidar_odometry_amd import _abi, imls_icp

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-6
FIG = dict(rows=0, projections=0, ratio=0.0, dy=0.0, left=0)


@pytest.fixture(scope="module")
def ctx():
    c = imls_icp.ImlsContext(tc.params(tc.scene_self(), tc.SELF_K))
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    print(f"\ntv edges: {FIG['projections']} projections, {FIG['rows']} rows compared, largest |Δn| / (2⁻²⁴ + B_q) "
          f"{FIG['ratio']:.3f}, largest |Δy| {FIG['dy']:.3e}, rows left out of the n comparison {FIG['left']}")


def load(c, s, k, iters=3):
    c.set_params(tc.params(s, k, iters))
    assert c.set_target(s.tgt) == int(np.isfinite(s.tgt[:, :3]).all(axis=1).sum())
    c.set_target_tensors(s.ten)
    assert len(c.set_source(s.src)) == len(s.src)


def against_oracle(got, s, k, pose=None, iters=3, votes=None, label=""):
    """One projection `got` = (x, y, n, idx, rej) of the device against the oracle at the same pose."""
    x, y, n, idx, rej = got
    wx, wy, wn, widx, wrej = tc.oracle_project(s, k, pose, iters)
    assert np.array_equal(rej, wrej), (label, rej, wrej)
    assert np.array_equal(idx, widx), label
    assert np.array_equal(x, wx), label
    dy = float(np.abs(y.astype(np.float64) - wy).max()) if len(idx) else 0.0
    if votes is None:
        votes = [tc.votes(s, k)[r] for r in idx] if pose is None else tc.bounds_at(s, k, x)
    worst, left, bad = 0.0, 0, []
    for j, v in enumerate(votes):
        if not tc.comparable(v):
            left += 1
            continue
        ratio = float(np.abs(n[j].astype(np.float64) - wn[j].astype(np.float64)).max() / tc.tol_of(v))
        worst = max(worst, ratio)
        if ratio > 1.0:
            bad.append((int(idx[j]), ratio, n[j], wn[j]))
    # rows that are not compared by the bound still agree in whether the normal is finite
    assert np.array_equal(np.isfinite(n).all(axis=1), np.isfinite(wn).all(axis=1)), label
    FIG["rows"] += len(idx) - left
    FIG["projections"] += 1
    FIG["ratio"] = max(FIG["ratio"], worst)
    FIG["dy"] = max(FIG["dy"], dy)
    FIG["left"] += left
    print(f"{label}: valid {len(idx)} rej {[int(r) for r in rej]} |Δn|/tol {worst:.3f} |Δy| {dy:.2e} left out {left}")
    assert not bad, (label, bad[:3])
    assert left <= 0.05 * max(len(idx), 1), (label, left)
    assert (n[:, 2] >= 0).all(), label
    assert dy <= tc.Y_TOL, (label, dy)
    return votes


# ---- every case ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(tc.CASE_LIST)), ids=tc.CASE_IDS)
def test_case(ctx, i):
    fn, a, k = tc.CASE_LIST[i]
    s = fn(*a)
    load(ctx, s, k)
    got = ctx.project()
    against_oracle(got, s, k, label=f"{s.name}/k{k}")
    idx = set(int(r) for r in got[3])
    for sub in s.subjects:                       # each subject is in the category its case names
        assert (sub.row in idx) == (sub.category == "valid"), sub.name


# ---- who reads tvn ---------------------------------------------------------------------------------------------------
TRAVERSALS = {"packets": _abi.IMLS_TRAVERSAL_PACKETS, "wave_per_query": _abi.IMLS_TRAVERSAL_WAVE_PER_QUERY,
              "lane": _abi.IMLS_TRAVERSAL_LANE}


@pytest.mark.parametrize("fallback", [0, 1])
@pytest.mark.parametrize("trav", list(TRAVERSALS))
def test_every_traversal_reads_the_voted_normal(trav, fallback):
    s, k = tc.scene_ball(50), 50
    with imls_icp.ImlsContext(tc.params(s, k)) as c:
        c.set_option("traversal", TRAVERSALS[trav])
        c.set_option("force_fallback", fallback)
        load(c, s, k)
        against_oracle(c.project(), s, k, label=f"{trav}/fallback{fallback}")


@pytest.mark.parametrize("leaf", [4, 64])
def test_leaf_sizes(leaf):
    s, k = tc.scene_ties(), 50
    with imls_icp.ImlsContext(tc.params(s, k)) as c:
        c.set_option("leaf_size", leaf)
        load(c, s, k)
        against_oracle(c.project(), s, k, label=f"leaf{leaf}")


def test_big_frame(ctx):
    """4,200 source rows: above kSmallRows the large-frame projection kernels read tvn."""
    s, k = tc.scene_big(), tc.FRAME_K
    assert len(s.src) > 4096
    load(ctx, s, k)
    against_oracle(ctx.project(), s, k, label="big-frame")


@pytest.mark.parametrize("n", tc.SMALL_N)
def test_small_n(ctx, n):
    s, k = tc.scene_small(n), tc.FRAME_K
    load(ctx, s, k)
    got = ctx.project()
    assert len(got[3]) == n
    against_oracle(got, s, k, label=f"small-n{n}")


# ---- frames: skin lists over several iterations ----------------------------------------------------------------------
def run_frame(s, k, iters, skin):
    with imls_icp.ImlsContext(tc.params(s, k, iters)) as c:
        c.set_option("tv_skin", skin)
        load(c, s, k, iters)
        c.capture_correspondences(True)
        r = c.register_frame()
        r["captured"] = [c.captured(it) for it in range(r["iters"])]
    return r


def same_trace(a, b):
    return len(a) == len(b) and all(list(t.delta) == list(u.delta) and list(t.pose) == list(u.pose) and
                                    list(t.reject) == list(u.reject) and t.n_valid == u.n_valid and t.n_kept == u.n_kept
                                    for t, u in zip(a, b))


def test_skins_equal_each_other_and_the_oracle():
    """register_frame with tv_skin 0, 0.01, 0.03, 0.3 and 1.0 on the crafted frame (tv_cases.scene_frame:
    list-64 / list-65, both overflows, the self match that becomes a voter, queries that walk again and
    reuse later): every skin bit-equal to skin 0 in pose, iterations, status, trace and every captured row,
    and every iteration's rows equal to the oracle's projection at that iteration's pose."""
    s, k, iters = tc.scene_frame(), tc.FRAME_K, tc.FRAME_ITERS
    runs = {skin: run_frame(s, k, iters, skin) for skin in tc.SKINS}
    ref = runs[0.0]
    assert ref["iters"] == iters >= 3
    for skin, r in runs.items():
        assert np.array_equal(r["pose"], ref["pose"]) and (r["iters"], r["status"]) == (ref["iters"], ref["status"]), skin
        assert same_trace(r["trace"], ref["trace"]), skin
        for it in range(iters):
            for a, b in zip(r["captured"][it], ref["captured"][it]):
                assert np.array_equal(a, b), (skin, it)
    poses = tc.frame_poses(ref)
    for it, T in enumerate(poses):
        x, y, n, idx = ref["captured"][it]
        rej = np.array(list(ref["trace"][it].reject), np.uint64)
        assert ref["trace"][it].n_valid == len(idx)
        against_oracle((x, y, n, idx, rej), s, k, T, iters, label=f"frame it {it}")
    want = tc.oracle_frame(s, k, iters)
    assert (want["iters"], want["status"]) == (ref["iters"], ref["status"])
    assert np.abs(ref["pose"] - want["pose"]).max() <= POSE_TOL


def test_skins_through_the_batched_entry():
    """The same skins through register_frames (k_tv_vote_b: grid y = frame) on the crafted frame beside a
    smaller member: every member bit-equal, at every skin, to its own register_frame at skin 0 — which the
    test above and test_batch_mixed hold to the oracle."""
    scenes, k, iters = [tc.scene_frame(), tc.batch_scenes()[1]], tc.FRAME_K, tc.FRAME_ITERS
    alone = [run_frame(s, k, iters, 0.0) for s in scenes]
    for skin in tc.SKINS:
        ctxs = [imls_icp.ImlsContext(tc.params(s, k, iters)) for s in scenes]
        try:
            for c, s in zip(ctxs, scenes):
                c.set_option("tv_skin", skin)
                load(c, s, k, iters)
            poses, its, status, traces = imls_icp.register_frames(ctxs)
        finally:
            for c in ctxs:
                c.close()
        for m, one in enumerate(alone):
            assert np.array_equal(one["pose"], poses[m]) and (one["iters"], one["status"]) == (its[m], status[m]), (skin, m)
            assert same_trace(one["trace"], list(traces[m])), (skin, m)


# ---- batches ---------------------------------------------------------------------------------------------------------
def test_batch_mixed():
    """register_frames over members of N = 3, 257 and 601 with different targets (grid x sized by the
    largest member, the smaller ones return early): each member bit-equal to its own register_frame and
    equal to the oracle."""
    scenes, k, iters = tc.batch_scenes(), tc.FRAME_K, 4
    alone = [run_frame(s, k, iters, 0.03) for s in scenes]
    ctxs = [imls_icp.ImlsContext(tc.params(s, k, iters)) for s in scenes]
    try:
        for c, s in zip(ctxs, scenes):
            load(c, s, k, iters)
        poses, its, status, traces = imls_icp.register_frames(ctxs)
    finally:
        for c in ctxs:
            c.close()
    for m, (s, one) in enumerate(zip(scenes, alone)):
        assert np.array_equal(one["pose"], poses[m]) and (one["iters"], one["status"]) == (its[m], status[m]), m
        assert same_trace(one["trace"], list(traces[m])), m
        want = oc.register_frame(tc.soa(s.src), tc.soa(s.tgt), tc.params(s, k, iters), tensors=tc.soa(s.ten))
        assert (want["iters"], want["status"]) == (its[m], status[m]), m
        assert np.abs(poses[m] - want["pose"]).max() <= POSE_TOL, m
        for t, u in zip(one["trace"], want["trace"]):
            assert list(t.reject) == list(u.reject) and t.n_valid == u.n_valid, m
        for it, T in enumerate(tc.frame_poses(one)):
            x, y, n, idx = one["captured"][it]
            against_oracle((x, y, n, idx, np.array(list(one["trace"][it].reject), np.uint64)), s, k, T, iters,
                           label=f"batch member {m} it {it}")


# ---- tensor inputs ---------------------------------------------------------------------------------------------------
def test_tensor_inputs():
    """Every way of handing the tensors over, on the NaN-rows variant of the ties scene (NaN rows at the
    first, a middle and the last input position: records follow the input order)."""
    s, k = tc.scene_ties(True), 50
    n_in, n_kept = len(s.tgt), len(s.tgt) - 3
    p = tc.params(s, k)
    dev_t, dev_g = gpu_mem.DevSoa(tc.soa(s.ten)), gpu_mem.DevSoa(tc.soa(s.tgt))
    try:
        with imls_icp.ImlsContext(p) as c:
            # a row stride of 9 floats, through the library entry
            wide = np.full((n_in, 9), 7.0, np.float32)
            wide[:, :6] = s.ten
            assert c.set_target(s.tgt) == n_kept
            c._check(c.lib.imls_set_target_tensors(c.ctx, wide.ctypes.data_as(C.c_void_p), n_in, 9))
            c.set_source(s.src)
            against_oracle(c.project(), s, k, label="stride 9")
            # the device form, SoA [6][n]
            assert c.set_target(s.tgt) == n_kept
            c.set_target_tensors_device(dev_t.ptr, n_in)
            against_oracle(c.project(), s, k, label="device tensors")
            # the device form while a count-less set_target is still pending
            assert c.set_target(s.tgt, count=False) is None
            c.set_target_tensors_device(dev_t.ptr, n_in)
            against_oracle(c.project(), s, k, label="device tensors, pending target")
            # the same with deferred reads
            c.set_defer(True)
            c.set_target_device(dev_g.ptr, n_in, count=False)
            c.set_target_tensors_device(dev_t.ptr, n_in)
            against_oracle(c.project(), s, k, label="device tensors, deferred target")
            c.set_defer(False)
            c.synchronize()
        # deferred, as a batch member beside a host-loaded one
        iters = 3
        pf = tc.params(s, k, iters)
        one = run_frame(s, k, iters, 0.03)
        with imls_icp.ImlsContext(pf) as a, imls_icp.ImlsContext(pf) as b:
            a.set_defer(True)
            a.set_target_device(dev_g.ptr, n_in, count=False)
            a.set_target_tensors_device(dev_t.ptr, n_in)
            a.set_source(s.src, count=False)
            load(b, s, k, iters)
            poses, its, status, traces = imls_icp.register_frames([a, b])
            a.set_defer(False)
            a.synchronize()
        for m in (0, 1):
            assert np.array_equal(poses[m], one["pose"]) and (its[m], status[m]) == (one["iters"], one["status"]), m
            assert same_trace(list(traces[m]), one["trace"]), m
        for it, T in enumerate(tc.frame_poses(one)):
            x, y, n, idx = one["captured"][it]
            against_oracle((x, y, n, idx, np.array(list(one["trace"][it].reject), np.uint64)), s, k, T, iters,
                           label=f"deferred batch member it {it}")
    finally:
        dev_t.free()
        dev_g.free()


# ---- argument checks -------------------------------------------------------------------------------------------------
def test_argument_checks(ctx):
    s = tc.scene_self()
    load(ctx, s, tc.SELF_K)
    for k in (0, 65):
        with pytest.raises(_abi.ImlsError) as e:
            ctx.set_params(tc.params(s, k))
        assert e.value.status == _abi.IMLS_ERR_UNSUPPORTED, k
    for skin in (-0.1, 1.1):
        with pytest.raises(_abi.ImlsError) as e:
            ctx.set_option("tv_skin", skin)
        assert e.value.status == _abi.IMLS_ERR_ARG, skin
    t = np.zeros((len(s.tgt), 5), np.float32)
    assert ctx.lib.imls_set_target_tensors(ctx.ctx, t.ctypes.data_as(C.c_void_p), len(s.tgt), 5) == _abi.IMLS_ERR_ARG
    # the refusals changed nothing: the context still computes the case
    assert ctx.params.tensor_k == tc.SELF_K and ctx.get_option("tv_skin") == 0.03
    against_oracle(ctx.project(), s, tc.SELF_K, label="after the refusals")
