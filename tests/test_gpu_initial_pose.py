"""imls_set_initial_pose: a registration that starts its loop at rPose = pose instead of I (the
predicted pose of a scan in a fixed map frame; scan-to-model odometry).

Only the frame-init kernels change, so: an identity start is the plain call bit for bit; from any
other start the loop is the reference's (laser_odometry.cpp:478-660) and is checked against its
restatement on the CPU oracle's step functions (tests/model_restatement.py, first pinned to
oc.register_frame from I) with the project's tolerances (tests/test_gpu_stream.py: rPose within 1e-6
for LS, 1e-5 through RANSAC→DRPM; iteration counts and statuses equal); every traversal mode gives the
same bits; each member of an imls_register_frames batch starts from its own context's pose and
equals that frame registered alone, bit for bit.  Fixtures: the golden pairs (≤ 2000 source points)."""
import pathlib

import numpy as np
import pytest

import model_restatement as mr
import oracle_ctypes as oc
from planetary_lidar_odometry_amd import _abi, config, imls_icp

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
NAMES = ("vlp16_pair", "planetary_pair")


def _golden(name):
    g = dict(np.load(GOLDEN / f"{name}.npz"))
    return g["src"], g["tgt"], g["frame_pose"]


def _rows(soa6):
    return np.ascontiguousarray(np.asarray(soa6, np.float32).T)


def _params(method):
    p = config.params_from_config(config.load())        # shipped: RANSAC → DRPM, 30 iterations
    p.solve_method = method
    return p


METHODS = [(_abi.IMLS_SOLVE_LS, 1e-6), (_abi.IMLS_SOLVE_RANSAC, 1e-5)]


def _starts(true_pose):
    """(close to the true pose, 0.3 m / 2° off it)"""
    near = mr.make_pose(yaw=2e-4, t=(0.004, -0.003, 0.001)) @ true_pose
    far = mr.make_pose(yaw=np.deg2rad(2.0), t=(0.3, 0.0, 0.0)) @ true_pose
    return near, far


def _trace_equal(a, b):
    return (list(a.delta) == list(b.delta) and list(a.pose) == list(b.pose) and list(a.reject) == list(b.reject)
            and a.n_valid == b.n_valid and a.n_kept == b.n_kept)


def _same_bits(a, b, key=None):
    assert (a["iters"], a["status"]) == (b["iters"], b["status"]), key
    assert np.array_equal(a["pose"], b["pose"]), (key, np.abs(a["pose"] - b["pose"]).max())
    assert len(a["trace"]) == len(b["trace"]) and all(_trace_equal(x, y) for x, y in zip(a["trace"], b["trace"])), key


@pytest.mark.parametrize("method,_tol", METHODS)
def test_restatement_is_the_oracle_from_identity(method, _tol):
    """No GPU: the restated loop started at I is oc.register_frame bit for bit (pose, iterations,
    status, trace, rand() state) — pinned before it is used from other starts."""
    for name in NAMES:
        src, tgt, _ = _golden(name)
        mr.assert_pinned_to_oracle(src, tgt, _params(method))


@pytest.mark.gpu
@pytest.mark.parametrize("method,_tol", METHODS)
def test_identity_start_is_the_plain_call(method, _tol):
    src, tgt, _ = _golden("vlp16_pair")
    p = _params(method)
    with imls_icp.ImlsContext(p) as c:
        c.set_target(_rows(tgt))
        c.set_source(_rows(src))
        plain = c.register_frame()
        c.seed_rng(p.ransac_seed)
        c.set_initial_pose(np.eye(4))
        _same_bits(c.register_frame(), plain, "identity")
        c.set_initial_pose(mr.make_pose(yaw=0.01, t=(0.2, 0, 0)))
        moved = c.register_frame()
        assert not np.array_equal(moved["trace"][0].pose, plain["trace"][0].pose)
        c.seed_rng(p.ransac_seed)
        c.set_initial_pose(None)                         # None restores identity
        _same_bits(c.register_frame(), plain, "restored")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("method,tol", METHODS)
def test_starts_match_the_restatement(name, method, tol):
    """Two frames in a row on one context (near start, then far start), the RANSAC rand() stream
    carried from the first into the second on both sides."""
    src, tgt, true_pose = _golden(name)
    p = _params(method)
    rs = oc.rand_state(p.ransac_seed)
    want_plain = mr.register_from(src, tgt, p, rand_state=oc.rand_state(p.ransac_seed))
    want = [mr.register_from(src, tgt, p, init=s, rand_state=rs) for s in _starts(true_pose)]
    # the near start needs fewer iterations than the start at I; the far one still converges
    assert want[0]["iters"] < want_plain["iters"]
    assert want[1]["status"] == _abi.IMLS_FRAME_CONVERGED
    with imls_icp.ImlsContext(p) as c:
        c.set_target(_rows(tgt))
        c.set_source(_rows(src))
        for s, w in zip(_starts(true_pose), want):
            c.set_initial_pose(s)
            got = c.register_frame()
            err = np.abs(got["pose"] - w["pose"]).max()
            print(f"{name} method {method}: iters {got['iters']}/{w['iters']} status {got['status']}/{w['status']} |Δpose| {err:.3e}")
            assert (got["iters"], got["status"]) == (w["iters"], w["status"])
            assert err < tol, err
            for tg, tw in zip(got["trace"], w["trace"]):
                assert tg.n_valid == tw["n_valid"] and list(tg.reject) == tw["reject"]
                assert np.abs(np.array(tg.pose).reshape(4, 4) - tw["pose"]).max() < tol


@pytest.mark.gpu
def test_too_few_at_iteration_zero_keeps_the_initial_pose():
    src, tgt, true_pose = _golden("vlp16_pair")
    p = _params(_abi.IMLS_SOLVE_LS)
    init = _starts(true_pose)[1]
    with imls_icp.ImlsContext(p) as c:
        c.set_target(_rows(tgt))
        c.set_source(_rows(src)[: p.correspond_number - 1])
        c.set_initial_pose(init)
        r = c.register_frame()
    assert (r["iters"], r["status"]) == (0, _abi.IMLS_FRAME_TOO_FEW)
    assert np.array_equal(r["pose"], init)


@pytest.mark.gpu
def test_traversal_modes_give_equal_bits():
    src, tgt, true_pose = _golden("vlp16_pair")
    p = _params(_abi.IMLS_SOLVE_LS)
    init = _starts(true_pose)[1]
    out = []
    for mode in (_abi.IMLS_TRAVERSAL_PACKETS, _abi.IMLS_TRAVERSAL_WAVE_PER_QUERY, _abi.IMLS_TRAVERSAL_LANE):
        with imls_icp.ImlsContext(p) as c:
            c.set_option("traversal", mode)
            c.set_target(_rows(tgt))
            c.set_source(_rows(src))
            c.set_initial_pose(init)
            out.append(c.register_frame())
    assert out[0]["iters"] > 1
    _same_bits(out[1], out[0], "wave per query")
    _same_bits(out[2], out[0], "lane")


@pytest.mark.gpu
@pytest.mark.parametrize("method,_tol", METHODS)
def test_batch_members_start_from_their_own_pose(method, _tol):
    """Three contexts of different sizes and different initial poses through register_frames: each
    bit-equal to that frame registered alone on a fresh context."""
    p = _params(method)
    src, tgt, true_pose = _golden("vlp16_pair")
    src2, tgt2, true2 = _golden("planetary_pair")
    frames = [(_rows(src), _rows(tgt), _starts(true_pose)[1]),
              (_rows(src2), _rows(tgt2), _starts(true2)[0]),
              (_rows(src)[:1100], _rows(tgt), None)]
    alone = []
    for s, t, init in frames:
        with imls_icp.ImlsContext(p) as c:
            c.set_target(t)
            c.set_source(s)
            c.set_initial_pose(init)
            alone.append(c.register_frame())
    ctxs = [imls_icp.ImlsContext(p) for _ in frames]
    try:
        for c, (s, t, init) in zip(ctxs, frames):
            c.set_target(t)
            c.set_source(s)
            c.set_initial_pose(init)
        poses, iters, status, traces = imls_icp.register_frames(ctxs)
    finally:
        for c in ctxs:
            c.close()
    for k, r in enumerate(alone):
        _same_bits(dict(pose=poses[k], iters=iters[k], status=status[k], trace=list(traces[k])), r, k)
    assert not np.array_equal(alone[0]["pose"], alone[2]["pose"])


@pytest.mark.gpu
def test_non_finite_pose_is_an_argument_error():
    src, tgt, _ = _golden("vlp16_pair")
    p = _params(_abi.IMLS_SOLVE_LS)
    with imls_icp.ImlsContext(p) as c:
        c.set_target(_rows(tgt))
        c.set_source(_rows(src))
        plain = c.register_frame()
        bad = np.eye(4)
        bad[1, 3] = np.nan
        with pytest.raises(_abi.ImlsError) as e:
            c.set_initial_pose(bad)
        assert e.value.status == _abi.IMLS_ERR_ARG
        bad[1, 3] = np.inf
        with pytest.raises(_abi.ImlsError):
            c.set_initial_pose(bad)
        _same_bits(c.register_frame(), plain, "unchanged after the refused poses")
