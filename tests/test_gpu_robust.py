"""GPU: the robust M-estimator solve (IMLS_SOLVE_ROBUST; csrc/solve_robust.hip) against its numpy
restatement (tests/robust_np.py: QR on √w-scaled rows per step, where the device reduces the weighted
normal equations) on the cases of tests/robust_cases.py, whose premises tests/test_robust_cases.py
proves on the CPU.

Bound: |Δ − Δ_np| < 1e-6, the project's POSE_TOL of every LS-family solve; the ok flags, iteration
counts, statuses and every trace n_valid equal.  Alone against batched and pipelined against
unpipelined: bit for bit.  Pose info: the weighted-LS bounds of tests/test_gpu_pose_info.py, plus — for
K > 1 — what the conditioning of the 6×6 solve allows the weights to move (check_robust_report)."""
import functools

import numpy as np
import pytest

import oracle_ctypes as oc
import pose_info_np as pin
import robust_cases as rc
import robust_np as rnp
from planetary_lidar_odometry_amd import _abi, config, imls_icp, synth
from test_gpu_frames import _batched, _single, _trace_equal
from test_gpu_ls_conditioning import corridor, targets
from test_gpu_pose_info import check_spectrum

pytestmark = pytest.mark.gpu
POSE_TOL = rc.POSE_TOL


@pytest.fixture(scope="module")
def ctx():
    with imls_icp.ImlsContext(rc.robust_params(), device=0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def rows_of(n):
    return rc.outlier_set(n)


def _solve(ctx, rows, loss, c, K, weights=None):
    p = rc.robust_params(loss, c, K)
    ctx.set_params(p)
    ok, D = ctx.solve_correspondences(_abi.IMLS_SOLVE_ROBUST, *rows, weights)
    okr, Dr = rnp.solve_rows(*rows, p, weights)
    return ok, D, okr, Dr


# ---- stand-alone fp64 rows ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", rc.ROW_SIZES)
def test_rows_against_restatement(ctx, n):
    rows = rows_of(n)
    worst = 0.0
    for loss in rc.LOSSES:
        for c in rc.SCALES:
            for K in rc.ITERATIONS:
                ok, D, okr, Dr = _solve(ctx, rows, loss, c, K)
                err = np.abs(D - Dr).max()
                worst = max(worst, err)
                assert ok == okr and ok and err < POSE_TOL, (loss, c, K, err)
    print(f"n={n}: worst |Δ − Δ_np| {worst:.3e}")


@pytest.mark.parametrize("n", (5, 257, 4097))
def test_rows_with_caller_weights(ctx, n):
    rows, u = rows_of(n), rc.caller_weights(n)
    for loss in rc.LOSSES:
        ok, D, okr, Dr = _solve(ctx, rows, loss, 0.1, 5, u)
        assert ok == okr and ok and np.abs(D - Dr).max() < POSE_TOL, loss
    if n >= 6:                                                # the weights are read: same loss, with and without
        _, Dw, _, _ = _solve(ctx, rows, "huber", 0.1, 5, u)
        _, D1, _, _ = _solve(ctx, rows, "huber", 0.1, 5)
        assert np.abs(Dw - D1).max() > 1e-9


@pytest.mark.parametrize("positive", (1, 4, 5, 7))
def test_zero_caller_weights_cap_the_rank(ctx, positive):
    """Rows of weight exactly 0 add nothing to H: with fewer than 6 rows of weight > 0 the rank is their
    count, as for the QR of the √w-scaled rows (whose zero rows are zero).  300 rows: two slabs."""
    rows = rows_of(300)
    u = np.zeros(300)
    u[np.linspace(3, 290, positive).astype(int)] = rc.caller_weights(positive)
    for loss in rc.LOSSES:
        ok, D, okr, Dr = _solve(ctx, rows, loss, 0.1, 5, u)
        assert ok and okr and np.abs(D - Dr).max() < POSE_TOL, (loss, np.abs(D - Dr).max())


def test_no_rows_fail(ctx):
    z = np.zeros((0, 3))
    ok, _, okr, _ = _solve(ctx, (z, z, z), "huber", 0.1, 5)
    assert not ok and not okr


def test_rank_deficient_corridor(ctx):
    s, nrm = corridor(4000, 0.0, 6)
    rows = (s, targets(s, nrm, 6), nrm)
    for loss in rc.LOSSES:
        ok, D, okr, Dr = _solve(ctx, rows, loss, 0.1, 5)
        assert ok and okr and np.abs(D - Dr).max() < POSE_TOL, loss
        assert D[0, 3] == 0.0                                 # t_x is unobservable: the basic solution


def test_every_residual_below_scale_is_unit_weight_ls(ctx):
    rows = rc.below_scale_set()
    ok, D, okr, Dr = _solve(ctx, rows, "huber", 0.5, 5)
    okw, Dw = ctx.solve_correspondences(_abi.IMLS_SOLVE_WEIGHTED_LS, *rows)
    assert ok and okw and np.abs(D - Dw).max() < 1e-12
    assert np.abs(D - Dr).max() < POSE_TOL


# ---- float rows through project() + solve() ----------------------------------------------------------
@pytest.mark.parametrize("n", rc.PROJECT_SIZES)
def test_projected_float_rows(ctx, n):
    ctx.set_params(rc.robust_params())
    ctx.set_target(rc.planes_map())
    ctx.set_source(rc.planes_source(n))
    x, y, nr, idx, _ = ctx.project(np.eye(4))
    assert len(idx) == n
    for loss, c, K in [(loss, 0.1, 5) for loss in rc.LOSSES] + [("huber", 0.5, 1), ("cauchy", 0.1, 32)]:
        p = rc.robust_params(loss, c, K)
        ctx.set_params(p)
        ctx.project(np.eye(4))
        ok, D = ctx.solve()
        okr, Dr = rnp.solve_rows(x, y, nr, p)
        assert ok and okr and np.abs(D - Dr).max() < POSE_TOL, (loss, c, K, np.abs(D - Dr).max())


# ---- register_frame against the restated loop --------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.FRAMES))
def test_register_frame(ctx, name):
    build, c, _ = rc.FRAMES[name]
    src, tgt = (rc.rows6(v) for v in build())
    p = rc.robust_params(scale=c, iters=rc.FRAME_ITERS)
    ctx.set_params(p)
    ctx.set_target(tgt)
    ctx.set_source(src)
    r = ctx.register_frame()
    ref = rnp.register_from(np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T), p)
    assert (r["iters"], r["status"]) == (ref["iters"], ref["status"])
    assert [t.n_valid for t in r["trace"]] == [t["n_valid"] for t in ref["trace"]]
    assert all(t.n_kept == t.n_valid for t in r["trace"])
    err = np.abs(r["pose"] - ref["pose"]).max()
    print(f"{name}: n_valid {[t.n_valid for t in r['trace']]} |pose − pose_np| {err:.3e}")
    assert err < POSE_TOL


# ---- alone against batched ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_frames():
    pair = synth.make_pairs(1, "vlp16", map_scans=1, scene_seed=5, traj_seed=2005, noise_seed=1005)[0]
    return [(synth.fps_subsample(pair.source, 1500, seed=1), pair.target),     # one block
            (pair.source, pair.target),                                        # > 4096 rows: the grid chain
            (pair.source[:4], pair.target)]                                    # 4 < correspond_number rows: TOO_FEW


@pytest.mark.parametrize("loss", rc.LOSSES)
def test_alone_equals_batched(mixed_frames, loss):
    p = rc.robust_params(loss, iters=4)
    ref = _single(p, mixed_frames)
    poses, iters, status, traces = _batched(p, mixed_frames)
    for k, r in enumerate(ref):
        assert np.array_equal(r["pose"], poses[k]), (k, np.abs(r["pose"] - poses[k]).max())
        assert (r["iters"], r["status"]) == (iters[k], status[k]), k
        assert len(r["trace"]) == len(traces[k]) and all(_trace_equal(a, b) for a, b in zip(r["trace"], traces[k])), k
    assert ref[2]["status"] == _abi.IMLS_FRAME_TOO_FEW and ref[0]["iters"] > 0
    assert max(t.n_valid for t in ref[1]["trace"]) > 4096 >= max(t.n_valid for t in ref[0]["trace"])


def test_alone_equals_imls_batch(mixed_frames):
    p = rc.robust_params(iters=4)
    ref = _single(p, mixed_frames)
    with imls_icp.ImlsBatch(p, streams=2) as b:
        poses, iters, status = b.register(mixed_frames)
    for k, r in enumerate(ref):
        assert np.array_equal(r["pose"], poses[k]) and (r["iters"], r["status"]) == (iters[k], status[k]), k


# ---- LaserOdometry -----------------------------------------------------------------------------------
def test_laser_odometry_pipelined_equals_unpipelined():
    sm, scene = synth.vlp16(), synth.make_scene(0)
    poses = synth.trajectory(8, 2000)
    scans = [synth.scan(scene, sm, poses[5 + k], seed=3000 + k) for k in range(3)]
    frames = [(s, synth.fps_subsample(s, 1500, seed=k)) for k, s in enumerate(scans)]
    p = rc.robust_params()
    p.max_queue_size = 1
    out = {}
    for pipelined in (False, True):
        with imls_icp.LaserOdometry(p, device=0, pipelined=pipelined) as lo:
            assert lo.pipelined == pipelined
            for filtered, flat in frames:
                lo.process(filtered, flat)
            out[pipelined] = list(lo.results)
    assert len(out[False]) == len(out[True]) == 2
    for (_, p0, i0, s0), (_, p1, i1, s1) in zip(out[False], out[True]):
        assert (i0, s0) == (i1, s1) and i0 > 0 and np.array_equal(p0, p1)


# ---- pose info ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def info_ctx():
    c = imls_icp.ImlsContext(rc.robust_params())
    c.capture_pose_info(True)
    yield c
    c.close()


def check_robust_report(info, rows, p, weights, what):
    """The device's report against robust_np.restate_info on the same rows: every row, the weights
    u·ψ(a·x^{K−1} − b) of the last 6×6 system.

    Bounds.  With K = 1 both sides take the weights under x⁰ = 0: the same bits per term, so every sum
    is held to the weighted-LS bound of tests/test_gpu_pose_info.py, 2·n·ε·Σ w|term|.  With K > 1 the
    device's x^{K−1} comes from its normal equations and the restatement's from QR; the two differ by
    at most dx = 64·κ₂(H)·ε·‖x‖∞ (the forward error of a Cholesky-type solve of H x = g; QR's is
    smaller).  |ψ'| ≤ 1.04/c for the three losses (Geman-McClure at |r| = c/√5), so a row's weight moves
    by at most dw = u·(2/c)·‖a‖₁·dx, and each sum gets Σ dw·|term| on top of the weighted-LS bound.  dx
    is ~1e-12 here; taking the weights under another vector (x^K, x^{K−2}, a stale slot) moves them by
    (1/c)·|a·Δx| with |Δx| ≥ 1e-7, orders of magnitude past it."""
    a, b = pin.rows_ab(*rows)
    n = len(b)
    ref = rnp.restate_info(*rows, p, weights)
    u = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    K, c = p.robust_iterations, p.robust_scale
    dx = 0.0 if K == 1 else 64 * np.linalg.cond(ref["hessian"]) * pin.EPS * np.abs(ref["x_prev"]).max()
    dw = u * (2 / c) * np.abs(a).sum(1) * dx
    eps_n = 2 * n * pin.EPS
    assert info["flags"] & _abi.IMLS_INFO_VALID and info["n_rows"] == n, what
    assert np.abs(info["x"] - ref["x"]).max() <= 1e-6, what
    bound_h = np.einsum("i,ir,ic->rc", dw, np.abs(a), np.abs(a)) + eps_n * ref["abs_hessian"]
    bound_g = np.einsum("i,ir,i->r", dw, np.abs(a), np.abs(b)) + eps_n * ref["abs_gradient"]
    err_h, err_g = np.abs(info["hessian"] - ref["hessian"]), np.abs(info["gradient"] - ref["gradient"])
    print(f"{what}: dx {dx:.2e}  hessian err/bound {np.max(err_h / bound_h):.3g}  gradient {np.max(err_g / bound_g):.3g}")
    assert (err_h <= bound_h).all() and (err_g <= bound_g).all(), what
    assert abs(info["btb"] - ref["btb"]) <= (dw * b * b).sum() + eps_n * ref["btb"], what
    assert abs(info["weight_sum"] - ref["weight_sum"]) <= dw.sum() + eps_n * ref["weight_sum"], what
    res = pin.dot_seq(a, info["x"]) - b                       # the residual under the DEVICE's x
    rss = float(((ref["weights"] * res) * res).sum())
    assert abs(info["rss"] - rss) <= (dw * res * res).sum() + eps_n * rss, (what, info["rss"], rss)
    check_spectrum(info, what)
    assert info["solve_method"] == _abi.IMLS_SOLVE_ROBUST and not info["drpm_probability"].any()


@pytest.mark.parametrize("n", (257, 4097))
@pytest.mark.parametrize("loss", rc.LOSSES)
def test_pose_info_of_caller_rows(info_ctx, n, loss):
    """K = 2 is the case that tells the vectors apart: x¹ lies ~2e-3 from x² and ~4e-2 from x⁰."""
    rows, u = rows_of(n), rc.caller_weights(n)
    for K, weights in ((1, None), (2, None), (2, u), (5, u)):
        p = rc.robust_params(loss, 0.1, K)
        info_ctx.set_params(p)
        ok, D = info_ctx.solve_correspondences(_abi.IMLS_SOLVE_ROBUST, *rows, weights)
        info = info_ctx.pose_info()
        assert ok and np.abs(D - oc.delta_from_x(info["x"])).max() <= 1e-14
        assert info["iteration"] == 0
        check_robust_report(info, rows, p, weights, f"{loss} n={n} K={K} {'u' if weights is not None else '1'}")


@pytest.mark.parametrize("name,K", [("vlp16_pair", 2), ("vlp16_pair", 5), ("planetary_pair", 2), ("config-a", 2)])
def test_pose_info_of_a_registration(info_ctx, name, K):
    """The export of the one-block kernel (the golden pairs) and of the grid chain on float rows
    (config A), on the device's own rows of the reported iteration (captured correspondences)."""
    build, c, _ = rc.FRAMES[name]
    src, tgt = (rc.rows6(v) for v in build())
    p = rc.robust_params(scale=c, iterations=K, iters=rc.FRAME_ITERS)
    info_ctx.set_params(p)
    info_ctx.capture_correspondences(True)
    try:
        info_ctx.set_target(tgt)
        info_ctx.set_source(src)
        r = info_ctx.register_frame()
        info = r["info"]
        assert info["iteration"] == r["iters"] - 1 and info["n_rows"] == r["trace"][-1].n_valid
        assert np.abs(np.array(r["trace"][-1].delta).reshape(4, 4) - oc.delta_from_x(info["x"])).max() <= 1e-14
        x, y, nr, _ = info_ctx.captured(info["iteration"])
    finally:
        info_ctx.capture_correspondences(False)
    check_robust_report(info, (x, y, nr), p, None, f"{name} K={K}")


# ---- parameter errors --------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value", [("robust_loss", 3), ("robust_loss", -1), ("robust_iterations", 0),
                                         ("robust_iterations", 33), ("robust_scale", 0.0), ("robust_scale", -0.1),
                                         ("robust_scale", float("nan")), ("robust_scale", float("inf"))])
def test_bad_robust_params(field, value):
    good = rc.robust_params()
    with imls_icp.ImlsContext(good) as c:
        bad = _abi.ImlsParams.from_buffer_copy(good)
        setattr(bad, field, value)
        with pytest.raises(_abi.ImlsError) as e:
            c.set_params(bad)
        assert e.value.status == _abi.IMLS_ERR_ARG
        bad.solve_method = _abi.IMLS_SOLVE_LS                 # the fields are read for Robust only
        c.set_params(bad)
        with pytest.raises(_abi.ImlsError) as e:              # … but a stand-alone robust solve reads them
            c.solve_correspondences(_abi.IMLS_SOLVE_ROBUST, *rows_of(6))
        assert e.value.status == _abi.IMLS_ERR_ARG
        lib = _abi.load_library()
        import ctypes as C
        bad.solve_method = _abi.IMLS_SOLVE_ROBUST
        assert not lib.imls_create(0, C.byref(bad))           # imls_create refuses the same values
