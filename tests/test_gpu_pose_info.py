"""GPU: the pose covariance / degeneracy report (imls_capture_pose_info, imls_pose_info) against its
numpy restatement (tests/pose_info_np.py) on the same rows.

Bounds (ε = 2.2e-16), derived, not measured:
  hessian, gradient, btb, weight_sum   2·n·ε·Σ w|term| per entry — the device and the restatement add
                                       the same n terms (the same bits per term) in different orders;
                                       each order's error is below n·ε·Σ|term|
  n_rows, rank, flags, sign rule       exact
  x                                    the solvers' contract: 1e-6, 1e-5 through DRPM
  Δ of the solve                       1e-14 from oc.delta_from_x(info.x) (the same x, two libm's)
  rss                                  the same form, the restatement evaluated with the device's x
  eigenpairs                           ‖H·u − λ·u‖ ≤ 1e-12·‖H‖_F and ‖U·Uᵀ − I‖ ≤ 1e-13 on the device's H
  covariance                           1e-12·(λ₅ / λ_min kept)·‖Σ‖ from the restatement on the device's H, rss
  drpm_probability                     1e-6 (device erfc, as the 1e-5 DRPM contract)
The premises (trim boundaries well separated, the sentinel's ranks, RANSAC's inliers) are proved on
the CPU in tests/test_pose_info_model.py."""
import numpy as np
import pytest

import model_restatement as mr
import oracle_ctypes as oc
import pose_info_cases as cases
import pose_info_np as pin
from planetary_lidar_odometry_amd import _abi, config, imls_icp
from ransac_cases import config_a_pair, hdl_strided, outlier_set, shipped_params

pytestmark = pytest.mark.gpu
EPS = pin.EPS
V, RD, NODOF, DRAN, DDEG = (_abi.IMLS_INFO_VALID, _abi.IMLS_INFO_RANK_DEFICIENT, _abi.IMLS_INFO_NO_DOF,
                            _abi.IMLS_INFO_DRPM_RAN, _abi.IMLS_INFO_DRPM_DEGENERATE)


def soa_to_rows(soa6):
    return np.ascontiguousarray(np.asarray(soa6, np.float32).T)


def params(solve="LS", iters=8, final="DRPM", **kw):
    p = shipped_params(iters=iters, final=final)
    p.solve_method = {"LS": _abi.IMLS_SOLVE_LS, "WLS": _abi.IMLS_SOLVE_WEIGHTED_LS, "RANSAC": _abi.IMLS_SOLVE_RANSAC}[solve]
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.fixture(scope="module")
def ctx():
    c = imls_icp.ImlsContext(params())
    c.capture_pose_info(True)
    yield c
    c.close()


def check_report(info, ref, rows, x_tol, what=""):
    """info: the device's report; ref: the restatement on the same rows (members = its kept rows);
    rows: (a, b, w) of every row, for the residual under the device's x."""
    n = ref["n_rows"]
    assert info["flags"] & V, what
    assert info["n_rows"] == n, (what, info["n_rows"], n)
    for key, absk in (("hessian", "abs_hessian"), ("gradient", "abs_gradient")):
        err, bound = np.abs(info[key] - ref[key]), 2 * n * EPS * ref[absk]
        print(f"{what} {key}: max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
        assert (err <= bound).all(), (what, key)
    assert abs(info["btb"] - ref["btb"]) <= 2 * n * EPS * ref["btb"], what
    assert abs(info["weight_sum"] - ref["weight_sum"]) <= 2 * n * EPS * ref["weight_sum"], what
    print(f"{what} |x − restatement| {np.abs(info['x'] - ref['x']).max():.3g}")
    assert np.abs(info["x"] - ref["x"]).max() <= x_tol, what
    a, b, w = rows
    m = ref["members"]
    rss = pin.sums(a[m], b[m], None if w is None else w[m], info["x"])["rss"]
    assert abs(info["rss"] - rss) <= 2 * n * EPS * rss, (what, info["rss"], rss)
    check_spectrum(info, what)


def check_spectrum(info, what=""):
    """Eigenpairs, order, sign, rank, sigma2 and covariance against the device's own H and rss."""
    H, ev, U = info["hessian"], info["eigenvalues"], info["eigenvectors"]
    assert np.array_equal(H, H.T) and np.all(np.diff(ev) >= 0), what
    fro = np.linalg.norm(H)
    for k in range(6):
        assert np.linalg.norm(H @ U[k] - ev[k] * U[k]) <= 1e-12 * fro, (what, k)
    assert np.abs(U @ U.T - np.eye(6)).max() <= 1e-13, what
    assert np.array_equal(pin.pin_sign(U), U), what
    rank = int((ev > pin.RANK_RELTOL * ev[5]).sum())
    assert info["rank"] == rank, what
    n = info["n_rows"]
    want = pin.spectrum(H, info["rss"], n)
    base = V | RD | NODOF
    assert info["flags"] & base == want["flags"] & base, (what, info["flags"], want["flags"])
    if n <= rank:
        assert info["sigma2"] == 0 and not info["covariance"].any(), what
        return
    assert abs(info["sigma2"] - info["rss"] / (n - rank)) <= 4 * EPS * info["sigma2"], what
    kept = ev[ev > pin.RANK_RELTOL * ev[5]]
    bound = 1e-12 * (ev[5] / kept.min()) * np.linalg.norm(want["covariance"])
    assert np.abs(info["covariance"] - want["covariance"]).max() <= bound, what


# ---- 1. stand-alone solves --------------------------------------------------------------------------
def _kept_subset(info, s, d, n, ref):
    """N = 6 at t = 0.25 (proved on the CPU): the first solve fits its six rows exactly, so the order of
    the |r₁| is rounding noise and the kept rows are not determined.  The report must still be the
    second solve over SOME n_rows of the rows: the subset whose sums it carries, found by search."""
    import itertools
    N = len(s)
    assert N <= 7 and info["n_rows"] == ref["n_rows"]
    for m in itertools.combinations(range(N), ref["n_rows"]):
        cand = pin.restate_ls_members(s, d, n, m)
        if (np.abs(info["hessian"] - cand["hessian"]) <= 2 * cand["n_rows"] * EPS * cand["abs_hessian"]).all():
            return cand
    raise AssertionError("the report's hessian is the sum over no subset of the rows")


@pytest.mark.parametrize("N", cases.SIZES)
def test_solve_correspondences_ls_wls_drpm(ctx, N):
    s, d, n = cases.solve_rows(N)
    a, b = pin.rows_ab(s, d, n)
    w = np.random.default_rng(N).uniform(0.2, 1.0, N)
    for t in cases.THRESHOLDS:
        p = params("LS", ls_threshold=t)
        ctx.set_params(p)
        ok, D = ctx.solve_correspondences(_abi.IMLS_SOLVE_LS, s, d, n)
        info = ctx.pose_info()
        assert ok and np.abs(D - oc.delta_from_x(info["x"])).max() <= 1e-14
        ref = pin.restate_ls(s, d, n, t)
        if ref["trimmed"] and ref["gap_scale"] < 1e-9:
            ref = _kept_subset(info, s, d, n, ref)
        check_report(info, ref, (a, b, None), 1e-6, f"LS N={N} t={t}")
        assert info["iteration"] == 0 and info["solve_method"] == _abi.IMLS_SOLVE_LS and not info["drpm_probability"].any()
        if N == 6:
            assert info["flags"] & NODOF and info["sigma2"] == 0 and not info["covariance"].any()
    p = params("LS")
    ctx.set_params(p)
    ok, D = ctx.solve_correspondences(_abi.IMLS_SOLVE_WEIGHTED_LS, s, d, n, w)
    info = ctx.pose_info()
    assert ok and np.abs(D - oc.delta_from_x(info["x"])).max() <= 1e-14
    check_report(info, pin.restate_wls(s, d, n, w), (a, b, w), 1e-6, f"WLS N={N}")
    ok, D = ctx.solve_correspondences(_abi.IMLS_SOLVE_DRPM, s, d, n, w)
    info = ctx.pose_info()
    ref = pin.restate_drpm(s, d, n, w, p)
    assert ok and np.abs(D - oc.delta_from_x(info["x"])).max() <= 1e-14
    check_report(info, ref, (a, b, w), 1e-5, f"DRPM N={N}")
    assert info["flags"] & DRAN and bool(info["flags"] & DDEG) == bool(ref["flags"] & DDEG)
    assert np.abs(info["drpm_probability"] - ref["drpm_probability"]).max() <= 1e-6
    assert info["solve_method"] == _abi.IMLS_SOLVE_DRPM


@pytest.mark.parametrize("N", [4000, 16385])
@pytest.mark.parametrize("final", ["LS", "WLS", "DRPM"])
def test_ransac_finals_on_outlier_set(ctx, N, final):
    """Both sides of the inlier-compaction switches.  The inliers are those of the restated hypothesis
    loop (pinned to the oracle on the CPU): n_rows is their count for the weighted finals and the trim
    of it for LS, and the sums run over exactly those rows with the weights w / Σw."""
    s, d, n = outlier_set(N, 0.02, 7)
    p = shipped_params(final=final)
    ctx.set_params(p)
    ctx.seed_rng(p.ransac_seed)
    ok, D = ctx.solve_correspondences(_abi.IMLS_SOLVE_RANSAC, s, d, n)
    info = ctx.pose_info()
    ref = pin.restate_ransac(s, d, n, p)
    m = len(ref["inliers"])
    lo, hi = pin.trim_ranks(m, p.ransac_ls_threshold)
    assert ok and info["n_rows"] == (hi - lo + 1 if final == "LS" else m)
    assert np.abs(D - oc.delta_from_x(info["x"])).max() <= 1e-14
    a, b = pin.rows_ab(s, d, n)
    w = None
    if final != "LS":
        inl, wi, _ = pin.ransac_inliers(s, d, n, p)
        w = np.zeros(N)
        w[inl] = wi
    check_report(info, ref, (a, b, w), 1e-5 if final == "DRPM" else 1e-6, f"RANSAC→{final} N={N}")
    assert info["solve_method"] == _abi.IMLS_SOLVE_RANSAC and info["final_method"] == p.ransac_final_method
    assert bool(info["flags"] & DRAN) == (final == "DRPM")
    if final == "DRPM":
        assert np.abs(info["drpm_probability"] - ref["drpm_probability"]).max() <= 1e-6


# ---- 2. the selection's sentinel --------------------------------------------------------------------
def test_trim_membership_sentinel(ctx):
    p = params("LS", ls_threshold=cases.SENTINEL_T)
    ctx.set_params(p)
    got = {}
    for side in ("in", "out"):
        s, d, n = cases.sentinel_rows(side)
        a, b = pin.rows_ab(s, d, n)
        ok, _ = ctx.solve_correspondences(_abi.IMLS_SOLVE_LS, s, d, n)
        info = ctx.pose_info()
        ref = pin.restate_ls(s, d, n, cases.SENTINEL_T)
        assert ok and (cases.SENTINEL_ROW in ref["members"]) == (side == "in")
        check_report(info, ref, (a, b, None), 1e-6, f"sentinel {side}")
        got[side] = info
    assert got["in"]["n_rows"] == got["out"]["n_rows"]
    assert np.abs(got["in"]["hessian"] - got["out"]["hessian"]).max() > 0.1   # one row's a·aᵀ (‖n‖ = 1)


# ---- 3. registrations -------------------------------------------------------------------------------
def _register(ctx, p, src, tgt, capture=True):
    ctx.set_params(p)
    ctx.seed_rng(p.ransac_seed)
    ctx.capture_correspondences(capture)
    ctx.set_target(tgt)
    ctx.set_source(src)
    return ctx.register_frame()


@pytest.mark.parametrize("name", ["vlp16_pair", "planetary_pair"])
@pytest.mark.parametrize("solve", ["LS", "WLS"])
def test_register_frame_report(ctx, name, solve):
    g = cases.golden(name)
    p = params(solve)
    r = _register(ctx, p, soa_to_rows(g["src"]), soa_to_rows(g["tgt"]))
    ctx.capture_correspondences(False)
    info = r["info"]
    it = info["iteration"]
    assert r["iters"] >= 2 and it == r["iters"] - 1 and info["status"] == r["status"]
    x, y, n, _ = ctx.captured(it)
    a, b = pin.rows_ab(x, y, n)
    ref = pin.restate_ls(x, y, n, p.ls_threshold) if solve == "LS" else pin.restate_wls(x, y, n)
    check_report(info, ref, (a, b, None), 1e-6, f"{name} {solve}")
    assert np.abs(np.array(r["trace"][it].delta).reshape(4, 4) - oc.delta_from_x(info["x"])).max() <= 1e-14
    assert r["trace"][it].n_valid == len(b)
    if solve == "LS":
        assert info["n_rows"] == r["trace"][it].n_kept


@pytest.mark.parametrize("name", ["vlp16_pair", "planetary_pair"])
def test_register_frame_ransac_drpm_report(ctx, name):
    """The shipped RANSAC → DRPM as a registration of several iterations: the report is the LAST
    iteration's, against the restatement on that iteration's captured rows under the rand() state the
    iteration began with (read after the same frame run for one iteration fewer), and against the
    stand-alone solve on those rows.  When the frame converges before `iterations`, the inlier rows,
    their count and Σw must have survived the skipped iterations."""
    g = cases.golden(name)
    src, tgt = soa_to_rows(g["src"]), soa_to_rows(g["tgt"])
    p = shipped_params(iters=8, final="DRPM")
    r = _register(ctx, p, src, tgt)
    ctx.capture_correspondences(False)
    info = r["info"]
    m = r["iters"]
    it = info["iteration"]
    print(f"{name}: iters {m} status {r['status']}")
    assert m >= 2 and it == m - 1 and info["status"] == r["status"] and info["flags"] & DRAN
    x, y, n, _ = ctx.captured(it)
    s, d, nn = (v.astype(np.float64) for v in (x, y, n))
    assert r["trace"][it].n_valid == len(s)
    short = _register(ctx, shipped_params(iters=m - 1, final="DRPM"), src, tgt, capture=False)
    assert short["iters"] == m - 1
    for t, u in zip(short["trace"], r["trace"]):
        assert np.array_equal(np.array(t.delta), np.array(u.delta))
    before = ctx.rng_state().copy()                       # the stream as iteration m − 1 found it
    ctx.set_params(p)
    ref = pin.restate_ransac(s, d, nn, p, state=before.copy())
    inl, wi, _ = pin.ransac_inliers(s, d, nn, p, state=before.copy())
    w = np.zeros(len(s))
    w[inl] = wi
    check_report(info, ref, (*pin.rows_ab(s, d, nn), w), 1e-5, f"{name} RANSAC→DRPM")
    assert np.abs(info["drpm_probability"] - ref["drpm_probability"]).max() <= 1e-6
    assert np.abs(np.array(r["trace"][it].delta).reshape(4, 4) - oc.delta_from_x(info["x"])).max() <= 1e-14
    ctx.set_rng_state(before)
    ok, D = ctx.solve_correspondences(_abi.IMLS_SOLVE_RANSAC, s, d, nn)
    alone = ctx.pose_info()
    assert ok and alone["n_rows"] == info["n_rows"] and alone["flags"] == info["flags"]
    assert np.abs(alone["x"] - info["x"]).max() <= 1e-5
    assert (np.abs(alone["hessian"] - info["hessian"]) <= 2 * info["n_rows"] * EPS * ref["abs_hessian"]).all()


def test_register_frame_above_the_small_solve_and_too_few(ctx):
    """A frame of more than 4096 valid rows takes the grid chain (k_solve_final's export), the golden
    frames above k_solve_small's; a frame below correspond_number reports nothing."""
    src, tgt = config_a_pair()
    p = params("LS", iters=3)
    r = _register(ctx, p, src, tgt)
    ctx.capture_correspondences(False)
    info = r["info"]
    it = info["iteration"]
    x, y, n, _ = ctx.captured(it)
    assert len(x) > 4096 and it == r["iters"] - 1
    ref = pin.restate_ls(x, y, n, p.ls_threshold)
    assert ref["gap"] >= 1e-9
    check_report(info, ref, (*pin.rows_ab(x, y, n), None), 1e-6, "config A LS")
    assert info["n_rows"] == r["trace"][it].n_kept
    p = params("LS", iters=3, correspond_number=1 << 20)
    r = _register(ctx, p, src, tgt, capture=False)
    assert r["status"] == _abi.IMLS_FRAME_TOO_FEW and r["iters"] == 0
    info = r["info"]
    assert info["flags"] == 0 and info["n_rows"] == 0 and not info["hessian"].any() and not info["covariance"].any()


# ---- 4. nothing else moves --------------------------------------------------------------------------
@pytest.mark.parametrize("solve", ["LS", "RANSAC"])
def test_capture_changes_nothing_else(solve):
    g = cases.golden("vlp16_pair")
    p = params(solve, iters=6)
    out = {}
    for on in (False, True):
        with imls_icp.ImlsContext(p) as c:
            c.capture_pose_info(on)
            c.enable_timing(True)
            c.set_target(soa_to_rows(g["tgt"]))
            c.set_source(soa_to_rows(g["src"]))
            r = c.register_frame()
            launches = c.kernel_timing(13)[1]
            if on:
                assert launches == 1 and r["info"]["flags"] & V
            else:
                assert launches == 0 and "info" not in r
                with pytest.raises(_abi.ImlsError) as e:
                    c.pose_info()
                assert e.value.status == _abi.IMLS_ERR_STATE
            out[on] = (r, c.rng_state().copy())
    (ra, sa), (rb, sb) = out[False], out[True]
    assert np.array_equal(ra["pose"], rb["pose"]) and ra["iters"] == rb["iters"] and ra["status"] == rb["status"]
    assert np.array_equal(sa, sb)
    for t, u in zip(ra["trace"], rb["trace"]):
        assert bytes(t) == bytes(u)


def test_report_needs_a_collected_result():
    g = cases.golden("vlp16_pair")
    with imls_icp.ImlsContext(params("LS", iters=3)) as c:
        c.capture_pose_info(True)
        c.set_target(soa_to_rows(g["tgt"]))
        c.set_source(soa_to_rows(g["src"]))
        c.register_frame_async()
        with pytest.raises(_abi.ImlsError) as e:
            c.pose_info()
        assert e.value.status == _abi.IMLS_ERR_STATE
        c.register_frame_result()
        assert c.pose_info()["flags"] & V
        c.capture_pose_info(False)
        c.register_frame()
        with pytest.raises(_abi.ImlsError):
            c.pose_info()


# ---- 5. batched -------------------------------------------------------------------------------------
@pytest.mark.parametrize("solve", ["LS", "RANSAC"])
def test_batched_reports_equal_the_lone_frames(solve):
    """imls_register_frames over four contexts — a small frame, one above 4096 rows, one that ends
    TOO_FEW, and one above 16,384 valid rows (RANSAC's three-kernel inlier compaction) — each member's
    report bit for bit the lone registration's."""
    g = cases.golden("vlp16_pair")
    big_src, big_tgt = config_a_pair()
    huge_src, huge_tgt = hdl_strided(5)
    far = soa_to_rows(g["src"]).copy()
    far[:, :3] += 500.0                                    # no neighbour within r: TOO_FEW at iteration 0
    frames = [(soa_to_rows(g["src"]), soa_to_rows(g["tgt"])), (big_src, big_tgt), (far, soa_to_rows(g["tgt"])),
              (huge_src, huge_tgt)]
    p = params(solve, iters=3)
    alone = []
    for src, tgt in frames:
        with imls_icp.ImlsContext(p) as c:
            c.capture_pose_info(True)
            c.set_target(tgt)
            c.set_source(src)
            alone.append(c.register_frame())
    ctxs = [imls_icp.ImlsContext(p) for _ in frames]
    assert all(c.last_info is None for c in ctxs)
    try:
        for c, (src, tgt) in zip(ctxs, frames):
            c.capture_pose_info(True)
            c.set_target(tgt)
            c.set_source(src)
        poses, iters, status, _ = imls_icp.register_frames(ctxs)
        for k, (c, r) in enumerate(zip(ctxs, alone)):
            assert np.array_equal(poses[k], r["pose"]) and iters[k] == r["iters"] and status[k] == r["status"]
            info = c.last_info
            for key, v in r["info"].items():
                assert np.array_equal(np.asarray(info[key]), np.asarray(v)), (k, key)
        assert status[2] == _abi.IMLS_FRAME_TOO_FEW and ctxs[2].last_info["flags"] == 0
        assert 4096 < alone[1]["trace"][-1].n_valid <= 16384 < alone[3]["trace"][-1].n_valid
        assert all(ctxs[k].last_info["flags"] & V for k in (0, 1, 3))
    finally:
        for c in ctxs:
            c.close()


# ---- 6. the degenerate plane through the shipped solver ----------------------------------------------
def test_degenerate_plane_report(ctx):
    s, d, n = cases.plane_rows()
    p = shipped_params(final="DRPM")
    ctx.set_params(p)
    ctx.seed_rng(p.ransac_seed)
    ok, _ = ctx.solve_correspondences(_abi.IMLS_SOLVE_RANSAC, s, d, n)
    info = ctx.pose_info()
    assert ok and info["flags"] & DRAN and info["flags"] & DDEG
    assert (np.sort(info["drpm_probability"])[:3] < p.drpm_threshold).all()
    weak = info["eigenvectors"][:3]                        # the three smallest eigenvalues
    print("off-span components", np.linalg.norm(weak[:, [0, 1, 5]], axis=1), "p", info["drpm_probability"])
    assert (np.linalg.norm(weak[:, [0, 1, 5]], axis=1) <= 0.05).all()
    check_spectrum(info, "degenerate plane")


# ---- 7. the driver ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream():
    return mr.vlp16_stream(8)[0]


@pytest.mark.parametrize("mode", ["raw-pipelined", "raw-single", "compensated"])
def test_laser_odometry_pose_covariances(stream, mode):
    p = config.params_from_config(config.load())
    p.solve_method = _abi.IMLS_SOLVE_LS
    p.max_queue_size = 3 if mode == "compensated" else 1
    kw = dict(map_model="compensated") if mode == "compensated" else dict(pipelined=mode == "raw-pipelined")
    runs = {}
    for on in (False, True):
        with imls_icp.LaserOdometry(p, device=0, pose_info=on, **kw) as lo:
            assert lo.pipelined == (mode == "raw-pipelined")
            anchors = []
            for k, (filtered, flat) in enumerate(stream):
                anchors.append(lo.anchor_pose.copy())
                lo.process(filtered, flat, timestamp=str(k))
            assert lo.covariance_gaps == []
            runs[on] = (list(lo.poses), list(lo.results), list(lo.infos), list(lo.pose_covariances), anchors)
    poses, results, infos, covs, anchors = runs[True]
    assert runs[False][2] == [] and len(infos) == len(covs) == len(poses) == 7
    for (_, a), (_, b) in zip(runs[False][0], poses):
        assert np.array_equal(a, b)
    cov, prev = np.zeros((6, 6)), np.eye(4)
    for k, (info, (_, now)) in enumerate(zip(infos, poses)):
        assert info is not None and info["flags"] & V and info["rank"] == 6
        rel = info["covariance"]
        if mode == "compensated":
            A = imls_icp.adjoint(imls_icp.inv_pose(anchors[k + 1]))
            rel = A @ rel @ A.T
        A = imls_icp.adjoint(prev)
        cov = cov + A @ rel @ A.T
        assert np.array_equal(covs[k], cov)
        tr = np.trace(cov)
        assert np.abs(cov - cov.T).max() <= 1e-12 * tr and np.linalg.eigvalsh(0.5 * (cov + cov.T)).min() >= -1e-12 * tr
        prev = now
