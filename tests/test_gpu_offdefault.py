"""GPU parity AWAY from the shipped config.json: every matcher gate, trim rank, RANSAC weight and DRPM
probability at values the rest of the suite never sets (tests/offdefault_cases.py holds the cases;
tests/test_offdefault_cases.py proves on the oracle alone that each one moves the oracle's own result
and populates the branch it is named for).  The device against the oracle through the C ABI, at the
suite's tolerances: masks, reject counters, indices, x, n, n_valid, n_kept, iteration
counts, statuses and the device rand() state exact; y within 1e-5; Δ and poses within 1e-6 (1e-5
with a DRPM final).  Batched runs (imls_register_frames) must equal each frame alone bit for bit.
Each test prints its largest |device − oracle| (MEASURED …) before it asserts.
"""
import numpy as np
import pytest

import offdefault_cases as od
import oracle_ctypes as oc
import ransac_cases as rc
from planetary_lidar_odometry_amd import _abi, imls_icp
from test_gpu_frames import _trace_equal

pytestmark = pytest.mark.gpu
LS, RANSAC = _abi.IMLS_SOLVE_LS, _abi.IMLS_SOLVE_RANSAC


@pytest.fixture(scope="module")
def ctx():
    c = imls_icp.ImlsContext(od.ls_params())
    yield c
    c.close()


@pytest.fixture(params=["auto", "packets", "wave_per_query"])
def traversal(request, ctx):
    ctx.set_option("traversal", {"auto": _abi.IMLS_TRAVERSAL_AUTO, "packets": _abi.IMLS_TRAVERSAL_PACKETS,
                                 "wave_per_query": _abi.IMLS_TRAVERSAL_WAVE_PER_QUERY}[request.param])
    yield request.param
    ctx.set_option("traversal", _abi.IMLS_TRAVERSAL_AUTO)


def _measured(section, label, err, tol):
    print(f"MEASURED section={section} {label} max|dev-oracle|={err:.3e} tol={tol:.0e}")


def _load(ctx, p, src, tgt):
    ctx.set_params(p)
    ctx.seed_rng(p.ransac_seed)
    ctx.set_target(tgt)
    ctx.set_source(src)


def _check_projection(got, want, section, label):
    """Exact mask, counters, x, n; y within Y_TOL.  `want` is the oracle's (x, y, n, idx, rej)."""
    x, y, n, idx, rej = got
    wx, wy, wn, widx, wrej = want
    assert np.array_equal(rej, wrej), (label, list(rej), list(wrej))
    assert np.array_equal(idx, widx), label
    assert np.array_equal(x, wx) and np.array_equal(n, wn), label
    err = float(np.abs(y.astype(np.float64) - wy.astype(np.float64)).max()) if len(idx) else 0.0
    _measured(section, f"{label} rows={len(idx)} y", err, od.Y_TOL)
    assert err <= od.Y_TOL, (label, err)


def _check_frame(r, want, tol, section, label, kept=True, compare_delta=True):
    """register_frame against the oracle: iterations, status, every iteration's n_valid, reject
    counters (and n_kept on the LS path) exact; every Δ and the pose within tol."""
    assert (r["iters"], r["status"]) == (want["iters"], want["status"]), label
    assert len(r["trace"]) == len(want["trace"])
    err = 0.0
    for t, u in zip(r["trace"], want["trace"]):
        assert t.n_valid == u.n_valid and list(t.reject) == list(u.reject), label
        if kept:
            assert t.n_kept == u.n_kept, (label, t.n_kept, u.n_kept)
        err = max(err, float(np.abs(np.array(t.delta) - np.array(u.delta)).max()))
    err = max(err, float(np.abs(r["pose"] - want["pose"]).max()))
    if compare_delta:
        _measured(section, f"{label} n_valid={[int(u.n_valid) for u in want['trace']]} pose", err, tol)
        assert err < tol, (label, err)


def _alone(p, names):
    """Every named frame registered alone in a fresh context (a fresh rand() stream): results with
    the stream's final state."""
    out = []
    for name in names:
        with imls_icp.ImlsContext(p) as c:
            src, tgt = od.frame(name)
            c.set_target(tgt)
            c.set_source(src)
            r = c.register_frame()
            r["rand_state"] = c.rng_state()
            out.append(r)
    return out


def _batched(p, names):
    ctxs = [imls_icp.ImlsContext(p) for _ in names]
    try:
        for c, name in zip(ctxs, names):
            src, tgt = od.frame(name)
            c.set_target(tgt)
            c.set_source(src)
        poses, iters, status, traces = imls_icp.register_frames(ctxs)
        return [dict(pose=poses[k], iters=int(iters[k]), status=int(status[k]), trace=list(traces[k]),
                     rand_state=c.rng_state()) for k, c in enumerate(ctxs)]
    finally:
        for c in ctxs:
            c.close()


def _batch_equals_alone(p, names):
    """imls_register_frames over the named frames: every frame bit-equal to itself alone (pose,
    iterations, status, trace, rand() state).  Returns the batch's results."""
    alone, batch = _alone(p, names), _batched(p, names)
    for k, (a, b) in enumerate(zip(alone, batch)):
        assert np.array_equal(a["pose"], b["pose"]), (names[k], np.abs(a["pose"] - b["pose"]).max())
        assert (a["iters"], a["status"]) == (b["iters"], b["status"]), names[k]
        assert len(a["trace"]) == len(b["trace"]) and all(_trace_equal(t, u) for t, u in zip(a["trace"], b["trace"])), names[k]
        assert np.array_equal(a["rand_state"], b["rand_state"]), names[k]
    return batch


# ================================================================================================
# A. angle gate
# ================================================================================================
_ANGLES = [(m, thr) for m in ("IMLS", "plane_ICP") for thr in od.ANGLE_THRESHOLDS[m]]


@pytest.mark.parametrize("matcher,thr", _ANGLES, ids=[f"{m}-{t:g}" for m, t in _ANGLES])
@pytest.mark.parametrize("name", od.PAIRS)
def test_angle_gate_projection(ctx, name, matcher, thr, traversal):
    """angle_reject at thresholds inside and outside [0°, 180°] (the reference compares the angle
    with any double: ≥ 180 rejects nothing, < 0 every row with a cosine in [−1, 1]), both matchers,
    both poses, the three traversals."""
    g = od.golden(name)
    _load(ctx, od.angle_params(matcher, thr), od.soa_to_rows(g["src"]), od.soa_to_rows(g["tgt"]))
    for k in (0, 1):
        want = od.oracle_projection(name, ("angle", matcher, thr), k)
        _check_projection(ctx.project(g[f"pose{k}"]), want, "A", f"{name} {matcher} thr={thr:g} pose{k} {traversal}")
    want = od.oracle_projection(name, ("angle", matcher, thr), 1)
    assert (len(want[3]), int(want[4][od.REJ_ANGLE])) == od.ANGLE_COUNTS[(name, matcher)][thr]


@pytest.mark.parametrize("thr", od.GATE_EDGE_THRESHOLDS)
def test_angle_gate_exact_branch(ctx, thr, traversal):
    """Cosines within a rounding of ±1, above 1 (NaN angle: passes) and 0/0, at thresholds at and
    beyond both ends of [0°, 180°]: the fp64 branch of angle_reject against the reference's acos."""
    src, tgt = od.gate_edge_scene()
    _load(ctx, od.angle_params("IMLS", thr), od.soa_to_rows(src), od.soa_to_rows(tgt))
    _check_projection(ctx.project(np.eye(4)), od.oracle_gate_edge(thr), "A", f"exact branch thr={thr:g} {traversal}")


@pytest.mark.parametrize("thr", [2.0, 360.0])
def test_angle_gate_frame(ctx, thr):
    p = od.angle_params("IMLS", thr)
    _load(ctx, p, *od.frame("golden"))
    _check_frame(ctx.register_frame(), od.oracle_frame("golden", p), od.POSE_TOL, "A", f"frame thr={thr:g}")


# ================================================================================================
# B. matcher radii and the correspondence gate
# ================================================================================================
@pytest.mark.parametrize("key", [k for k, v in od.PROJECT_CASES.items() if v[1]])
def test_matcher_radii(ctx, key):
    """r_proj, picp_r (with the reference's swapped ‖p−x‖ < r·r gate), picp_r_proj and h > r on the
    [:, ::2] subsample at pose1."""
    g = od.golden("vlp16_pair")
    src = np.ascontiguousarray(g["src"][:, ::od.PROJECT_STEP])
    _load(ctx, od.case_params(key), od.soa_to_rows(src), od.soa_to_rows(g["tgt"]))
    _check_projection(ctx.project(g["pose1"]), od.oracle_projection("vlp16_pair", key, 1, od.PROJECT_STEP), "B", key)


def _gate_params(solver, n):
    p = od.ls_params(3) if solver == "LS" else od.ransac_frame_params(3)
    p.correspond_number = n
    return p


@pytest.mark.parametrize("solver", ["LS", "RANSAC-DRPM"])
@pytest.mark.parametrize("name", ["golden", "full"])
def test_correspond_number_gate(ctx, name, solver):
    """correspond_number = N* (iteration 0's n_valid): the frame runs, the gate is `<`; N* + 1:
    TOO_FEW at iteration 0 with the pose kept.  The one-block solve (golden pair) and the grid chain
    (a full scan); RANSAC has its own gate."""
    tol = od.POSE_TOL if solver == "LS" else od.DRPM_TOL
    n0 = int(od.oracle_frame(name, od.ls_params(3))["trace"][0].n_valid)
    for n in (n0, n0 + 1):
        p = _gate_params(solver, n)
        _load(ctx, p, *od.frame(name))
        r = ctx.register_frame()
        want = od.oracle_frame(name, p)
        _check_frame(r, want, tol, "B", f"gate {name} {solver} correspond_number=N*{'+1' if n > n0 else ''}", kept=solver == "LS")
        assert np.array_equal(ctx.rng_state(), want["rand_state"])
        if n > n0:
            assert (r["iters"], r["status"]) == (0, _abi.IMLS_FRAME_TOO_FEW) and np.array_equal(r["pose"], np.eye(4))
        else:
            assert r["iters"] >= 1 and r["trace"][0].n_valid == n0


@pytest.mark.parametrize("solver", ["LS", "RANSAC-DRPM"])
@pytest.mark.parametrize("lead", ["golden", "full"])
def test_correspond_number_gate_batched(lead, solver):
    """The same gate inside a batch of three: the lead frame sits exactly on the gate, the others
    fall below it."""
    tol = od.POSE_TOL if solver == "LS" else od.DRPM_TOL
    names = [lead, "tiny", "g40"] if lead == "golden" else ["g40", lead, "golden"]
    n0 = int(od.oracle_frame(lead, od.ls_params(3))["trace"][0].n_valid)
    for n in (n0, n0 + 1):
        p = _gate_params(solver, n)
        for name, r in zip(names, _batch_equals_alone(p, names)):
            want = od.oracle_frame(name, p)
            _check_frame(r, want, tol, "B", f"batched gate {name} {solver} n={n}", kept=solver == "LS")
            assert np.array_equal(r["rand_state"], want["rand_state"]), name
            assert (r["status"] == _abi.IMLS_FRAME_TOO_FEW) == (name != lead or n > n0)


# ================================================================================================
# C. trimmed LS ranks
# ================================================================================================
@pytest.mark.parametrize("t", od.TRIMS)
@pytest.mark.parametrize("name", od.PAIRS)
def test_trim_small_solve(ctx, name, t):
    """Route 1, k_solve_small on float rows: project(pose1) + solve(), then register_frame with
    every iteration's n_kept."""
    g = od.golden(name)
    p = od.ls_params(ls_threshold=t)
    _load(ctx, p, od.soa_to_rows(g["src"]), od.soa_to_rows(g["tgt"]))
    ctx.project(g["pose1"])
    ok, D = ctx.solve()
    okr, Dr = oc.solve(LS, *od.golden_rows(name), p)
    err = float(np.abs(D - Dr).max())
    _measured("C", f"solve {name} t={t}", err, od.POSE_TOL)
    assert ok == okr and err < od.POSE_TOL, err
    if name == "vlp16_pair":
        _check_frame(ctx.register_frame(), od.oracle_frame("golden", p), od.POSE_TOL, "C", f"frame golden t={t}")


@pytest.mark.parametrize("t", od.TRIMS)
@pytest.mark.parametrize("rows", ["golden", "spread"])
def test_trim_grid_chain_double_rows(ctx, rows, t):
    """Route 2: solve_correspondences (double rows always take the grid chain)."""
    rw = od.golden_rows() if rows == "golden" else od.spread_rows()
    p = od.ls_params(ls_threshold=t)
    ctx.set_params(p)
    ok, D = ctx.solve_correspondences(LS, *rw)
    okr, Dr = oc.solve(LS, *rw, p)
    err = float(np.abs(D - Dr).max())
    _measured("C", f"solve_correspondences {rows} t={t}", err, od.POSE_TOL)
    assert ok == okr and err < od.POSE_TOL, err


@pytest.mark.parametrize("t", od.TRIMS)
def test_trim_grid_chain_frame(ctx, t):
    """Route 3: a full scan (> 4096 valid rows in every iteration)."""
    p = od.ls_params(3, ls_threshold=t)
    _load(ctx, p, *od.frame("full"))
    want = od.oracle_frame("full", p)
    assert all(u.n_valid > 4096 for u in want["trace"])
    _check_frame(ctx.register_frame(), want, od.POSE_TOL, "C", f"frame full t={t}")


@pytest.mark.parametrize("t", [0.0, 0.49])
def test_trim_batched(t):
    """Route 4: one batch over the one-block solve, the grid chain and a TOO_FEW frame."""
    p = od.ls_params(3, ls_threshold=t)
    names = ["golden", "full", "tiny"]
    for name, r in zip(names, _batch_equals_alone(p, names)):
        _check_frame(r, od.oracle_frame(name, p), od.POSE_TOL, "C", f"batched {name} t={t}")


@pytest.mark.parametrize("name", sorted(od.EDGE_ROWS))
def test_trim_edges_grid_chain(ctx, name):
    """Both boundary ranks in one 1/128-octave bin (also with more than kCandCap rows in it: the
    overflow select), in adjacent bins, and N = 13 / N = 40 (7 / 2 rows kept).  A kept set of fewer
    than 6 rows is rank-deficient (test_gpu_ls_conditioning.py's contract): `ok` only."""
    build, t = od.EDGE_ROWS[name]
    rw = build()
    p = od.ls_params(ls_threshold=t)
    ctx.set_params(p)
    ok, D = ctx.solve_correspondences(LS, *rw)
    okr, Dr = oc.solve(LS, *rw, p)
    assert ok == okr
    lo, hi = od.trim_ranks(t, len(rw[0]))
    if hi - lo + 1 >= 6:
        err = float(np.abs(D - Dr).max())
        _measured("C", f"edge rows {name}", err, od.POSE_TOL)
        assert err < od.POSE_TOL, err


@pytest.mark.parametrize("name", sorted(od.EDGE_SCENES))
def test_trim_edges_small_solve(ctx, name):
    """k_solve_small with both boundary ranks in one 1/16-octave bin / in adjacent bins, with ≤ 512
    candidates (rank_sort) and more (the bitonic branch): project + solve(), and one iteration of
    register_frame (n_kept)."""
    n, kind, t = od.EDGE_SCENES[name]
    src, tgt = od.plane_scene(n, kind)
    p = od.ls_params(1, ls_threshold=t)
    _load(ctx, p, src, tgt)
    want = oc.project(np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T), np.eye(4), p)
    _check_projection(ctx.project(np.eye(4)), want, "C", f"edge scene {name}")
    ok, D = ctx.solve()
    okr, Dr = oc.solve(LS, *(v.astype(np.float64) for v in want[:3]), p)
    err = float(np.abs(D - Dr).max())
    _measured("C", f"edge scene {name} solve", err, od.POSE_TOL)
    assert ok == okr and err < od.POSE_TOL, err
    r = ctx.register_frame()
    wf = oc.register_frame(np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T), p)
    lo, hi = od.trim_ranks(t, n)
    assert wf["trace"][0].n_kept == hi - lo + 1
    _check_frame(r, wf, od.POSE_TOL, "C", f"edge scene {name} frame")


@pytest.mark.parametrize("name,t,kept", [("g13", 0.3, 7), ("g40", 0.49, 2)])
def test_trim_small_n_frames(ctx, name, t, kept):
    """N = 13, t = 0.3 (lo 3, hi 9) and N = 40, t = 0.49 (lo 19, hi 20) through k_solve_small; the
    2-row system is rank-deficient: status and n_kept only."""
    p = od.ls_params(1, ls_threshold=t)
    _load(ctx, p, *od.frame(name))
    want = od.oracle_frame(name, p)
    assert want["trace"][0].n_kept == kept
    _check_frame(ctx.register_frame(), want, od.POSE_TOL, "C", f"frame {name} t={t}", compare_delta=kept >= 6)


def _trim_pair_params(solver, ls_t, ransac_t, iters=2):
    if solver == "LS":
        return od.ls_params(iters, ls_threshold=ls_t, ransac_ls_threshold=ransac_t)
    return rc.shipped_params(iters=iters, final="LS", pct=0.5, hyps=40, ls_threshold=ls_t, ransac_ls_threshold=ransac_t)


@pytest.mark.parametrize("ls_t,ransac_t", [(0.02, 0.0), (0.02, 0.25), (0.0, 0.02), (0.25, 0.02)])
def test_the_two_trim_fields_are_not_crossed(ctx, ls_t, ransac_t):
    """RANSAC's final LS trims by ransac_ls_threshold and the LS solver by ls_threshold, with the
    other field at another value: stand-alone solves (≤ 4096 and > 4096 rows), then frames alone
    and batched."""
    for n in od.HUBER_SIZES:
        rows = rc.outlier_set(n)
        p = _trim_pair_params("RANSAC", ls_t, ransac_t)
        ctx.set_params(p)
        ctx.seed_rng(p.ransac_seed)
        ok, D = ctx.solve_correspondences(RANSAC, *rows)
        okr, Dr, st, _ = rc.oracle_solve(rows, p)
        err = float(np.abs(D - Dr).max())
        _measured("C", f"RANSAC-LS rows={n} ls={ls_t} ransac_ls={ransac_t}", err, od.POSE_TOL)
        assert ok == okr and err < od.POSE_TOL, err
        assert np.array_equal(ctx.rng_state(), st)
        p = _trim_pair_params("LS", ls_t, ransac_t)
        ctx.set_params(p)
        ok, D = ctx.solve_correspondences(LS, *rows)
        okr, Dr = oc.solve(LS, *rows, p)
        err = float(np.abs(D - Dr).max())
        _measured("C", f"LS rows={n} ls={ls_t} ransac_ls={ransac_t}", err, od.POSE_TOL)
        assert ok == okr and err < od.POSE_TOL, err
    names = ["golden", "full", "tiny"]
    for solver in ("RANSAC", "LS"):
        p = _trim_pair_params(solver, ls_t, ransac_t)
        for name, r in zip(names, _batch_equals_alone(p, names)):
            want = od.oracle_frame(name, p)
            _check_frame(r, want, od.POSE_TOL, "C", f"batched {solver} {name} ls={ls_t} ransac_ls={ransac_t}", kept=solver == "LS")
            assert np.array_equal(r["rand_state"], want["rand_state"]), name


# ================================================================================================
# D. RANSAC inlier gate and Huber weights
# ================================================================================================
def _ransac_solve_both(ctx, rows, p, final, section, label):
    ctx.set_params(p)
    ctx.seed_rng(p.ransac_seed)
    ok, D = ctx.solve_correspondences(RANSAC, *rows)
    okr, Dr, st, _ = rc.oracle_solve(rows, p)
    err = float(np.abs(D - Dr).max())
    _measured(section, f"{label} final={final} rows={len(rows[0])}", err, rc.tol_of(final))
    assert ok == okr and err < rc.tol_of(final), err
    assert np.array_equal(ctx.rng_state(), st)
    return D


@pytest.mark.parametrize("dist,huber", sorted(od.HUBER_CASES))
@pytest.mark.parametrize("n", od.HUBER_SIZES)
def test_huber_weights_and_gate(ctx, n, dist, huber):
    """Both branches of w = √a < h₂ ? a : 2h₂√a − h₂² and the gate dist < distance_threshold, at
    ≤ 4096 rows (one-block compaction) and above (grid); the weighted-LS and DRPM finals consume the
    weights, the LS final must not (bit-equal Δ under another huber threshold)."""
    rows = rc.outlier_set(n)
    for final in ("WLS", "DRPM", "LS"):
        D = _ransac_solve_both(ctx, rows, od.huber_params(dist, huber, final), final, "D", f"gate={dist} huber={huber}")
        if final == "LS":
            other = od.huber_params(dist, 0.5 * huber, final)
            ctx.set_params(other)
            ctx.seed_rng(other.ransac_seed)
            assert np.array_equal(ctx.solve_correspondences(RANSAC, *rows)[1], D)


@pytest.mark.parametrize("final", ["WLS", "DRPM"])
@pytest.mark.parametrize("dist,huber", sorted(od.HUBER_CASES))
def test_huber_batched(dist, huber, final):
    p = rc.shipped_params(iters=2, final=final, pct=0.5, hyps=40, thr=dist, ransac_huber_threshold=huber)
    names = ["golden", "full", "tiny"]
    for name, r in zip(names, _batch_equals_alone(p, names)):
        want = od.oracle_frame(name, p)
        _check_frame(r, want, rc.tol_of(final), "D", f"batched {name} gate={dist} huber={huber} {final}", kept=False)
        assert np.array_equal(r["rand_state"], want["rand_state"]), name


@pytest.mark.parametrize("dist,huber", od.HUBER_FRAME_CASES)
def test_huber_frame(ctx, dist, huber):
    p = od.ransac_frame_params(3, ransac_distance_threshold=dist, ransac_huber_threshold=huber)
    _load(ctx, p, *od.frame("golden"))
    want = od.oracle_frame("golden", p)
    _check_frame(ctx.register_frame(), want, od.DRPM_TOL, "D", f"frame gate={dist} huber={huber}", kept=False)
    assert np.array_equal(ctx.rng_state(), want["rand_state"])


# ================================================================================================
# E. DRPM probabilities
# ================================================================================================
@pytest.mark.parametrize("case", od.DRPM_CASES, ids=lambda c: "-".join(f"{v:g}" for v in c))
@pytest.mark.parametrize("n", od.DRPM_SIZES)
def test_drpm_probabilities(ctx, n, case):
    """drpm_threshold / stdevs away from the saturated probabilities, with caller weights
    (imls_solve_correspondences(IMLS_SOLVE_DRPM)) and as RANSAC's final, at ≤ 4096 rows
    (k_drpm_head_small) and above (the grid pass + k_drpm_eig)."""
    rows = rc.outlier_set(n)
    p = od.drpm_params(case)
    w = od.caller_weights(n)
    ctx.set_params(p)
    ok, D = ctx.solve_correspondences(_abi.IMLS_SOLVE_DRPM, *rows, w)
    okr, Dr = oc.solve(_abi.IMLS_SOLVE_DRPM, *rows, p, weights=w)
    err = float(np.abs(D - Dr).max())
    _measured("E", f"caller weights {case} rows={n}", err, od.DRPM_TOL)
    assert ok == okr and err < od.DRPM_TOL, err
    _ransac_solve_both(ctx, rows, p, "DRPM", "E", f"RANSAC->DRPM {case}")


@pytest.mark.parametrize("case", od.DRPM_CASES, ids=lambda c: "-".join(f"{v:g}" for v in c))
def test_drpm_batched(case):
    p = od.drpm_params(case)
    p.iterations = 2
    names = ["golden", "full", "tiny"]
    for name, r in zip(names, _batch_equals_alone(p, names)):
        want = od.oracle_frame(name, p)
        _check_frame(r, want, od.DRPM_TOL, "E", f"batched {name} {case}", kept=False)
        assert np.array_equal(r["rand_state"], want["rand_state"]), name
