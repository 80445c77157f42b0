"""GPU parity of the RANSAC solve path with the oracle ABOVE the sizes where the RANSAC solve
(csrc/ransac.hip, compact_rows.hip, drpm.hip) changes its code path (tests/test_gpu_ransac.py stays
at ≤ 4000 rows):

  > 4096 rows   grid inlier compaction, grid pass 1 + k_drpm_eig and the grid LS chain instead of
                k_drpm_head_small / the folded selection; 256-thread hypothesis blocks when batched
  > 16384 rows  k_compact_count / _scan / _scatter (lone and batched) instead of k_compact_one
  hypotheses    a lone frame's chunks 272 + 8192 + …, the batched launch's 16 + 256 + …

Every case (tests/ransac_cases.py; tests/test_ransac_size_cases.py proves on the oracle alone that
each does what it is meant to) asserts `ok` equal, |Δ − Δ_oracle| below the suite's tolerances (1e-6
LS / weighted LS, 1e-5 DRPM, as test_gpu_ransac.py) and the device rand() state EQUAL to the
oracle's — the exact number of hypotheses evaluated and committed, which Δ alone does not show.  The
sentinel cases make Δ sensitive to single rows at the compaction's block edges (one sentinel lost
moves the oracle's Δ by ≥ 100 × the tolerance); register_frame adds iterations, status and every
iteration's n_valid and Δ.  Each test prints its measured |Δ − Δ_oracle| before it asserts.
"""
import numpy as np
import pytest

import oracle_ctypes as oc
import ransac_cases as rc
from planetary_lidar_odometry_amd import _abi, imls_icp, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = imls_icp.ImlsContext(rc.shipped_params())
    yield c
    c.close()


def _solve_both(ctx, rows, p, final, label):
    """One stand-alone RANSAC solve on the device and in the oracle, each on a fresh rand() stream."""
    ctx.set_params(p)
    ctx.seed_rng(p.ransac_seed)
    ok, D = ctx.solve_correspondences(_abi.IMLS_SOLVE_RANSAC, *rows)
    st = oc.rand_state(p.ransac_seed)
    okr, Dr = oc.solve(_abi.IMLS_SOLVE_RANSAC, *rows, p, rand_state=st)
    err = np.abs(D - Dr).max()
    print(f"MEASURED {label} final={final} rows={len(rows[0])} max|dDelta|={err:.3e}")
    assert ok == okr
    assert err < rc.tol_of(final), err
    got = ctx.rng_state()
    assert np.array_equal(got, st), ("draws", rc.draws_consumed(oc.rand_state(p.ransac_seed), got, 10000),
                                    rc.draws_consumed(oc.rand_state(p.ransac_seed), st, 10000))
    return D


_SOLVES = [(n, mode) for n in rc.SIZES for mode in rc.solve_modes(n)]


@pytest.mark.parametrize("final", ["LS", "WLS", "DRPM"])
@pytest.mark.parametrize("n,mode", _SOLVES, ids=[f"{n}-{m}" for n, m in _SOLVES])
def test_standalone_solve_sizes(ctx, n, mode, final):
    """solve_correspondences on fp64 rows at both sides of 4096 and 16384 and well above: an exit
    within the first hypotheses, no exit (300 hypotheses), and a late exit in the chunk the case
    names (second lone chunk; first lone chunk but second batched chunk)."""
    rows, p = rc.solve_case(n, mode, final)
    _solve_both(ctx, rows, p, final, f"solve[{mode}]")


@pytest.mark.parametrize("final", ["LS", "DRPM"])
def test_three_lone_chunks(ctx, final):
    """9000 hypotheses without an exit at 4097 rows: chunks 272 + 8192 + 536, the last behind a commit
    of the first 8464 draws; the final state is the oracle's after exactly 9000 draws."""
    rows, p = rc.three_chunk_case(final)
    _solve_both(ctx, rows, p, final, "three-chunks")
    assert rc.draws_consumed(oc.rand_state(p.ransac_seed), ctx.rng_state(), 9000) == 9000


@pytest.mark.parametrize("swap", [False, True], ids=["rows", "swapped"])
@pytest.mark.parametrize("final", ["LS", "WLS", "DRPM"])
@pytest.mark.parametrize("n", [4096, 16385, 40000])
def test_sentinel_rows(ctx, n, final, swap):
    """Rows that alone fix t_y sit on both sides of every block edge of the compactions (0, 255|256,
    4095|4096, 16383|16384, 39935|39936, n − 1): a row dropped, doubled or replaced there moves Δ
    by ≥ 100 × the tolerance (single rows for LS / weighted LS, groups for DRPM, whose single rows
    still move it by ≥ 3 ×).  `swapped`: the first and last sentinel exchanged."""
    rows, p, _ = rc.sentinel_case(n, final, swap=swap)
    _solve_both(ctx, rows, p, final, f"sentinels[{'swapped' if swap else 'rows'}]")


@pytest.fixture(scope="module")
def frames():
    return {name: build() for name, (build, _) in rc.FRAMES.items()}


def _check_frame(r, want, final, label, n_valid_range=None):
    tol = rc.tol_of(final)
    errs = [np.abs(np.array(t.delta) - np.array(u.delta)).max() for t, u in zip(r["trace"], want["trace"])]
    err = max([np.abs(r["pose"] - want["pose"]).max()] + errs)
    print(f"MEASURED {label} final={final} n_valid={[int(u.n_valid) for u in want['trace']]} max|dDelta|={err:.3e}")
    assert r["iters"] == want["iters"] and r["status"] == want["status"]
    assert len(r["trace"]) == len(want["trace"])
    for t, u in zip(r["trace"], want["trace"]):
        assert t.n_valid == u.n_valid
        if n_valid_range:
            assert n_valid_range[0] <= u.n_valid < n_valid_range[1]
    assert err < tol, err


_FRAME_CASES = [("hdl-stride5", "LS"), ("hdl-stride5", "WLS"), ("hdl-stride5", "DRPM"), ("hdl-stride3", "LS"),
                ("hdl-stride3", "DRPM"), ("config-a", "LS"), ("config-a", "DRPM")]


@pytest.mark.parametrize("mode", sorted(rc.FRAME_MODES))
@pytest.mark.parametrize("name,final", _FRAME_CASES, ids=[f"{a}-{b}" for a, b in _FRAME_CASES])
def test_register_frame_sizes(ctx, frames, name, final, mode):
    """register_frame end to end (the float valid-row compaction, which the stand-alone solves never
    reach) with > 16384 valid rows (strided HDL-64) and 4096 < valid rows ≤ 16384 (config A), with
    the shipped exit bar and without an exit."""
    src, tgt = frames[name]
    p = rc.frame_params(final, mode)
    ctx.set_params(p)
    ctx.seed_rng(p.ransac_seed)
    ctx.set_target(tgt)
    ctx.set_source(src)
    r = ctx.register_frame()
    st = oc.rand_state(p.ransac_seed)
    want = oc.register_frame(synth.soa(src), synth.soa(tgt), p, rand_state=st)
    _check_frame(r, want, final, f"frame[{name},{mode}]", rc.FRAMES[name][1])
    assert np.array_equal(ctx.rng_state(), st)


@pytest.mark.parametrize("final", ["DRPM", "LS"])
def test_batched_launch_against_oracle(frames, final):
    """imls_register_frames on a > 16384-row frame, a 1500-query frame and a TOO_FEW frame, each in
    a fresh context: the small frame runs through the 256-thread batched hypothesis kernel and the
    three-kernel batched compaction because of the large one.  Every frame against the oracle on a
    fresh rand() stream (test_gpu_frames.py compares batched with alone, not with the oracle)."""
    vsrc, vtgt = frames["config-a"]
    batch = [frames["hdl-stride5"], (synth.fps_subsample(vsrc, 1500, seed=1), vtgt), (vsrc[:4], vtgt)]
    p = rc.frame_params(final, "no-exit", iters=2)
    ctxs = [imls_icp.ImlsContext(p) for _ in batch]
    try:
        for c, (src, tgt) in zip(ctxs, batch):
            c.set_target(tgt)
            c.set_source(src)
        poses, iters, status, traces = imls_icp.register_frames(ctxs)
        states = [c.rng_state() for c in ctxs]
    finally:
        for c in ctxs:
            c.close()
    for k, (src, tgt) in enumerate(batch):
        st = oc.rand_state(p.ransac_seed)
        want = oc.register_frame(synth.soa(src), synth.soa(tgt), p, rand_state=st)
        got = dict(pose=poses[k], iters=int(iters[k]), status=int(status[k]), trace=list(traces[k]))
        _check_frame(got, want, final, f"batched[{k}]")
        assert np.array_equal(states[k], st), k
    assert status[2] == _abi.IMLS_FRAME_TOO_FEW
    assert traces[0][0].n_valid > 16384 and traces[1][0].n_valid <= 4096
