"""CPU: the cases of tests/ransac_cases.py do what they are meant to do — proved on the oracle
alone, so that none of them can silently degrade into a case the device passes for free.  These are
conditions on the cases, not measurements of the device:

* every late exit falls in its window of hypotheses (the chunk of the device launch it targets);
  the early exit is inside the first batched chunk, "no exit" runs every hypothesis;
* every sentinel (LS, weighted LS) and every sentinel group (DRPM) matters: with it turned into a
  gross outlier — in place, same row count, same rand() % N, same number of draws — the oracle's Δ
  moves by at least 100 × the tolerance test_gpu_ransac_sizes.py compares with;
* the real-scan frames have their valid-row counts on the intended side of 4096 / 16384 at every
  ICP iteration.
"""
import numpy as np
import pytest

import oracle_ctypes as oc
import ransac_cases as rc
from planetary_lidar_odometry_amd import synth


@pytest.mark.parametrize("name", sorted(rc.LATE_EXITS))
def test_late_exit_falls_in_its_window(name):
    rows, p = rc.late_exit(name, "LS")
    lo, hi = rc.LATE_EXITS[name][4]
    ok, _, _, draws = rc.oracle_solve(rows, p)
    assert ok and draws is not None
    assert lo <= draws < hi, draws
    assert hi <= p.ransac_max_iterations                # an exit, not the end of the loop
    if "second-chunk" in name:                          # 272 + the rest, both within one jump table
        assert p.ransac_max_iterations - 272 > 0 and p.ransac_max_iterations <= 8192


@pytest.mark.parametrize("n", rc.SIZES)
def test_early_and_no_exit(n):
    rows, p = rc.solve_case(n, "early", "LS")
    ok, _, _, draws = rc.oracle_solve(rows, p)
    assert ok and 1 <= draws <= 16, draws
    rows, p = rc.solve_case(n, "none", "LS")
    ok, _, _, draws = rc.oracle_solve(rows, p)
    assert ok and draws == p.ransac_max_iterations == 300


def test_three_chunks_draw_9000():
    rows, p = rc.three_chunk_case("LS")
    assert len(rows[0]) == 4097 and p.ransac_max_iterations == 9000 > 272 + 8192
    ok, _, _, draws = rc.oracle_solve(rows, p)
    assert ok and draws == 9000


@pytest.mark.parametrize("final", ["LS", "WLS", "DRPM"])
@pytest.mark.parametrize("n", [4096, 16385, 40000])
def test_every_sentinel_matters(n, final):
    rows, p, units = rc.sentinel_case(n, final)
    ok, D0, st0, draws0 = rc.oracle_solve(rows, p)
    assert ok and 1 <= draws0 < p.ransac_max_iterations
    edges = [e for e in (0, 256, 4096, 16384, 39936, n) if e <= n]
    covered = np.concatenate(units)
    for e in edges:                                     # a sentinel on both sides of every edge
        assert (e == 0 or e - 1 in covered) and (e == n or e in covered), e
    need = 100 * rc.tol_of(final)
    for u in units:
        broken, _, _ = rc.sentinel_case(n, final, broken=u)
        ok, D, st, draws = rc.oracle_solve(broken, p)
        assert ok and draws == draws0 and np.array_equal(st, st0)      # the row's effect, not a changed draw
        assert np.abs(D - D0).max() >= need, (int(u[0]), len(u), np.abs(D - D0).max())
    if final == "DRPM":
        # one row of a group still shows above the tolerance (the groups' zig-zag offsets)
        for i in (units[0][0], units[0][-1], units[-1][0], units[-1][-1]):
            broken, _, _ = rc.sentinel_case(n, final, broken=[i])
            ok, D, st, _ = rc.oracle_solve(broken, p)
            assert ok and np.array_equal(st, st0)
            assert np.abs(D - D0).max() >= 3 * rc.DRPM_TOL, (int(i), np.abs(D - D0).max())


@pytest.mark.parametrize("final", ["LS", "DRPM"])
def test_swapped_sentinels_are_another_case(final):
    """The permuted copy exchanges two rows that differ (offsets, positions): the same set, another order."""
    rows, _, units = rc.sentinel_case(16385, final)
    swapped, _, _ = rc.sentinel_case(16385, final, swap=True)
    i, j = int(units[0][0]), int(units[-1][-1])
    for a, b in zip(rows, swapped):
        assert np.array_equal(a[i], b[j]) and np.array_equal(a[j], b[i])
        keep = np.ones(len(a), bool)
        keep[[i, j]] = False
        assert np.array_equal(a[keep], b[keep])
    assert not np.array_equal(rows[1][i] - rows[0][i], rows[1][j] - rows[0][j])


@pytest.mark.parametrize("mode", sorted(rc.FRAME_MODES))
@pytest.mark.parametrize("name", sorted(rc.FRAMES))
def test_frame_sizes(name, mode):
    build, (lo, hi) = rc.FRAMES[name]
    src, tgt = build()
    assert len(src) >= lo                               # the query count is the device's `cap`
    p = rc.frame_params("DRPM", mode)
    r = oc.register_frame(synth.soa(src), synth.soa(tgt), p)
    assert r["iters"] == 3
    for t in r["trace"]:
        assert lo <= t.n_valid < hi, t.n_valid
