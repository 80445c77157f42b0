"""Deterministic RANSAC cases above the solver's size switches (shared by test_ransac_size_cases.py,
which proves on the CPU oracle alone that each case does what it is meant to, and
test_gpu_ransac_sizes.py, which runs them on the device).  No GPU imports.

The RANSAC solve (csrc/ransac.hip, compact_rows.hip, drpm.hip) changes its code path at three row counts: > 4096 rows (kSmallRows: grid inlier
compaction, grid pass 1 and LS chain instead of the one-launch head; 256-thread hypothesis blocks in
the batched launch), > 16384 rows (kCompactOne: three-kernel compaction instead of one block) and,
for a lone frame, at hypothesis 272 and 8464 (the chunk edges 272 + 8192 + …).

outlier_set():    correspondences of a known motion on three plane families, a fraction corrupted.
sentinel_set():   the same, but every bulk normal has an exactly zero y component, so the bulk rows
                  leave t_y free: only the sentinel rows (normal e_y, each with its own target offset
                  along y) fix it.  One sentinel dropped, duplicated or replaced by its neighbour moves
                  Δ by far more than the parity tolerance — a compaction off by one row shows.
draws_consumed(): number of rand() words between two glibc states (one per hypothesis).
hdl_strided():    an HDL-64 scan thinned by a stride against its 1-scan map (> 16384 valid rows).
"""
import functools

import numpy as np

import oracle_ctypes as oc
from planetary_lidar_odometry_amd import _abi, config, synth

POSE_TOL = 1e-6
DRPM_TOL = 1e-5
FINALS = {"LS": _abi.IMLS_FINAL_LS, "WLS": _abi.IMLS_FINAL_WEIGHTED_LS, "DRPM": _abi.IMLS_FINAL_DRPM}
SIZES = (4096, 4097, 16384, 16385, 40000)


def tol_of(final):
    return DRPM_TOL if final == "DRPM" else POSE_TOL


def shipped_params(iters=10, final="DRPM", **ransac):
    """The shipped config.json (RANSAC → DRPM) with the chosen final method; keyword arguments set
    the ransac_* fields (pct= is short for ransac_min_inliers_percentage, hyps= for
    ransac_max_iterations, thr= for ransac_distance_threshold)."""
    p = config.params_from_config(config.load())
    p.iterations = iters
    p.solve_method = _abi.IMLS_SOLVE_RANSAC
    p.ransac_final_method = FINALS[final]
    short = dict(pct="ransac_min_inliers_percentage", hyps="ransac_max_iterations", thr="ransac_distance_threshold")
    for k, v in ransac.items():
        setattr(p, short.get(k, k), v)
    return p


def outlier_set(n=4000, frac=0.3, seed=7):
    """Correspondences of a known motion on three plane families, `frac` of them corrupted."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-15, 15, (n, 3))
    nrm = np.zeros((n, 3))
    nrm[np.arange(n), rng.integers(0, 3, n)] = 1.0
    nrm += rng.normal(0, 0.05, (n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    a = 0.02
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    d = s @ R.T + np.array([0.3, -0.1, 0.05])
    bad = rng.random(n) < frac
    d[bad] += rng.normal(0, 2.0, (bad.sum(), 3))
    return s, d, nrm


def sentinel_offsets(count):
    """The default target offsets of `count` sentinels, 0.10 + 0.005·k·(k + 1): all distinct, and none
    equal to the mean of the others (an LS solve would not miss that one)."""
    k = np.arange(count)
    return 0.10 + 0.005 * k * (k + 1)


def sentinel_set(n, sentinels, frac=0.2, seed=7, offsets=None, broken=()):
    """Correspondences of a known motion whose bulk rows have normals in the x and z families only
    (y component exactly zero), `frac` of the bulk corrupted.  Row sentinels[k] has the normal e_y
    and its target moved by offsets[k] along y (default sentinel_offsets); its source point lies within
    1.5 m of the origin, so a hypothesis' rotation error cannot push it past the inlier threshold.
    Sentinels are never outliers, except those listed in `broken`, which become gross outliers (5 m
    along y) in place: the row count, every other row and so every rand() % N stay what they were."""
    sentinels = np.asarray(sentinels, dtype=np.int64)
    assert len(np.unique(sentinels)) == len(sentinels) and sentinels.min() >= 0 and sentinels.max() < n
    offsets = sentinel_offsets(len(sentinels)) if offsets is None else np.asarray(offsets, dtype=np.float64)
    assert offsets.shape == sentinels.shape
    rng = np.random.default_rng(seed)
    s = rng.uniform(-15, 15, (n, 3))
    nrm = np.zeros((n, 3))
    nrm[np.arange(n), 2 * rng.integers(0, 2, n)] = 1.0          # x or z family
    nrm[:, [0, 2]] += rng.normal(0, 0.05, (n, 2))               # y stays exactly zero
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    s[sentinels] *= 0.1
    a = 0.02
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    d = s @ R.T + np.array([0.3, -0.1, 0.05])
    bad = rng.random(n) < frac
    bad[sentinels] = False
    d[bad] += rng.normal(0, 2.0, (bad.sum(), 3))
    nrm[sentinels] = (0.0, 1.0, 0.0)
    d[sentinels, 1] += offsets
    broken = np.asarray(list(broken), dtype=np.int64)
    assert np.isin(broken, sentinels).all()
    d[broken, 1] += 5.0
    return s, d, nrm


def boundary_sentinels(n):
    """Single sentinel rows on both sides of every block edge the compactions have at n rows: the
    first and last row, the 256-row block edge, the 4096 and 16384 switches and the last block."""
    idx = [0, 255, 256, 4095, 4096, 16383, 16384, 39935, 39936, n - 1]
    return sorted({i for i in idx if 0 <= i < n})


def boundary_groups(n):
    """For DRPM, which zeroes a direction that only a handful of rows constrain (the direction's
    share of the weight must exceed about 11·drpm_stdev_normals², 2.75 % shipped): the rows within
    n // 100 of an edge (0, 256, 4096, 16384, 39936, n) are sentinels, 4 to 7 % of all; one group per
    run of consecutive rows, each straddling its edges.  A list of index arrays."""
    half = max(n // 100, 1)
    mask = np.zeros(n, bool)
    for e in (0, 256, 4096, 16384, 39936, n):
        if e <= n:
            mask[max(e - half, 0):min(e + half, n)] = True
    idx = np.flatnonzero(mask)
    return np.split(idx, np.flatnonzero(np.diff(idx) > 1) + 1)


def group_offsets(groups):
    """Each group sentinel its own offset: 0.10 + 0.02·g for group g, plus a zig-zag of ±0.3 m within
    the run (so two neighbours differ by ~0.6 m: one row dropped or doubled moves the mean)."""
    out = []
    for g, idx in enumerate(groups):
        j = np.arange(len(idx))
        out.append(0.10 + 0.02 * g + 0.3 * (1 - 2 * (j % 2)) * (1.0 - 0.5 * j / max(len(idx), 1)))
    return np.concatenate(out)


def swap_rows(rows, i, j):
    """The same correspondences with rows i and j exchanged."""
    out = tuple(np.array(a, copy=True) for a in rows)
    for a in out:
        a[[i, j]] = a[[j, i]]
    return out


def draws_consumed(state_before, state_after, limit):
    """rand() words drawn between two glibc states (a hypothesis draws exactly one): steps a copy of
    state_before until it equals state_after; None if more than `limit` steps would be needed."""
    st = np.array(state_before, dtype=np.int32, copy=True)
    want = np.asarray(state_after, dtype=np.int32)
    nxt, ptr = oc.lib().oracle_rand_next, oc._ptr(st)
    for k in range(limit + 1):
        if np.array_equal(st, want):
            return k
        nxt(ptr)
    return None


def oracle_solve(rows, p):
    """(ok, Δ, rand() state after, draws) of the oracle's RANSAC on a fresh stream."""
    st = oc.rand_state(p.ransac_seed)
    ok, D = oc.solve(_abi.IMLS_SOLVE_RANSAC, *rows, p, rand_state=st)
    return ok, D, st, draws_consumed(oc.rand_state(p.ransac_seed), st, p.ransac_max_iterations)


@functools.lru_cache(maxsize=None)
def _pair(model):
    return synth.make_pair("hdl64", map_scans=1) if model == "hdl64" else synth.make_pair("vlp16", map_scans=1, start=5)


def hdl_strided(stride):
    """(source, target): every stride-th point of an HDL-64 scan against its 1-scan map."""
    pair = _pair("hdl64")
    return pair.source[::stride], pair.target


def config_a_pair():
    """(source, target) of the full config-A pair (VLP-16 against a 1-scan map)."""
    pair = _pair("vlp16")
    return pair.source, pair.target


# real-scan frames: name -> (builder, the range the oracle's n_valid must lie in at every iteration)
FRAMES = {
    "hdl-stride5": (lambda: hdl_strided(5), (16385, 1 << 30)),
    "hdl-stride3": (lambda: hdl_strided(3), (16385, 1 << 30)),
    "config-a": (config_a_pair, (4097, 16385)),
}
FRAME_MODES = {"shipped": dict(pct=0.95, hyps=5000), "no-exit": dict(pct=1.0, hyps=300)}


def frame_params(final, mode, iters=3):
    return shipped_params(iters=iters, final=final, **FRAME_MODES[mode])


# ---- the frozen cases ------------------------------------------------------------------------------
# Late exits, placed by a search on the oracle alone (over the outlier fraction, the set's seed and
# the inlier bar; ransac_seed 1, distance threshold 0.2; each bar sits well inside the range of bars that give
# the same exit); `window` is the half-open range of draws the exit must fall in, which
# test_ransac_size_cases.py asserts:
#   ≥ 272            the lone launch's second chunk (at ≤ 4096 rows with the DRPM final: one selection
#                    over both chunks and the `hit` shortcut of k_ransac_hyp with base > 0)
#   17 … 272         the lone launch's first chunk, but the batched launch's second
SECOND_CHUNK = (273, 5000)      # draws: exit at hypothesis index >= 272, before the 5000 run out
FIRST_CHUNK = (17, 273)         # draws: exit at index 16 … 271
LATE_EXITS = {
    # name: (n, frac, set seed, inlier bar, window of draws)
    "4096-second-chunk": (4096, 0.5, 9, 0.51, SECOND_CHUNK),
    "4097-second-chunk": (4097, 0.5, 7, 0.52, SECOND_CHUNK),
    "16384-first-chunk": (16384, 0.3, 7, 0.70, FIRST_CHUNK),
    "16385-first-chunk": (16385, 0.3, 7, 0.70, FIRST_CHUNK),
    "16385-second-chunk": (16385, 0.5, 8, 0.52, SECOND_CHUNK),
    "40000-first-chunk": (40000, 0.3, 7, 0.70, FIRST_CHUNK),
}


# stand-alone solves on outlier_set rows: how the hypothesis loop ends
def solve_case(n, mode, final):
    """(rows, params): "early" — 2 % outliers, the shipped 0.95 / 5000 bar: exit within the first
    hypotheses; "none" — 30 % outliers, a 100 % bar, 300 hypotheses: all of them run; any LATE_EXITS name."""
    if mode == "early":
        return outlier_set(n, 0.02, 7), shipped_params(final=final)
    if mode == "none":
        return outlier_set(n, 0.3, 7), shipped_params(final=final, pct=1.0, hyps=300)
    assert LATE_EXITS[mode][0] == n
    return late_exit(mode, final)


def three_chunk_case(final):
    """(rows, params): 4097 rows, 9000 hypotheses without an exit — a lone frame's chunks are
    272 + 8192 + 536, the third behind a commit and a re-jump of the rand() table."""
    return outlier_set(4097, 0.3, 7), shipped_params(final=final, pct=1.0, hyps=9000)


def solve_modes(n):
    return ["early", "none"] + [k for k, v in LATE_EXITS.items() if v[0] == n]


def late_exit(name, final):
    """(rows, params) of a LATE_EXITS case: the shipped 5000 hypotheses, distance threshold 0.2."""
    n, frac, seed, pct, _ = LATE_EXITS[name]
    return outlier_set(n, frac, seed), shipped_params(final=final, pct=pct, hyps=5000, thr=0.2)


def sentinel_case(n, final, broken=(), swap=False):
    """(rows, params, sentinels or groups) of the sentinel case at n rows: single boundary rows for
    the LS / weighted-LS finals, boundary groups for DRPM; the inlier bar 70 % of the rows (80 % are
    inliers), at most 300 hypotheses.  swap: the first and the last sentinel row exchanged."""
    if final == "DRPM":
        units = boundary_groups(n)
        idx = np.concatenate(units)
        rows = sentinel_set(n, idx, offsets=group_offsets(units), broken=broken)
    else:
        idx = np.asarray(boundary_sentinels(n))
        units = [np.array([i]) for i in idx]
        rows = sentinel_set(n, idx, broken=broken)
    if swap:
        rows = swap_rows(rows, int(idx[0]), int(idx[-1]))
    return rows, shipped_params(final=final, pct=0.7, hyps=300), units
