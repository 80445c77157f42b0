"""Premises of test_gpu_index_edges.py, on numpy and the CPU oracle alone: each generator of
index_edge_cases.py reaches the edge it is named for, so the GPU tests cannot pass by missing it."""
import collections

import numpy as np
import pytest

import index_edge_cases as ec
import oracle_ctypes as oc


# ---- the reference ---------------------------------------------------------------------------------
def _argsort_knn(P, q, k, r, self_ok):
    """A second formulation: the candidates in index order, one stable argsort by distance."""
    P64 = np.asarray(P, np.float64)
    idx = np.full((len(q), k), -1, np.int32)
    d2o = np.full((len(q), k), np.inf)
    for i, x in enumerate(np.asarray(q, np.float64)):
        d = x[None, :] - P64
        d2 = (d[:, 0] ** 2 + d[:, 1] ** 2) + d[:, 2] ** 2
        cand = np.array([j for j in range(len(P64)) if d2[j] <= r * r and (self_ok or d2[j] > np.finfo(np.float64).eps)], np.int64)
        o = np.argsort(d2[cand], kind="stable")[:k]
        idx[i, : len(o)] = cand[o]
        d2o[i, : len(o)] = d2[cand][o]
    return idx, d2o


def test_brute_force_equals_stable_argsort():
    rng = np.random.default_rng(1)
    P = rng.integers(-3, 4, (700, 3)).astype(np.float32) * np.float32(0.5)     # many exact ties and duplicates
    q = np.concatenate([P[:40], rng.uniform(-2, 2, (40, 3)).astype(np.float32)])
    for k, r, self_ok in ((20, 1.0, False), (32, np.inf, True), (1, np.inf, True), (7, 0.5, True)):
        got = ec.brute_knn(P, q, k, r, self_ok)
        want = _argsort_knn(P, q, k, r, self_ok)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (k, r, self_ok)


def test_census_is_the_k1_row():
    P = ec.geometry("duplicate_groups")[::7]
    P = np.concatenate([P, P[:50]])
    idx, d2 = ec.census(P)
    bidx, bd2 = ec.brute_knn(P, P, 1, np.inf, True)
    assert np.array_equal(idx, bidx) and np.array_equal(d2, bd2)
    assert (idx[-50:, 0] <= np.arange(50)).all()


@pytest.mark.parametrize("name", ec.ORACLE_OK)
def test_oracle_agrees_with_brute_force(name):
    """The CPU oracle's kd-tree against the brute force where its tree stays shallow (the identical and
    duplicate-group clouds are left out: thousands of coincident points degenerate its tree)."""
    P = ec.geometry(name)
    q = ec.probes(P, 120, seed=3)
    tgt6 = np.ascontiguousarray(ec.rows6(P).T)
    for (k, r, self_ok), (bidx, bd2) in zip(ec.PROBE_CONFIGS, ec.brute_knn_multi(P, q, ec.PROBE_CONFIGS)):
        d2, idx = oc.knn(tgt6, np.ascontiguousarray(q.T), k, float(r), self_ok)
        assert np.array_equal(idx, bidx) and np.array_equal(d2, bd2), (name, k, r)


# ---- geometry ----------------------------------------------------------------------------------------
def _ext(a):
    return a.max(axis=0).astype(np.float64) - a.min(axis=0)


def test_geometry_cases_are_what_they_claim():
    g = {n: ec.geometry(n) for n in ec.GEOMETRY}
    for n in ("identical_200", "identical_2400"):
        assert len(np.unique(g[n], axis=0)) == 1 and len(g[n]) == int(n.split("_")[1])
    assert (_ext(g["line_4096"])[1:] == 0).all() and _ext(g["line_4096"])[0] > 90
    assert _ext(g["plane_4096"])[2] == 0 and (_ext(g["plane_4096"])[:2] > 35).all()
    far = g["far_offset_4096"]
    assert far.dtype == np.float32 and (_ext(far) <= 2.0 + 2 ** -6).all()
    assert (np.abs(far.mean(axis=0) - np.array(ec.FAR_CENTRE)) < 0.1).all()
    assert np.array_equal(far[:, :2] * 128, np.round(far[:, :2] * 128))        # the 2⁻⁷ m float grid at 1e5
    assert len(np.unique(far[:, 0])) <= 257                                    # 4,096 values on ≤ 257 grid lines
    sl = _ext(g["sliver_4096"])
    assert sl[0] > 990 and (sl[1:] <= 1e-3).all() and (sl[1:] > 0).all()
    _, counts = np.unique(g["duplicate_groups"], axis=0, return_counts=True)
    assert sorted(counts)[-5:] == [2400] * 5 and len(counts) == 3005            # groups ≫ k (32) and a leaf (64)
    assert all(len(g[n]) == 4096 for n in g if n.endswith("4096"))


@pytest.mark.parametrize("leaf", ec.LEAVES)
def test_size_edges_reach_the_subtree_rounds(leaf):
    for M in ec.SIZE_EDGES[leaf]:
        L, P, levels, rounds = ec.tree_shape(M, leaf)
        assert (P, rounds) == ec.SIZE_SHAPES[(leaf, M)], (leaf, M)
        assert P == 1 << levels and L <= P < 2 * max(L, 1)
    shapes = [tuple(ec.tree_shape(M, leaf)[3]) for M in ec.SIZE_EDGES[leaf]]
    assert (256,) in shapes and (256, 2) in shapes          # one round; 256 then 2
    if leaf == 4:
        assert (256, 256) in shapes and (256, 256, 2) in shapes and () in shapes
        assert [ec.tree_shape(M, 4)[1] for M in (1024, 1025, 262144, 262145)] == [256, 512, 65536, 131072]
    else:
        assert [ec.tree_shape(M, 64)[1] for M in (16384, 16385)] == [256, 512]


# ---- ties on the merge diagonals -----------------------------------------------------------------------
def _cross_run_groups(scans):
    """Sizes of the groups of equal points that have members in more than one scan."""
    runs = collections.defaultdict(set)
    size = collections.Counter()
    for r, s in enumerate(scans):
        for row in map(bytes, np.ascontiguousarray(ec.filtered_map([s]))):
            runs[row].add(r)
            size[row] += 1
    return [size[k] for k in size if len(runs[k]) > 1]


def test_tie_groups_span_a_tile():
    seq = ec.ties_sequence()
    for state in ec.fifo_states(seq, 3)[2:]:
        groups = _cross_run_groups(state)
        assert len(groups) == 5 and min(groups) > ec.MERGE_TILE, groups


def test_stationary_scans_tie_every_key():
    for seq in (ec.stationary_sequence(2), ec.id_wrap_sequence()):
        assert all(np.array_equal(s, seq[0][0]) for s, _ in seq)
    assert len(ec.stationary_sequence(31)) == 33
    assert len(ec.id_wrap_sequence()) == 70 > 2 * 32          # the 32 run ids wrap twice


@pytest.mark.parametrize("case", ["ties", "stationary"])
def test_merge_model_tie_rules(case):
    """Consistent tie rules reproduce the stable sort of the concatenation.  A strict per-thread split
    against the non-strict sequential merge drops one entry and doubles another — so the cases put
    ties on the threads' diagonals (every MERGE_PER outputs, the tile edges among them).  The tile split
    flipped alone keeps the multiset (both diagonals of a tile use the one rule, so the tiles still
    partition the inputs) but takes B first across a tile edge: the order is no longer the stable
    sort's — so the cases put ties on the tile diagonals too."""
    scans = [s for s, _ in (ec.ties_sequence()[:3] if case == "ties" else ec.stationary_sequence(2)[:3])]
    got, want = ec.model_fifo_merge(scans)
    assert got == want
    got, _ = ec.model_fifo_merge(scans, tile_strict=True, thread_strict=True, take_strict=True)
    assert collections.Counter(got) == collections.Counter(want) and got != want    # consistent, but B first: not stable
    got, _ = ec.model_fifo_merge(scans, thread_strict=True)
    assert collections.Counter(got) != collections.Counter(want)                    # dropped and doubled entries
    got, _ = ec.model_fifo_merge(scans, take_strict=True)
    assert collections.Counter(got) != collections.Counter(want)
    got, _ = ec.model_fifo_merge(scans, tile_strict=True)
    assert collections.Counter(got) == collections.Counter(want) and got != want


def test_merge_model_on_distinct_keys_ignores_the_rules():
    """Control: without cross-run ties no rule matters — what the suite had before these cases."""
    scans = [ec._scan(900 + k, 2500) for k in range(3)]
    got, want = ec.model_fifo_merge(scans, thread_strict=True)
    assert got == want


# ---- sizes on tile and block edges ------------------------------------------------------------------------
def test_size_sequence_visits_every_edge():
    tr = ec.fifo_trace(ec.SIZE_SEQUENCE, 3)
    assert {0, 1, ec.MERGE_TILE - 1} <= {t["total"] % ec.MERGE_TILE for t in tr}
    comp = [t for t in tr if t["compacts"]]
    assert {0, 1, ec.KEEP_TILE - 1} <= {t["old"] % ec.KEEP_TILE for t in comp}       # the compaction's input tiles
    assert {0, 1, ec.KEEP_TILE - 1} <= {t["kept"] % ec.KEEP_TILE for t in comp}      # its output: kept before the merge
    assert any(t["new"] == 1 and t["old"] == 0 for t in tr)                         # a one-point run, alone
    assert any(t["new"] == 1 and t["kept"] > ec.MERGE_TILE for t in tr)             # and merged into a large order
    assert tr[0]["old"] == 0                                                        # an empty old order
    assert any(t["grows"] for t in tr)                                              # order buffers grow while holding entries
    a, b = [k for _, k in ec.size_sequence("host")], [k for _, k in ec.size_sequence("device")]
    assert all({x, y} == {"host", "device"} for x, y in zip(a, b))                  # every edge through both filters
    assert [len(s) for s, _ in ec.size_sequence()] == list(ec.SIZE_SEQUENCE)


def test_empty_sequences():
    e = ec.empties_sequences()
    assert len(e["first_n0"][0][0]) == 0 and len(e["first_n0_device"][0][0]) == 0
    nan = e["first_nan"][0][0]
    assert len(nan) > 0 and len(ec.finite_rows(nan)) == 0
    for name in ("first_n0", "first_nan"):
        states = ec.fifo_states(e[name], 3)
        assert len(ec.filtered_map(states[0])) == 0                     # first push: no target
        assert len(ec.filtered_map(states[1])) > 0 and len(ec.finite_rows(states[1][0])) == 0   # first entry at the frame
        assert len(states[2]) == 3 and len(ec.finite_rows(states[2][0])) == 0                   # held in a full FIFO
        assert all(len(ec.finite_rows(s)) > 0 for s in states[3])                               # then evicted
    mid = ec.fifo_states(e["middle"], 3)
    assert any(len(s) == 3 and len(ec.finite_rows(s[1])) == 0 for s in mid)                     # in the middle
    assert any(len(a[0]) == 0 and all(x is not a[0] for x in b) for a, b in zip(mid[2:], mid[3:]))   # n = 0 evicted
    assert any(len(a[0]) > 0 and len(ec.finite_rows(a[0])) == 0 and all(x is not a[0] for x in b)
               for a, b in zip(mid[2:], mid[3:]))                                               # all-NaN evicted
    ni = ec.nan_interleaved(7)
    assert 0 < len(ec.finite_rows(ni)) < len(ni) and np.isfinite(ni[1, :3]).all()
    assert not np.isfinite(ni[::3, :3]).all(axis=1).any()


def test_clamped_sequences():
    """The frames are the device's: every counted push builds, so the first frame comes from scan 0
    alone (fifo_build, !fq_valid) and stays until a build sees clamped keys; the next build re-frames
    over the scans the FIFO then holds."""
    seq = [s for s, _ in ec.clamping_sequence()]

    def cube(scans):                                 # k_fifo_frame: [lo − ext/2, lo + 3·ext/2] on every axis
        m = ec.filtered_map(scans)
        lo, ext = m.min(axis=0), float(_ext(m).max())
        return m, lo - 0.5 * ext, lo + 1.5 * ext

    first, lo, hi = cube(seq[:1])                    # push 0's frame
    p1 = ec.filtered_map([seq[1]])
    assert (p1 >= lo).all() and (p1 <= hi).all()     # scan 1 fits: no re-frame before the far scans
    for k in (2, 3):                                 # outside it on all three axes
        p = ec.filtered_map([seq[k]])
        assert (p > hi).all() and len(p) > ec.MERGE_TILE
        assert len(np.unique(ec.model_keys(p, first))) == 1          # a whole run on one key, above a tile
    # the frame the far scans force — single: re-framed at push 3 over scans 1-3; paired (push 2 unbuilt,
    # push 3 builds both far runs under push 0's frame): re-framed at push 4 over scans 2-4
    for held in (seq[1:4], seq[2:5]):
        forced, lo, hi = cube(held)
        p = ec.filtered_map([seq[5]])
        assert (p < lo).all() and len(np.unique(ec.model_keys(p, forced))) == 1              # the negative faces
        p4 = ec.filtered_map([seq[4]])
        assert (p4 >= lo).all() and (p4 <= hi).all()                                         # scan 4 clamps nothing
    assert ec.CLAMP_PAIRED_UNCHECKED == (2,)
    d = ec.degenerate_frame_sequence()
    assert len(np.unique(d[0][0], axis=0)) == 1 and len(d[0][0]) == 500


def test_small_sources():
    src = ec._scan(1, 2500)
    for n in (ec.SMALL_ORDER_N - 1, ec.SMALL_ORDER_N, ec.SMALL_ORDER_N + 1):
        s = ec.small_source(src, n)
        _, counts = np.unique(s, axis=0, return_counts=True)
        assert len(s) == n and counts.max() == 1500 and (np.sort(counts)[:-1] == 1).all()
