"""Edge cases of the index builders (shared by test_index_edge_cases.py, which proves on numpy alone
that each generator reaches the edge it is named for, and test_gpu_index_edges.py, which runs them on
the device).  No GPU imports.

The spatial index has three builders and one small-source path (csrc/index.hip, csrc/fifo_index.hip): the full build
(morton_perm → k_gather → k_leaf_boxes → k_subtree), the batched build (build_batch, the k_*_b
kernels), the incremental map-FIFO build (fifo_run_build, k_keep_*, k_merge_tile, k_fifo_gather, driven
by fifo_build in csrc/api_map.hip) and k_small_order.  An index that drops, doubles or mis-boxes one
point still gives a plausible pose, so the builders are pinned through the public exact kNN:

  reference  brute_knn: imls_np.exact_d2 (((dx²+dy²)+dz²) in double from the floats), the radius and
             self-match masks, np.lexsort((index, d2))[:k]; indices count the NaN-filtered
             concatenation, oldest scan first.  No tree of any kind: thousands of coincident points
             are exactly where a second tree is not independent evidence.
  census     every point of the filtered map queries k = 1, self-match allowed, radius +inf: the row
             is known without a search (d² = 0, idx = the lowest index among the point's exact
             duplicates).  An index that lost or replaced any single entry fails it.

Generators are seeded and deterministic; clouds are (M, 6) float32 rows x y z nx ny nz.
"""
import functools

import numpy as np

import imls_np

BLOCK = 256                 # internal.h kBlock: boxes per k_subtree block per round
MERGE_TILE = 2048           # fifo_index.hip kMergeTile: outputs per k_merge_tile block
MERGE_PER = MERGE_TILE // BLOCK
KEEP_TILE = 4096            # fifo_index.hip kKeepTile: entries per k_keep_* block
SMALL_ORDER_N = 2048        # index.h kSmallOrderN
LEAVES = (4, 64)


def rows6(xyz):
    """(M, 6) float32 rows from (M, 3) points, normals +z."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    out = np.zeros((len(xyz), 6), np.float32)
    out[:, :3] = xyz
    out[:, 5] = 1.0
    return out


def finite_rows(a6):
    a6 = np.asarray(a6, np.float32).reshape(-1, 6)
    return a6[np.isfinite(a6[:, :3]).all(axis=1)]


def filtered_map(scans):
    """(M, 3) float32: the NaN-filtered concatenation, oldest scan first (the index's numbering)."""
    if not len(scans):
        return np.zeros((0, 3), np.float32)
    return np.ascontiguousarray(finite_rows(np.concatenate([np.asarray(s, np.float32).reshape(-1, 6) for s in scans]))[:, :3])


# ---- the reference -------------------------------------------------------------------------------
def brute_knn_multi(P, q, configs):
    """[(idx (nq, k) int32, d2 (nq, k) float64)] for every (k, r, self_ok) of `configs`, one distance
    pass per query.  Candidates beyond the k-th smallest distance are cut before the lexsort (they
    cannot enter the first k of it); test_index_edge_cases.py checks the result against a full stable
    argsort."""
    P = np.ascontiguousarray(np.asarray(P, np.float32)[:, :3])
    q = np.asarray(q, np.float32)
    P64 = P.astype(np.float64)
    out = [(np.full((len(q), k), -1, np.int32), np.full((len(q), k), np.inf)) for k, _, _ in configs]
    for i, x in enumerate(q):
        d2_all = imls_np.exact_d2(x[:3], P64)
        for (k, r, self_ok), (idx, d2o) in zip(configs, out):
            m = d2_all <= float(r) * float(r)
            if not self_ok:
                m &= d2_all > np.finfo(np.float64).eps
            ii = np.nonzero(m)[0]
            d2 = d2_all[ii]
            if len(ii) > 4 * k:
                keep = d2 <= np.partition(d2, k - 1)[k - 1]
                ii, d2 = ii[keep], d2[keep]
            o = np.lexsort((ii, d2))[:k]
            idx[i, : len(o)] = ii[o]
            d2o[i, : len(o)] = d2[o]
    return out


def brute_knn(P, q, k, r=np.inf, self_ok=True):
    return brute_knn_multi(P, q, [(k, r, self_ok)])[0]


def census(P):
    """(idx (M, 1) int32, d2 (M, 1) float64) of knn(P, k=1, r=+inf, self-match allowed): no search."""
    P = np.asarray(P, np.float32)[:, :3]
    if len(P) == 0:
        return np.zeros((0, 1), np.int32), np.zeros((0, 1))
    # (+0.0 so that −0.0 and 0.0, at distance 0 from each other, fall in one group)
    _, first, inv = np.unique(P + np.float32(0.0), axis=0, return_index=True, return_inverse=True)
    return first[np.asarray(inv).reshape(-1)].astype(np.int32).reshape(-1, 1), np.zeros((len(P), 1))


PROBE_CONFIGS = ((20, 3.0, False), (32, np.inf, True))


def probes(P, n=500, seed=0):
    """n float32 queries: half jittered map points, the rest uniform in and just outside the bbox."""
    P = np.asarray(P, np.float32)[:, :3]
    rng = np.random.default_rng(seed)
    h = n // 2
    jit = P[rng.integers(0, len(P), h)] + rng.normal(0.0, 0.05, (h, 3)).astype(np.float32)
    lo, hi = P.min(axis=0).astype(np.float64), P.max(axis=0).astype(np.float64)
    pad = 0.1 * (hi - lo) + 0.5
    uni = rng.uniform(lo - pad, hi + pad, (n - h, 3))
    return np.ascontiguousarray(np.concatenate([jit.astype(np.float32), uni.astype(np.float32)]))


# ---- tree shape ----------------------------------------------------------------------------------
def tree_shape(M, B):
    """(leaves L, padded leaves P, levels, [boxes per block of every k_subtree round])."""
    L = (M + B - 1) // B
    P, levels = 1, 0
    while P < L:
        P <<= 1
        levels += 1
    rounds, count = [], P
    while count > 1:
        width = min(count, BLOCK)
        rounds.append(width)
        count //= width
    return L, P, levels, rounds


# ---- degenerate geometry (full and batched builds) --------------------------------------------------
def _rng(name):
    return np.random.default_rng(hash_name(name))


def hash_name(name):
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


def identical(n):
    return np.repeat(np.array([[1.25, -2.5, 0.75]], np.float32), n, axis=0)


def line_4096():
    r = _rng("line")
    xyz = np.empty((4096, 3), np.float32)
    xyz[:, 0] = r.uniform(-50, 50, 4096)
    xyz[:, 1], xyz[:, 2] = 1.25, -0.5
    return xyz


def plane_4096():
    r = _rng("plane")
    xyz = r.uniform(-20, 20, (4096, 3)).astype(np.float32)
    xyz[:, 2] = 0.75
    return xyz


FAR_CENTRE = (1e5, -1e5, 3e4)


def far_offset_4096():
    """2 m of extent at 1e5 m, generated in float32: x and y land on the 2⁻⁷ m grid."""
    r = _rng("far")
    return (np.array(FAR_CENTRE, np.float32)[None, :] + r.uniform(-1, 1, (4096, 3)).astype(np.float32)).astype(np.float32)


def sliver_4096():
    r = _rng("sliver")
    xyz = r.uniform(0, 1e-3, (4096, 3)).astype(np.float32)
    xyz[:, 0] = r.uniform(0, 1000, 4096)
    return xyz


def duplicate_groups():
    """5 distinct points × 2,400 copies plus 3,000 uniform points, shuffled."""
    r = _rng("dups")
    five = r.uniform(-5, 5, (5, 3)).astype(np.float32)
    xyz = np.concatenate([np.repeat(five, 2400, axis=0), r.uniform(-8, 8, (3000, 3)).astype(np.float32)])
    return xyz[r.permutation(len(xyz))]


GEOMETRY = {
    "identical_200": lambda: identical(200),
    "identical_2400": lambda: identical(2400),
    "line_4096": line_4096,
    "plane_4096": plane_4096,
    "far_offset_4096": far_offset_4096,
    "sliver_4096": sliver_4096,
    "duplicate_groups": duplicate_groups,
}
# cases whose kd-tree in the CPU oracle stays shallow: the oracle is asserted to agree with the brute
# force on them (the others — thousands of coincident points — give it deep degenerate trees)
ORACLE_OK = ("line_4096", "plane_4096", "far_offset_4096", "sliver_4096")

SIZE_EDGES = {4: (3, 4, 5, 1023, 1024, 1025, 1028, 1029, 262144, 262145), 64: (16384, 16385)}
BIG = 100000                # maps above this: 300 probes and a 20,000-point census sample
# (P, rounds) every size edge must give (issue: one round, 256-then-2, two full rounds, three rounds)
SIZE_SHAPES = {(4, 3): (1, []), (4, 4): (1, []), (4, 5): (2, [2]), (4, 1023): (256, [256]), (4, 1024): (256, [256]),
               (4, 1025): (512, [256, 2]), (4, 1028): (512, [256, 2]), (4, 1029): (512, [256, 2]),
               (4, 262144): (65536, [256, 256]), (4, 262145): (131072, [256, 256, 2]),
               (64, 16384): (256, [256]), (64, 16385): (512, [256, 2])}


@functools.lru_cache(maxsize=None)
def geometry(name):
    a = GEOMETRY[name]()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def uniform_cloud(M):
    a = np.random.default_rng(M).uniform(-50, 50, (M, 3)).astype(np.float32)
    a.setflags(write=False)
    return a


# ---- FIFO push sequences: lists of (scan (n, 6) float32, "host" | "device") ----------------------------
def _scan(seed, n, centre=(0.0, 0.0, 0.0), half=10.0):
    r = np.random.default_rng(seed)
    return rows6(np.asarray(centre, np.float32)[None, :] + r.uniform(-half, half, (n, 3)).astype(np.float32))


TIE_POINTS = np.array([[1.5, 2.5, -0.5], [-3.25, 0.75, 1.0], [4.0, -4.0, 0.25], [0.125, 0.5, -2.0], [-1.0, -1.0, 3.0]],
                      np.float32)


def tie_scan(seed):
    """The same 5 points × 800 copies plus 1,500 points of the scan's own, shuffled."""
    r = np.random.default_rng(1000 + seed)
    a = np.concatenate([rows6(np.repeat(TIE_POINTS, 800, axis=0)), _scan(2000 + seed, 1500)])
    return a[r.permutation(len(a))]


def ties_sequence():
    """Queue 3: three tied scans, then a 4th and a 5th (compaction over tied runs).  Every cross-run
    group of equal points has 3 × 800 = 2,400 > 2,048 members: a tile diagonal lies inside it."""
    return [(tie_scan(k), "host") for k in range(5)]


def stationary_sequence(queue):
    s = _scan(77, 3000)
    return [(s, "host")] * (queue + 2)


def id_wrap_sequence():
    s = _scan(77, 3000)                 # the stationary scan: the references are shared
    return [(s, "host")] * 70


# sizes of the size sequence (queue 3); test_index_edge_cases.py asserts which edges they visit
SIZE_SEQUENCE = (1, 2047, 2048, 2, 2045, 2051, 2046, 40000, 1)


def size_sequence(first="host"):
    """Host and device pushes alternate, starting with `first` (the two filter from different buffers:
    both parities together reach every size edge through both)."""
    kinds = ("host", "device") if first == "host" else ("device", "host")
    return [(_scan(300 + k, n), kinds[k % 2]) for k, n in enumerate(SIZE_SEQUENCE)]


def fifo_trace(sizes, queue):
    """Per build of a FIFO that builds after every push (kept sizes `sizes`): dict(old = entries of the
    previous merged order, the input of the compaction; kept = of them still live; new; total;
    compacts; grows = the order buffers must be reallocated whatever a recycled buffer's slack
    (api.hip grow: request + 25 % + 256, a recycled buffer at most 4× that)).  Assumes a fresh context:
    the order buffers start empty (imls_map_clear keeps a used context's buffers, of unknown size)."""
    fifo, out, old, cap = [], [], 0, 0
    for n in sizes:
        fifo.append(n)
        evicted = fifo.pop(0) if len(fifo) > queue else 0
        kept = old - evicted
        total = kept + n
        need = total * 8 + 64
        grows = cap > 0 and need > cap
        out.append(dict(old=old, kept=kept, new=n, total=total, compacts=old > 0 and kept != old, grows=grows and old > 0 and kept > 0))
        cap = max(cap, 4 * (need + need // 4 + 256))
        old = total
    return out


def nan_interleaved(seed, n=2500):
    a = _scan(seed, n)
    a[::3, seed % 3] = np.nan
    a[5, 0] = np.inf
    return a


def empty_scan():
    return np.zeros((0, 6), np.float32)


def all_nan_scan(n=300):
    a = _scan(5, n)
    a[:, 1] = np.nan
    return a


def empties_sequences():
    """name → push sequence (queue 3).  first_n0 / first_nan: the empty entry is the first push (no
    target), the first entry when the frame is computed (push 2), in the middle, and the entry evicted
    (push 4).  middle: both kinds pushed between ordinary scans, each evicted later, and a scan with NaN
    rows interleaved, so that the concatenated indices renumber across runs."""
    A = [_scan(400 + k, 2000 + 37 * k) for k in range(8)]
    return {
        "first_n0": [(empty_scan(), "host"), (A[0], "host"), (A[1], "device"), (A[2], "host"), (A[3], "host")],
        "first_nan": [(all_nan_scan(), "device"), (A[0], "host"), (A[1], "host"), (A[2], "device"), (A[3], "host")],
        "first_n0_device": [(empty_scan(), "device"), (A[4], "device"), (A[5], "host")],
        "middle": [(A[0], "host"), (empty_scan(), "host"), (all_nan_scan(), "host"), (A[1], "host"),
                   (nan_interleaved(7), "device"), (A[2], "host"), (nan_interleaved(8), "host"), (A[3], "host")],
    }


# pushes of clamping_sequence() made count-less and unchecked in the "paired" variant: the two far scans
# then meet in ONE build under the old frame — two whole runs on one key, tied across runs (built after
# every push, the second far scan is keyed under the frame its predecessor forced)
CLAMP_PAIRED_UNCHECKED = (2,)


def clamping_sequence():
    """Queue 3: two scans far outside the frame on all three axes (every key of the run equal),
    ordinary scans, then one outside the negative faces of the frame the far scans forced."""
    far = (500.0, 500.0, 500.0)
    neg = (-500.0, -500.0, -500.0)
    return [(_scan(500, 2500), "host"), (_scan(501, 2500), "host"), (_scan(502, 2500, far), "host"),
            (_scan(503, 2500, far), "device"), (_scan(504, 2500), "host"), (_scan(505, 2500, neg), "host"),
            (_scan(506, 2500), "host"), (_scan(507, 2500), "host")]


def degenerate_frame_sequence():
    """The first scan is 500 copies of one point (frame extent floored at 1e-6): everything after clamps."""
    first = rows6(np.repeat(np.array([[2.0, -1.0, 0.5]], np.float32), 500, axis=0))
    return [(first, "host")] + [(_scan(600 + k, 2200), "host") for k in range(4)]


def fifo_states(seq, queue):
    """The scans a FIFO of `queue` entries holds after each push of `seq` (oldest first)."""
    fifo, out = [], []
    for scan, _ in seq:
        fifo.append(scan)
        if len(fifo) > queue:
            fifo.pop(0)
        out.append(list(fifo))
    return out


# ---- a numpy model of the tiled merge path (fifo_index.hip merge_split_at / k_merge_tile) -----------------
def model_keys(P, frame_of):
    """48-bit Morton keys of (n, 3) float32 points under the FIFO frame of `frame_of` (k_fifo_frame's
    cube: side 2 × the largest extent, origin half an extent below the bbox).  Equal points get equal
    keys under any frame, which is all the tie cases rely on: the device keeps the frame of the build
    that last (re-)framed the FIFO — its first build's scans, not `frame_of` as the callers here pass it."""
    lo, hi = frame_of.min(axis=0).astype(np.float32), frame_of.max(axis=0).astype(np.float32)
    ext = np.float32(max(float((hi - lo).max()), 1e-6))
    org = lo - np.float32(0.5) * ext
    sc = np.float32(65535.0) / (np.float32(2.0) * ext)
    u = np.clip((np.asarray(P, np.float32) - org) * sc, 0, 65535).astype(np.uint64)
    key = np.zeros(len(P), np.uint64)
    for b in range(16):
        for d in range(3):
            key |= ((u[:, d] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + d)
    return key


def _le(a, b, strict):
    return a < b if strict else a <= b


def _split(a, b, d, strict):
    lo, hi = max(0, d - len(b)), min(d, len(a))
    while lo < hi:
        mid = (lo + hi) >> 1
        if _le(a[mid], b[d - 1 - mid], strict):
            lo = mid + 1
        else:
            hi = mid
    return lo


def tiled_merge(ak, av, bk, bv, tile_strict=False, thread_strict=False, take_strict=False):
    """merge(A, B) as k_merge_tile computes it: tile splits on the diagonals, per-thread splits inside
    the tile, MERGE_PER sequential outputs per thread; A first on equal keys unless a rule is flipped to
    strict.  Returns (keys, values); an output nobody wrote stays −1."""
    ak, bk = [int(x) for x in ak], [int(x) for x in bk]
    na, nb = len(ak), len(bk)
    okey, oval = [-1] * (na + nb), [-1] * (na + nb)
    for d0 in range(0, na + nb, MERGE_TILE):
        d1 = min(d0 + MERGE_TILE, na + nb)
        i0, i1 = _split(ak, bk, d0, tile_strict), _split(ak, bk, d1, tile_strict)
        j0, j1 = d0 - i0, d1 - i1
        sk = ak[i0:i1] + bk[j0:j1]
        sv = list(av[i0:i1]) + list(bv[j0:j1])
        la, lb = i1 - i0, j1 - j0
        n = la + lb
        for q in range(0, n, MERGE_PER):
            x = _split(sk[:la], sk[la:], q, thread_strict)
            y = q - x
            for r in range(q, min(q + MERGE_PER, n)):
                take_a = y >= lb or (x < la and _le(sk[x], sk[la + y], take_strict))
                src = x if take_a else la + y
                okey[d0 + r], oval[d0 + r] = sk[src], sv[src]
                x, y = x + take_a, y + (not take_a)
    return okey, oval


def model_fifo_merge(scans, **rules):
    """The merged order of the runs of `scans` (oldest first), each run stably sorted by key, merged
    one after the other into the order so far.  Returns (values, the stable sort's values); a value is
    (run, position in the run's sorted order).  Keys under the frame of the first scan alone, as on the
    device when every push builds (fifo_build frames the FIFO at its first build and keeps the frame
    while no key clamps: the scans here fit it)."""
    frame = filtered_map(scans[:1])
    keys = [model_keys(filtered_map([s]), frame) for s in scans]
    runs = []
    for r, k in enumerate(keys):
        o = np.argsort(k, kind="stable")
        runs.append(([int(x) for x in k[o]], [(r, j) for j in range(len(o))]))
    mk, mv = [], []
    for rk, rv in runs:
        mk, mv = tiled_merge(mk, mv, rk, rv, **rules)
    allk = np.array([k for rk, _ in runs for k in rk], np.uint64)
    allv = [v for _, rv in runs for v in rv]
    want = [allv[i] for i in np.argsort(allk, kind="stable")]
    return mv, want


# ---- small source order ----------------------------------------------------------------------------
def small_source(src_rows, n, seed=0):
    """n source rows of which 1,500 are one repeated row of `src_rows`, the rest distinct rows of it."""
    r = np.random.default_rng(seed + n)
    src_rows = finite_rows(src_rows)
    pick = r.choice(len(src_rows), n - 1500 + 1, replace=False)
    a = np.concatenate([np.repeat(src_rows[pick[:1]], 1500, axis=0), src_rows[pick[1:]]])
    assert len(a) == n
    return np.ascontiguousarray(a[r.permutation(n)])
