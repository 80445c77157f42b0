"""Edge cases of the tensor-voting normals (csrc/tv.hip), shared by test_tv_cases.py — which proves on
numpy and the CPU oracle alone that every case reaches the edge it is named for — and
test_gpu_tv_edges.py, which runs them on the device.  No GPU imports.

A scene is a curved carrier sheet (z = Z0 + 0.15·sin(1.5x)·cos(1.2y) over [−3.2, 3.2]², 1,200 points,
tensors = the plate I − n·nᵀ of the analytic normal plus a random symmetric part) with features in the
plane z = 0 at slot centres 1.25 m apart (exact in float).  The carrier lies 0.6 to 0.9 m under the
features: farther than every voting radius ρ = thr·σ used here (≤ 0.3 m) and nearer than h = 1 m, so a
feature's query counts exactly the feature's points in its ball, has an NN-1 within h whatever the
feature holds, and has IMLS neighbours with count-mode normals (K = 5 within 1 m).  The angle gate is off.
Every target row has a random, distinct symmetric tensor unless the feature says otherwise, and the
target rows are shuffled: the index order is unrelated to position.

The source is a sample of carrier points moved by ≤ 0.02 m, in random order, with the features' subject
queries in the middle of it.  Every query is valid or rejected as no_normal (one named variant:
invalid_normal), so the voted normal of every row is compared or its absence is counted.

vote() is the restatement with switches: unmutated it equals imls_np.tv_normals (asserted by
test_tv_cases.py); the switches are the wrong variants of the sensitivity tests.
"""
import functools
import math
from dataclasses import dataclass, field

import numpy as np

import imls_np
import map_normals_cases as mc

EPS = float(np.finfo(np.float64).eps)
ULP = 2.0 ** -24                    # the float32 rounding of a normal's component
Z0 = -0.75
SLOT = 1.25
CARRIER_M = 1200
N_CARRIER_Q = 160
REJ_NO_NORMAL, REJ_INVALID = 0, 2
CAP = 256                           # tv.hip kTvCap
LIST = 64                           # internal.h kTvList
SLACK = np.float32(1.0) + np.float32(2e-6)      # tv.hip kTvSlack
JACOBI = 8.0                        # backward error of the 3×3 cyclic Jacobi, in units of ε·‖A‖_F
Y_TOL = 1e-5


def slot(i, j):
    return np.array([SLOT * i, SLOT * j, 0.0])


# ---- clouds ------------------------------------------------------------------------------------------
def sheet_z(x, y):
    return Z0 + 0.15 * np.sin(1.5 * x) * np.cos(1.2 * y)


def sheet_normal(x, y):
    gx = 0.15 * 1.5 * np.cos(1.5 * x) * np.cos(1.2 * y)
    gy = -0.15 * 1.2 * np.sin(1.5 * x) * np.sin(1.2 * y)
    n = np.stack([-gx, -gy, np.ones_like(gx)], axis=-1)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def sym6(rng, n, scale=1.0):
    """n random symmetric tensors (xx, xy, xz, yy, yz, zz), entries uniform in ±scale."""
    return rng.uniform(-scale, scale, (n, 6))


def plates(n3):
    n = np.asarray(n3, np.float64)
    return np.stack([1 - n[:, 0] * n[:, 0], -n[:, 0] * n[:, 1], -n[:, 0] * n[:, 2], 1 - n[:, 1] * n[:, 1],
                     -n[:, 1] * n[:, 2], 1 - n[:, 2] * n[:, 2]], axis=1)


@functools.lru_cache(maxsize=None)
def carrier(seed=101, M=CARRIER_M):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-3.2, 3.2, (M, 2))
    P = np.column_stack([xy, sheet_z(xy[:, 0], xy[:, 1])])
    T = plates(sheet_normal(xy[:, 0], xy[:, 1])) + sym6(rng, M, 0.2)
    return P.astype(np.float32), T.astype(np.float32)


def ball_points(rng, n, centre, rmax, rmin=0.01):
    """n points uniform in the shell rmin ≤ ‖p − centre‖ ≤ rmax."""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    r = (rng.uniform(rmin ** 3, rmax ** 3, n)) ** (1.0 / 3.0)
    return np.asarray(centre) + v * r[:, None]


def lattice2(half, s):
    """(2·half + 1)² points (i·s, j·s, 0) with s applied in float32: symmetric about the origin bit for bit."""
    a = (np.arange(-half, half + 1).astype(np.float32) * np.float32(s)).astype(np.float64)
    i, j = np.meshgrid(a, a, indexing="ij")
    return np.column_stack([i.ravel(), j.ravel(), np.zeros(i.size)])


# ---- scenes --------------------------------------------------------------------------------------------
@dataclass
class Subject:
    name: str
    q: np.ndarray                   # the query (source point; identity pose)
    category: str = "valid"         # valid | no_normal | invalid_normal
    count: object = None            # the named number of target points with dist < thr (None: not named)
    row: int = -1                   # its source row, set by Scene


@dataclass
class Scene:
    name: str
    sigma: float
    thr: float
    tgt: np.ndarray = None          # (M, 6) float32 rows, input order (may hold NaN rows)
    ten: np.ndarray = None          # (M, 6) float32 tensors, input order
    src: np.ndarray = None          # (N, 6) float32
    subjects: list = field(default_factory=list)
    carrier_rows: np.ndarray = None

    @property
    def rho(self):
        return self.thr * self.sigma

    def subject(self, name):
        return next(s for s in self.subjects if s.name == name)

    def filtered(self):
        """(P (M', 3) float64, T (M', 6) float64) after the NaN filter: the index order of the kNN."""
        keep = np.isfinite(self.tgt[:, :3]).all(axis=1)
        return self.tgt[keep, :3].astype(np.float64), self.ten[keep].astype(np.float64)


def build(name, sigma, thr, features, seed, nan_rows=(), n_carrier_q=N_CARRIER_Q, extra_src=None):
    """features: [(points (n, 3), tensors (n, 6) or None = random, [Subject])]."""
    rng = np.random.default_rng(seed)
    cp, ct = carrier()
    pts, tens, subs = [cp.astype(np.float64)], [ct.astype(np.float64)], []
    for P, T, ss in features:
        P = np.asarray(P, np.float64).reshape(-1, 3)
        pts.append(P)
        tens.append(sym6(rng, len(P)) if T is None else np.asarray(T, np.float64).reshape(-1, 6))
        subs += ss
    P, T = np.concatenate(pts), np.concatenate(tens)
    perm = rng.permutation(len(P))
    P, T = P[perm].astype(np.float32), T[perm].astype(np.float32)
    tgt = mc.map_rows(P)
    for at in nan_rows:             # NaN rows at input positions: the filtered index differs from the input's
        at = len(tgt) if at < 0 else at
        bad = np.full((1, 6), np.nan, np.float32)
        tgt = np.concatenate([tgt[:at], bad, tgt[at:]])
        T = np.concatenate([T[:at], sym6(rng, 1).astype(np.float32), T[at:]])
    cq = cp[rng.permutation(len(cp))[:n_carrier_q]].astype(np.float64) + rng.uniform(-0.02, 0.02, (n_carrier_q, 3))
    half = n_carrier_q // 2
    q = np.concatenate([cq[:half]] + [s.q.reshape(1, 3) for s in subs] + [cq[half:]])
    if extra_src is not None:
        q = np.concatenate([q, extra_src])
    src = np.zeros((len(q), 6), np.float32)
    src[:, :3] = q
    src[:, 5] = 1.0
    for k, s in enumerate(subs):
        s.row = half + k
    rows = np.r_[0:half, half + len(subs):len(q)]
    return Scene(name, sigma, thr, np.ascontiguousarray(tgt), np.ascontiguousarray(T), src, subs, rows)


def params(scene, k, iters=3):
    p = mc.params(5, 1.0, gate=False, iters=iters, tensor_voting=1)
    p.tensor_k, p.tensor_sigma, p.tensor_distance_threshold = int(k), float(scene.sigma), float(scene.thr)
    return p


BALL_KS = (1, 8, 50, 64)


def ball_sizes_of(k):
    return sorted({0, 1, k - 1, k, k + 1, 200, 256, 257, 300, 1000} - {-1})


@functools.lru_cache(maxsize=None)
def scene_ball(k):
    """One query each at the centre of a cluster of the named number of points inside ρ = 0.3."""
    rng = np.random.default_rng(200 + k)
    feats = []
    slots = [(i, j) for i in (-2, -1, 0, 1, 2) for j in (-2, -1, 0, 1, 2)]
    for n, (i, j) in zip(ball_sizes_of(k), slots):
        c = slot(i, j)
        feats.append((ball_points(rng, n, c, 0.28), None,
                      [Subject(f"ball-{n}", c, "valid" if n else "no_normal", n)]))
    return build(f"ball-sizes-k{k}", 1.0, 0.3, feats, 300 + k)


TIE_KS = (6, 50)
TIE_S = 0.0625                      # ties-at-k: 68 lattice points inside ρ
CUT_S = 0.03125                     # ties-at-the-cut: about 290
SPHERE_N2, SPHERE_UNIT = 1521, 256.0
NEAR_R, NEAR_M = 0.25, 400


@functools.lru_cache(maxsize=None)
def integer_sphere(n2=SPHERE_N2):
    """Every integer point (i, j, l) with i² + j² + l² = n2, over 256: one shell of exactly equal d² around
    its centre (the coordinates and their squares are exact in float and double)."""
    r = int(math.isqrt(n2))
    a = np.arange(-r, r + 1)
    i, j, l = np.meshgrid(a, a, a, indexing="ij")
    m = (i * i + j * j + l * l) == n2
    return np.column_stack([i[m], j[m], l[m]]) / SPHERE_UNIT


@functools.lru_cache(maxsize=None)
def scene_ties(nan=False):
    """Lattice patches in z = 0 — `tie-point` (the query on a lattice point) and `tie-centre` (on a cell
    centre) at spacing 1/16, `cut-point` and `cut-centre` at spacing 1/32 with more than 256 members inside
    ρ = 0.3: whole shells share one d² — and two shells that no arrival order can get past the cut whole:
    `cut-sphere`, the integer points of one sphere (more than 256 exactly tied members, so every cut's bound
    lies inside the shell and later members pass or fail by index), and `cut-near` at the origin, 400 points
    at 0.25 m in float32: distinct d² closer together than the fp32 screen resolves, so a bound without
    slack refuses members that beat it.  nan: NaN rows at the first, a middle and the last input position."""
    rng = np.random.default_rng(401)
    a, b, c, d, e = slot(1, 1), slot(-1, 1), slot(1, 0), slot(-1, -1), slot(1, -1)
    v = rng.normal(size=(NEAR_M, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    feats = [
        (lattice2(6, TIE_S) + a, None, [Subject("tie-point", a)]),
        (lattice2(6, TIE_S) + b, None, [Subject("tie-centre", b + np.array([TIE_S / 2, TIE_S / 2, 0.0]))]),
        (lattice2(10, CUT_S) + c, None, [Subject("cut-point", c)]),
        (lattice2(10, CUT_S) + d, None, [Subject("cut-centre", d + np.array([CUT_S / 2, CUT_S / 2, 0.0]))]),
        (integer_sphere() + e, None, [Subject("cut-sphere", e)]),
        (NEAR_R * v, None, [Subject("cut-near", np.zeros(3))]),
    ]
    return build("ties-nan" if nan else "ties", 1.0, 0.3, feats, 400, nan_rows=(0, 900, -1) if nan else ())


THR_KS = (5, 6, 7)
THR_NEAR = 4
F32_BELOW = float(np.nextafter(np.float32(0.25), np.float32(0.0)))
F32_ABOVE = float(np.nextafter(np.float32(0.25), np.float32(1.0)))


@functools.lru_cache(maxsize=None)
def scene_threshold():
    """σ = 0.5, thr = 0.5, the query at the origin: four voters within 0.2, then `below` at nextafter(0.25, 0)
    (votes), `on` at 0.25 exactly (dist == thr: a slot, no vote) and `above` at nextafter(0.25, 1) (inside
    the fp32 screen's slack, no vote).  k = 6: `on` takes the last slot; k = 5: it is cut itself."""
    rng = np.random.default_rng(500)
    near = ball_points(rng, THR_NEAR, np.zeros(3), 0.2, 0.05)
    edge = np.array([[0.0, F32_BELOW, 0.0], [0.25, 0.0, 0.0], [0.0, 0.0, F32_ABOVE]])
    return build("threshold-edge", 0.5, 0.5, [(np.concatenate([near, edge]), None, [Subject("thr", np.zeros(3), "valid", THR_NEAR + 1)])], 501)


SELF_K = 6


@functools.lru_cache(maxsize=None)
def scene_self():
    """The query at the origin; target points at the origin (d² = 0), at 1e-8 m (d² ≤ DBL_EPSILON: no slot)
    and at 2e-8 m (a slot and a vote), and five more voters: with k = 6 a slot given to either of the
    first two pushes the farthest voter out."""
    rng = np.random.default_rng(600)
    three = np.array([[0.0, 0.0, 0.0], [1e-8, 0.0, 0.0], [0.0, 2e-8, 0.0]])
    more = ball_points(rng, SELF_K - 1, np.zeros(3), 0.25, 0.05)
    return build("self-match", 1.0, 0.3, [(np.concatenate([three, more]), None, [Subject("self", np.zeros(3), "valid", SELF_K)])], 601)


MISC_K = 64
ZERO_T = np.array([1.0, 0.25, 0.5, 2.0, 0.125, 3.0])


def _one_voter_sum(r, T6):
    R = np.eye(3) - 2.0 * np.outer(r, r) / (r @ r)
    Rp = (np.eye(3) - 0.5 * np.outer(r, r) / (r @ r)) @ R
    T = np.array([[T6[0], T6[1], T6[2]], [T6[1], T6[3], T6[4]], [T6[2], T6[4], T6[5]]])
    return math.exp(-(r @ r)) * (R @ T @ Rp)


def lower(A):
    return np.tril(A) + np.tril(A, -1).T


def _abs_smallest_tensor():
    """An indefinite input tensor whose one vote (from (0.125, 0.0625, −0.125) off the query, σ = 1) has
    lower-triangle eigenvalues near (−3, 1, 2)·w: the smallest |λ| is not the smallest λ."""
    rng = np.random.default_rng(700)
    r = np.array([0.125, 0.0625, -0.125])
    while True:
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        T = Q @ np.diag([-6.0, 1.0, 2.0]) @ Q.T
        T6 = np.array([T[0, 0], T[0, 1], T[0, 2], T[1, 1], T[1, 2], T[2, 2]]).astype(np.float32).astype(np.float64)
        lam, U = np.linalg.eigh(lower(_one_voter_sum(r, T6)))
        a = int(np.argmin(np.abs(lam)))
        if a != 0 and lam[0] < -2.0 * abs(lam[a]) and abs(U[2, a]) > 0.2 and abs(U[2, 0]) > 0.2:
            return r, T6


@functools.lru_cache(maxsize=None)
def scene_misc():
    """k = 64, ρ = 0.3: duplicates (70 coincident points, one equal-d² group larger than k), the zero test's
    variants, a single indefinite voter, a visibly non-symmetric sum, and an overhang."""
    rng = np.random.default_rng(800)
    feats = []
    c = slot(-2, -2)
    feats.append((np.repeat((c + [0.0625, 0.125, 0.0])[None], 70, axis=0), None, [Subject("duplicates", c, "valid", 70)]))
    feats.append((np.zeros((0, 3)), None, [Subject("zero-empty", slot(-2, -1), "no_normal", 0)]))
    c = slot(-2, 0)
    feats.append((ball_points(rng, 5, c, 0.25, 0.05), np.zeros((5, 6)), [Subject("zero-tensors", c, "no_normal", 5)]))
    r = np.array([0.125, 0.0, -0.0625])
    m = np.abs(_one_voter_sum(r, ZERO_T)).max()
    s_rej = 2.0 ** round(math.log2(0.5e-12 / m))
    for nm, sc, cat, (i, j) in (("zero-below", s_rej, "no_normal", (-2, 1)), ("zero-above", 4 * s_rej, "valid", (-2, 2))):
        c = slot(i, j)
        feats.append(((c - r)[None], (sc * ZERO_T)[None], [Subject(nm, c, cat, 1)]))
    c = slot(-1, -2)
    r, T6 = _abs_smallest_tensor()
    feats.append(((c - r)[None], T6[None], [Subject("abs-smallest", c, "valid", 1)]))
    c = slot(-1, -1)
    feats.append((ball_points(rng, 2, c, 0.2, 0.1), None, [Subject("lower-triangle", c, "valid", 2)]))
    # the overhang: a slab above the query whose plates' normal (0.6, 0, −0.8) points down
    c = slot(-1, 0)
    n = np.array([0.6, 0.0, -0.8])
    u, v = np.array([0.8, 0.0, 0.6]), np.array([0.0, 1.0, 0.0])
    ab = rng.uniform(-0.2, 0.2, (30, 2))
    slab = c - 0.02 * n + ab[:, :1] * u + ab[:, 1:] * v
    feats.append((slab, plates(np.repeat(n[None], 30, axis=0)) + sym6(rng, 30, 0.05), [Subject("flip", c, "valid", 30)]))
    return build("misc", 1.0, 0.3, feats, 801)


OVERHANG = np.array([0.6, 0.0, -0.8])


@functools.lru_cache(maxsize=None)
def scene_nan_tensor():
    """One voter whose tensor holds a NaN entry: the sum is NaN, not zero, and the normal is not finite."""
    c = slot(0, 1)
    T = np.array([[1.0, np.nan, 0.5, 2.0, 0.125, 3.0]])
    return build("nan-tensor", 1.0, 0.3, [((c - [0.125, 0.0, -0.0625])[None], T, [Subject("nan-tensor", c, "invalid_normal", 1)])], 901)


@functools.lru_cache(maxsize=None)
def scene_big():
    """About 4,200 source rows (above kSmallRows = 4,096: the large-frame projection kernels read tvn)."""
    rng = np.random.default_rng(1000)
    cp, _ = carrier()
    extra = cp[rng.integers(0, len(cp), 4040)].astype(np.float64) + rng.uniform(-0.03, 0.03, (4040, 3))
    return build("big-frame", 1.0, 0.3, [], 1001, extra_src=extra)


def scene_small(n):
    """The first n carrier queries of the plain carrier scene (a block holds four queries)."""
    s = build(f"small-n{n}", 1.0, 0.3, [], 1100)
    s.src = np.ascontiguousarray(s.src[:n])
    s.carrier_rows = np.arange(n)
    return s


SMALL_N = (1, 2, 3, 5)


# (scene builder, its arguments, the k values it runs at)
PROJECT_CASES = (
    [("ball", scene_ball, (k,), (k,)) for k in BALL_KS]
    + [("ties", scene_ties, (False,), TIE_KS), ("ties-nan", scene_ties, (True,), TIE_KS),
       ("threshold", scene_threshold, (), THR_KS), ("self", scene_self, (), (SELF_K,)),
       ("misc", scene_misc, (), (MISC_K,)), ("nan-tensor", scene_nan_tensor, (), (MISC_K,))]
)
CASE_IDS = [f"{nm}{'-' + str(a[0]) if nm == 'ball' else ''}/k{k}" for nm, _, a, ks in PROJECT_CASES for k in ks]
CASE_LIST = [(fn, a, k) for _, fn, a, ks in PROJECT_CASES for k in ks]


# ---- the restatement with switches ---------------------------------------------------------------------------
@dataclass
class Vote:
    listed: np.ndarray              # the k slots (filtered indices), (d², index) order
    voters: np.ndarray              # the listed points that vote
    acc: np.ndarray                 # (3, 3) summed tensor
    found: bool
    n: np.ndarray                   # the normal ((0, 0, 0) when not found)
    lam: np.ndarray = None          # eigenvalues of the triangle read, ascending
    pick: int = -1
    bound: float = np.inf           # B_q
    stable: float = 0.0             # (second-smallest |λ| − smallest |λ|) / ‖A‖_F


def morton_rank(P):
    """A position order unrelated to the index order: the rank of a 3 × 10-bit Morton code of P."""
    lo, hi = P.min(axis=0), P.max(axis=0)
    g = np.minimum(((P - lo) / np.maximum(hi - lo, 1e-30) * 1024).astype(np.int64), 1023)
    code = np.zeros(len(P), np.int64)
    for b in range(10):
        for a in range(3):
            code |= ((g[:, a] >> b) & 1) << (3 * b + a)
    rank = np.empty(len(P), np.int64)
    rank[np.lexsort((np.arange(len(P)), code))] = np.arange(len(P))
    return rank


def knn_list(x, P, k, order="index", self_slot=False):
    d2 = imls_np.exact_d2(np.asarray(x, np.float64), P)
    cand = np.arange(len(P)) if self_slot else np.nonzero(d2 > EPS)[0]
    key = {"index": np.arange(len(P)), "reverse": -np.arange(len(P))}[order] if isinstance(order, str) else order
    return cand[np.lexsort((key[cand], d2[cand]))][:k]


def vote(x, P, T6, k, sigma, thr, listed=None, ge=True, order="index", self_slot=False, uplo="L", pick="abs"):
    """VoteForAny for one query (float-valued x), brute force.  Wrong variants: ge=False (`>` for `≥` at the
    threshold), order="reverse" or a position rank (ties), self_slot (the self match holds a slot),
    uplo="U", pick="min" (argmin λ); listed: a candidate list from a model of the cut or the skin list."""
    x = np.asarray(x, np.float32).astype(np.float64)
    if listed is None:
        listed = knn_list(x, P, k, order, self_slot)
    acc, delta, voters = np.zeros((3, 3)), 0.0, []
    for j in listed:
        r = x - P[j]
        nr = math.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
        dist = nr / sigma
        if dist <= 0.0 or (dist >= thr if ge else dist > thr):
            continue
        u = r / nr
        t = T6[j]
        T = np.array([[t[0], t[1], t[2]], [t[1], t[3], t[4]], [t[2], t[4], t[5]]])
        R = np.eye(3) - 2.0 * np.outer(u, u)
        S = math.exp(-(nr * nr) / sigma) * (R @ T @ ((np.eye(3) - 0.5 * np.outer(u, u)) @ R))
        acc += S
        delta += 4.0 * EPS * np.linalg.norm(S)
        voters.append(j)
    out = Vote(np.asarray(listed), np.asarray(voters, np.int64), acc, False, np.zeros(3))
    if np.all(np.abs(acc) <= 1e-12):
        return out
    if not np.isfinite(acc).all():          # a NaN sum is not zero: a normal is found, and it is not finite
        out.found, out.n = True, np.full(3, np.nan)
        return out
    lam, U = np.linalg.eigh(acc, UPLO=uplo)
    m = int(np.argmin(np.abs(lam))) if pick == "abs" else 0
    n = U[:, m] if U[2, m] >= 0 else -U[:, m]
    A = lower(acc) if uplo == "L" else lower(acc.T)
    nA = float(np.linalg.norm(A))
    gap = float(np.min(np.abs(np.delete(lam, m) - lam[m])))
    a = np.sort(np.abs(lam))
    out.found, out.n, out.lam, out.pick = True, n, lam, m
    out.bound = 2.0 * (delta + JACOBI * EPS * nA) / gap if gap > 0 else np.inf
    out.stable = float(a[1] - a[0]) / nA
    return out


def tol_of(v):
    return ULP + v.bound


def moved(a, b):
    """Whether vote b differs from vote a by more than 100 × a's tolerance, or in the found flag."""
    if a.found != b.found or np.isfinite(a.n).all() != np.isfinite(b.n).all():
        return True
    return bool(a.found and np.isfinite(a.n).all() and np.abs(a.n - b.n).max() > 100.0 * tol_of(a))


_VOTES = {}


def votes(scene, k, rows=None):
    """{source row: Vote} of the scene's queries at the identity pose (cached)."""
    key = (scene.name, k)
    if key not in _VOTES:
        P, T = scene.filtered()
        _VOTES[key] = {i: vote(scene.src[i, :3], P, T, k, scene.sigma, scene.thr) for i in range(len(scene.src))}
    return _VOTES[key]


def comparable(v):
    """The premise of the n comparison for one query: B_q ≤ 1e-7, a stable |λ| pick, n_z away from 0."""
    return v.found and np.isfinite(v.n).all() and v.bound <= 1e-7 and v.stable >= 1e-6 and v.n[2] > 100.0 * ULP


# ---- models of the kernel's buffer (for the sensitivity proofs only) ----------------------------------------------
def screen_d2(p, xf):
    """tv.hip screen_d2 in float32: fma(ex, ex, fma(ey, ey, ez·ez)) — the products are exact in double."""
    e = (np.asarray(p, np.float32) - np.asarray(xf, np.float32)).astype(np.float64)
    t = np.float32(e[..., 2] * e[..., 2]).astype(np.float64)
    t = np.float32(e[..., 1] * e[..., 1] + t).astype(np.float64)
    return np.float32(e[..., 0] * e[..., 0] + t)


def r2s_of(rho):
    return np.float32(np.float32(rho * rho) * SLACK + np.float32(1e-30))


def cut_walk(x, P, k, rho, arrival, tie_rule=True, slack=True):
    """The kernel's buffer: leaves of 64 in `arrival` order, members appended while they beat the bound
    (bk, bi) of the last cut; a buffer that would pass 256 is sorted and cut to the best k.  tie_rule=False:
    a later member must beat the bound's d² alone; slack=False: the fp32 screen bound after a cut is
    float(bk) without kTvSlack."""
    xf = np.asarray(x, np.float32)
    d2 = imls_np.exact_d2(xf.astype(np.float64), P)
    d32 = screen_d2(P, xf)
    r2s = r2s_of(rho)
    bnd, bk, bi, buf = r2s, np.inf, len(P), []

    def beats(j):
        return d2[j] < bk or (tie_rule and d2[j] == bk and j < bi)

    for a0 in range(0, len(arrival), 64):
        leaf = [j for j in arrival[a0:a0 + 64] if d32[j] <= bnd and d2[j] > EPS and beats(j)]
        if len(buf) + len(leaf) > CAP:
            buf = sorted(buf, key=lambda j: (d2[j], j))[:k]
            if len(buf) == k:
                bk, bi = d2[buf[-1]], buf[-1]
                f = np.float32(bk) * SLACK + np.float32(1e-30) if slack else np.float32(bk)
                bnd = min(r2s, np.float32(f))
            leaf = [j for j in leaf if beats(j) and (slack or d32[j] <= bnd)]
        buf += leaf
    return np.asarray(sorted(buf, key=lambda j: (d2[j], j))[:k], np.int64)


def skin_radius(rho, skin):
    """tv.hip: rs = √r2s·(1 + 1e-5) + skin and the screen bound rs²·(1 + 1e-5), in float32."""
    rs = np.float32(np.sqrt(r2s_of(rho))) * (np.float32(1.0) + np.float32(1e-5)) + np.float32(skin)
    return rs, np.float32(rs * rs * (np.float32(1.0) + np.float32(1e-5)))


def skin_count(x, P, rho, skin):
    """Members of the skin ball (self matches included) by the kernel's float32 expression."""
    return int((screen_d2(P, np.asarray(x, np.float32)) <= skin_radius(rho, skin)[1]).sum())


# ---- frames: skin lists over several iterations ------------------------------------------------------------------------
FRAME_K, FRAME_ITERS = 50, 5
SKINS = (0.0, 0.01, 0.03, 0.3, 1.0)
FRAME_MOTION = dict(yaw=0.004, pitch=-0.002, t=(0.05, -0.03, 0.02))


@functools.lru_cache(maxsize=None)
def scene_frame():
    """The carrier under a small rigid motion, with subjects crafted for the skin lists (skin 0.03 unless
    named): `list-64` / `list-65` (the skin ball at iteration 0 holds exactly 64 / 65 points, all within
    0.8 of the skin radius, none between 0.8 and 1.2 of it, at skins 0.01 and 0.03), `overflow-ball`
    (skin 0.3: skin ball above 256, ball proper below), `overflow-cut` (both above 256), and `self` — a
    source row equal to a target point at iteration 0 (identity) that has moved off it at iteration 1."""
    import model_restatement as mr
    rng = np.random.default_rng(1200)
    feats = []
    for n, (i, j) in ((64, (1, 1)), (65, (-1, 1))):
        c = slot(i, j)
        feats.append((ball_points(rng, n, c, 0.24, 0.02), None, [Subject(f"list-{n}", c, "valid")]))
    c = slot(1, -1)
    feats.append((np.concatenate([ball_points(rng, 100, c, 0.28), ball_points(rng, 200, c, 0.55, 0.36)]), None,
                  [Subject("overflow-ball", c, "valid")]))
    c = slot(-1, -1)
    feats.append((ball_points(rng, 400, c, 0.28), None, [Subject("overflow-cut", c, "valid")]))
    c = slot(0, 2)
    feats.append((np.concatenate([c[None], ball_points(rng, 20, c, 0.25, 0.05)]), None, [Subject("self", c, "valid")]))
    s = build("frame", 1.0, 0.3, feats, 1201, n_carrier_q=400)
    rows = s.carrier_rows
    s.src[rows] = mr.pose_cloud(s.src[rows], np.linalg.inv(mr.make_pose(**FRAME_MOTION)))
    s.src[:, 3:] = np.float32([0.0, 0.0, 1.0])
    return s


def frame_queries(scene, pose):
    """The float32 queries x = pose · source row (the oracle's expression: imls_np.project)."""
    T = np.asarray(pose, np.float64).reshape(4, 4)
    p = scene.src[:, :3].astype(np.float64)
    x = np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], axis=1)
    return x.astype(np.float32)


def reuse_plan(xs, skin):
    """Per iteration and query, whether the kernel walks (True) or screens its stored list (False), from
    the queries xs[it] (float32) alone — tv.hip's reference rule, lists that fit or not left aside."""
    ref = xs[0].copy()
    walks = [np.ones(len(ref), bool)]
    for x in xs[1:]:
        d = (x - ref).astype(np.float32)
        far = ~((d * d).sum(axis=1, dtype=np.float32) <= np.float32(skin) * np.float32(skin) * (np.float32(1.0) - np.float32(1e-4)))
        far |= skin <= 0.0
        ref[far] = x[far]
        walks.append(far)
    return np.array(walks)


# ---- batches, tensor inputs ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_scenes():
    """Members of N = 3, 257 and about 600 with different targets."""
    a = scene_small(3)
    rng = np.random.default_rng(1299)
    b = build("batch-257", 1.0, 0.3, [(ball_points(rng, 300, slot(0, 0), 0.28), None, [Subject("b-300", slot(0, 0))])], 1300,
              n_carrier_q=256)
    c = build("batch-601", 1.0, 0.3, [(ball_points(rng, 400, slot(1, 1), 0.28), None, [Subject("c-400", slot(1, 1))])], 1301,
              n_carrier_q=600)
    return [a, b, c]


def soa(rows):
    return np.ascontiguousarray(np.asarray(rows, np.float32).T)


# ---- the CPU oracle, cached ----------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_project(scene, k, pose=None, iters=3):
    """oracle_ctypes.project of the scene at `pose` (None: identity): (x, y, n, idx, rej)."""
    import oracle_ctypes as oc
    T = np.eye(4) if pose is None else np.asarray(pose, np.float64).reshape(4, 4)
    key = ("p", scene.name, len(scene.src), k, T.tobytes())
    if key not in _ORACLE:
        _ORACLE[key] = oc.project(soa(scene.src), soa(scene.tgt), T, params(scene, k, iters), tensors=soa(scene.ten))
    return _ORACLE[key]


def oracle_votes(scene, k, X=None):
    """oracle_ctypes.tv_normals at the queries X ((N, 3) float32; None: the source at the identity pose):
    (normals, found, summed tensors)."""
    import oracle_ctypes as oc
    X = scene.src[:, :3] if X is None else np.asarray(X, np.float32)
    key = ("v", scene.name, k, X.tobytes())
    if key not in _ORACLE:
        _ORACLE[key] = oc.tv_normals(soa(scene.tgt), soa(scene.ten), np.ascontiguousarray(X.T), params(scene, k))
    return _ORACLE[key]


def oracle_frame(scene, k=FRAME_K, iters=FRAME_ITERS):
    import oracle_ctypes as oc
    key = ("f", scene.name, k, iters)
    if key not in _ORACLE:
        _ORACLE[key] = oc.register_frame(soa(scene.src), soa(scene.tgt), params(scene, k, iters), tensors=soa(scene.ten))
    return _ORACLE[key]


def frame_poses(result):
    """The pose every iteration that ran projects at: identity, then the trace's pose after each iteration."""
    trace = list(result["trace"])
    return ([np.eye(4)] + [np.array(t.pose).reshape(4, 4) for t in trace])[:len(trace)]


def bounds_at(scene, k, X):
    """[Vote] of the restatement at the float32 queries X: B_q and the premises of the n comparison."""
    P, T = scene.filtered()
    return [vote(x, P, T, k, scene.sigma, scene.thr) for x in np.asarray(X, np.float32)]


def compare_normals(n, votes_of_rows, label):
    """The n comparison of one projection: n (float32 rows, device or oracle) against the restated votes of
    the same rows, |Δ| ≤ 2⁻²⁴ + B_q per component on the comparable rows.  Returns (largest ratio, rows
    left out)."""
    worst, left = 0.0, 0
    for row, v in zip(np.asarray(n, np.float64), votes_of_rows):
        if not comparable(v):
            left += 1
            continue
        worst = max(worst, float(np.abs(row - v.n).max() / tol_of(v)))
    return worst, left
