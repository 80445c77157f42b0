"""Edge cases of the IMLS matcher — the neighbour lists of csrc/knn_wave.hip and knn_qwave.hip, their fp64
certificate and the deferral to k_project_lane (finish.hip), the gates and the IMLS height
(exact_stage.h) — shared by test_matcher_cases.py, which proves on numpy and the CPU oracle alone that
every case reaches the edge it is named for, and test_gpu_matcher_edges.py, which runs them on the device.
No GPU imports.

A scene is a curved carrier sheet (z = −0.75 + 0.15·sin(1.5x)·cos(1.2y) over [−3.2, 3.2]², 1,200 points
that carry their analytic normals, get_normals = 1) with small features in the plane z = 0 at slot centres
1.25 m apart.  The sheet lies 0.6 to 0.9 m under the features — farther than every radius used beside it
(≤ 0.5 m) — so a feature's *subject* query sees the feature's points alone, and every feature point
carries a unit normal of its own: one neighbour swapped moves y.  Features whose radius is 1 m stand on
islands 7.5 m and more along x.  The map rows are shuffled (the index order is unrelated to position); the
source is a sample of carrier points moved by ≤ 0.02 m (the *background* queries, with the sheet's normal)
with the subjects in the middle of it.  The angle gate is off except where a case names it.

Every named equality is exact in fp64: subjects sit on slot centres, lattice features use power-of-two
units, and a point `on` a squared distance t is found by on_d2 — three float coordinates whose
((dx² + dy²) + dz²) rounds to t bit for bit.
"""
import functools
import math
from dataclasses import dataclass, field, replace

import numpy as np

import imls_np
import matcher_np as mp

EPS = mp.EPS
Z0, SLOT = -0.75, 1.25
CARRIER_M, N_CARRIER_Q = 1200, 100
Y_TOL = 1e-5                        # the projection's parity contract
POSE_TOL = 1e-6
COVERAGE = 0.95
MOVES = 100.0 * Y_TOL               # what a wrong variant must move y by
UNIT = 2.0 ** -6                    # lattice unit; the cell-centre lattices use odd multiples of UNIT / 2
FAR = np.array([1e5, -1e5, 512.0])  # float spacing 2⁻⁷ there
LIST_KL = {8: 12, 16: 20, 20: 22, 32: 36}           # project_common.h with_list_sizes
LONE_KL = {8: 22, 16: 30, 20: 32, 32: 46}           # … lone_kl
BIG_FRAME = 4096                    # internal.h kSmallRows


def slot(i, j=0):
    return np.array([SLOT * i, SLOT * j, 0.0])


def island(i):
    return np.array([7.5 + SLOT * i, 0.0, 0.0])


# ---- clouds ------------------------------------------------------------------------------------------
def sheet_z(x, y):
    return Z0 + 0.15 * np.sin(1.5 * x) * np.cos(1.2 * y)


def sheet_normal(x, y):
    gx = 0.15 * 1.5 * np.cos(1.5 * x) * np.cos(1.2 * y)
    gy = -0.15 * 1.2 * np.sin(1.5 * x) * np.sin(1.2 * y)
    n = np.stack([-gx, -gy, np.ones_like(gx)], axis=-1)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def carrier(seed=11, M=CARRIER_M):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-3.2, 3.2, (M, 2))
    P = np.column_stack([xy, sheet_z(xy[:, 0], xy[:, 1])])
    return P, sheet_normal(xy[:, 0], xy[:, 1])


def unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def cone_normals(rng, n, lo_deg, hi_deg):
    """Unit normals between lo and hi degrees off +z."""
    t = np.radians(rng.uniform(lo_deg, hi_deg, n))
    a = rng.uniform(0, 2 * np.pi, n)
    return np.column_stack([np.sin(t) * np.cos(a), np.sin(t) * np.sin(a), np.cos(t)])


def shell_points(rng, n, centre, rmin, rmax):
    return np.asarray(centre) + unit_vectors(rng, n) * rng.uniform(rmin, rmax, n)[:, None]


def on_d2(target, cx, sx=1.0, sy=1.0, sz=1.0):
    """A float32 point p beside the centre (cx, 0, 0) with imls_np.exact_d2(centre, p) == target bit for bit:
    dx takes what float spacing at cx allows, dy (≈ 1e-4) and dz (≈ 1e-7) the rest."""
    a = math.sqrt(target)
    px = np.float32(cx + sx * a)
    while (float(px) - cx) ** 2 > target:
        px = np.nextafter(px, np.float32(cx))
    dx = float(px) - cx
    py = np.float32(math.sqrt(max(target - dx * dx, 0.0)))
    for _ in range(64):
        while dx * dx + float(py) ** 2 > target:
            py = np.nextafter(py, np.float32(0.0))
        rem = target - (dx * dx + float(py) ** 2)
        pz = np.float32(math.sqrt(max(rem, 0.0)))
        for cand in [pz] + [np.nextafter(pz, np.float32(s)) for s in (0.0, 1.0)]:
            if (dx * dx + float(py) ** 2) + float(cand) ** 2 == target:
                p = np.array([float(px), sy * float(py), sz * float(cand)])
                assert imls_np.exact_d2(np.array([cx, 0.0, 0.0]), p[None])[0] == target
                return p
        py = np.nextafter(py, np.float32(0.0))
    raise AssertionError("no float point on the target distance")


def up(t):
    return float(np.nextafter(t, np.inf))


@functools.lru_cache(maxsize=None)
def int_vectors(R, odd):
    """Integer vectors with components in [−R, R] (odd: all three odd) and their squared lengths."""
    a = np.arange(-R, R + 1)
    a = a[a % 2 == 1] if odd else a
    i, j, l = np.meshgrid(a, a, a, indexing="ij")
    V = np.column_stack([i.ravel(), j.ravel(), l.ravel()])
    return V, (V * V).sum(axis=1)


# ---- scenes --------------------------------------------------------------------------------------------
@dataclass
class Subject:
    name: str
    q: np.ndarray
    cat: object = "valid"           # the category its case names; None: read from the oracle
    facts: dict = field(default_factory=dict)
    ns: tuple = (0.0, 0.0, 1.0)
    row: int = -1


@dataclass
class Scene:
    name: str
    par: mp.Par
    tgt: np.ndarray = None          # (M, 6) float32 map rows (points and stored normals)
    src: np.ndarray = None          # (N, 6) float32
    subjects: list = field(default_factory=list)
    carrier_rows: np.ndarray = None
    deferred: int = 0               # subjects no list can certify (a shell larger than the list)

    def subject(self, name):
        return next(s for s in self.subjects if s.name == name)


def build(name, par, feats, seed, n_carrier_q=N_CARRIER_Q, extra_src=0, shift=None, with_carrier=True, deferred=0):
    """feats: [(points (n, 3), normals (n, 3) or None = random unit vectors, [Subject], exact)] — exact:
    the points must be floats as given (asserted)."""
    rng = np.random.default_rng(seed)
    cp, cn = carrier()
    off = np.zeros(3) if shift is None else np.asarray(shift, np.float64)
    pts, nrm, subs = ([cp + off], [cn], []) if with_carrier else ([], [], [])
    for P, N, ss, exact in feats:
        P = np.asarray(P, np.float64).reshape(-1, 3) + off
        if exact:
            assert np.array_equal(P.astype(np.float32).astype(np.float64), P), name
        pts.append(P)
        nrm.append(unit_vectors(rng, len(P)) if N is None else np.asarray(N, np.float64).reshape(-1, 3))
        subs += [replace(s, q=np.asarray(s.q, np.float64) + off) for s in ss]
    P, N = np.concatenate(pts), np.concatenate(nrm)
    perm = rng.permutation(len(P))
    tgt = np.ascontiguousarray(np.column_stack([P[perm], N[perm]]).astype(np.float32))
    rows = []
    if with_carrier:
        inner = np.nonzero((np.abs(cp[:, 0]) < 2.7) & (np.abs(cp[:, 1]) < 2.7))[0]
        pick = inner[rng.integers(0, len(inner), n_carrier_q + extra_src)]
        cq = cp[pick] + rng.uniform(-0.02, 0.02, (len(pick), 3)) + off
        rows = np.column_stack([cq, cn[pick]])
    half = n_carrier_q // 2 if with_carrier else 0
    srows = np.array([np.r_[s.q, s.ns] for s in subs]).reshape(-1, 6)
    src = np.concatenate([rows[:half], srows, rows[half:]]) if with_carrier else srows
    for k, s in enumerate(subs):
        s.row = half + k
        assert np.array_equal(np.float32(s.q).astype(np.float64), s.q), (name, s.name)
    crow = np.r_[0:half, half + len(subs):len(src)] if with_carrier else np.zeros(0, np.int64)
    return Scene(name, par, tgt, np.ascontiguousarray(src.astype(np.float32)), subs, crow, deferred)


def with_big_source(scene, n=4200):
    """The same scene with background queries added up to n rows (above BIG_FRAME: one wave per query then
    goes through k_finish, not the fused kernel)."""
    rng = np.random.default_rng(len(scene.src))
    base = scene.src[scene.carrier_rows]
    k = rng.integers(0, len(base), n - len(scene.src))
    extra = base[k].copy()
    extra[:, :3] += rng.uniform(-0.03, 0.03, (len(k), 3)).astype(np.float32)
    s = replace(scene, name=scene.name + "/big", src=np.ascontiguousarray(np.concatenate([scene.src, extra])))
    s.carrier_rows = np.r_[scene.carrier_rows, len(scene.src):n]
    return s


def params(scene, iters=3):
    """ImlsParams of a scene: the shipped parameters with the LS solver, stored normals, the scene's matcher."""
    from planetary_lidar_odometry_amd import _abi, config
    a = scene.par
    p = config.bench_params(iters)
    p.get_normals, p.use_tensor_voting, p.use_projected_distance, p.transform_normal = 1, 0, 0, 0
    p.search_number, p.r, p.h = int(a.K), float(a.r), float(a.h)
    p.normal_angle_constraint, p.angle_diff_threshold = int(a.gate), float(a.thr)
    p.matching_method = _abi.IMLS_MATCH_IMLS if a.matcher == "imls" else _abi.IMLS_MATCH_PLANE_ICP
    p.picp_r, p.picp_r_proj = float(a.picp_r), float(a.picp_r_proj)
    p.picp_use_projected_distance = int(a.matcher == "picp_proj")
    p.picp_normal_angle_constraint, p.picp_angle_diff_threshold = int(a.picp_gate), float(a.picp_thr)
    return p


def soa(rows):
    return np.ascontiguousarray(np.asarray(rows, np.float32).T)


# ---- group 1: the K cut inside a shell -------------------------------------------------------------------
CUT_KS = (3, 8, 9, 16, 17, 20, 21, 32)
CUT_TIES = (("point", 1, 1), ("point", 2, 2), ("point", 3, 3), ("centre", 2, 1), ("centre", 1, 4), ("centre", 4, 2))
CUT_SLOTS = ((-2, -2), (0, -2), (2, -2), (-2, 2), (0, 2), (2, 2))


def cut_feature(rng, c, K, a, b, odd, name, unit=UNIT):
    """K − a lattice points just inside one shell, a + b members of the shell (the K-th and the (K + 1)-th
    neighbour among them: a of the tie inside the list, b outside, decided by index), six points beyond.
    odd: the query on a cell centre (odd multiples of unit / 2), else on a lattice point."""
    R, u = (49, unit / 2) if odd else (25, unit)
    V, n2 = int_vectors(R, odd)
    want = (0.375 / u) ** 2
    vals, counts = np.unique(n2, return_counts=True)
    ok = vals[(counts >= a + b) & (vals <= want)]
    cut = int(ok[-1])
    shell = V[n2 == cut][rng.permutation(int((n2 == cut).sum()))[:a + b]]
    lo = V[(n2 >= 0.88 * cut) & (n2 < cut)]
    inner = lo[rng.permutation(len(lo))[:K - a]]
    hi = V[(n2 > cut) & (n2 <= 1.2 * cut)]
    outer = hi[rng.permutation(len(hi))[:6]]
    P = c + np.concatenate([inner, shell, outer]) * u
    return (P, None, [Subject(name, c, "valid", dict(kcut_d2=cut * u * u, kcut_count=a + b, cut_in=a))], True)


@functools.lru_cache(maxsize=None)
def scene_cut(K, far=False):
    rng = np.random.default_rng(100 + K)
    feats = [cut_feature(rng, slot(i, j), K, a, b, kind == "centre", f"cut-{kind}-{a}+{b}")
             for (kind, a, b), (i, j) in zip(CUT_TIES, CUT_SLOTS) if a <= K]
    return build(f"cut-K{K}" + ("-far" if far else ""), mp.Par(K=K, r=0.5, h=1.0), feats, 200 + K, shift=FAR if far else None)


# ---- group 2: a shell larger than the list ---------------------------------------------------------------------
SHELL_KS = (8, 16, 20, 32)
SHELL_SIZES = (42, 56)              # above every KL (≤ 36); above every lone_kl (≤ 46)
SHELL_IN = 5


@functools.lru_cache(maxsize=None)
def scene_shell(K):
    rng = np.random.default_rng(300 + K)
    V, n2 = int_vectors(25, False)
    vals, counts = np.unique(n2, return_counts=True)
    cut = int(vals[(counts >= max(SHELL_SIZES)) & (vals <= 24 * 24)][-1])
    feats = []
    for size, (i, j) in zip(SHELL_SIZES, ((-1, -2), (1, 2))):
        c = slot(i, j)
        sphere = V[n2 == cut]
        shell = sphere[rng.permutation(len(sphere))[:size]]
        lo = V[(n2 >= 0.88 * cut) & (n2 < cut)]
        inner = lo[rng.permutation(len(lo))[:K - SHELL_IN]]
        feats.append((c + np.concatenate([inner, shell]) * UNIT, None,
                      [Subject(f"shell-{size}", c, "valid", dict(kcut_d2=cut * UNIT * UNIT, kcut_count=size, cut_in=SHELL_IN))], True))
    return build(f"shell-K{K}", mp.Par(K=K, r=0.5, h=1.0), feats, 400 + K, deferred=len(SHELL_SIZES))


# ---- group 3: distances fp32 cannot tell apart at the cut ------------------------------------------------------
KEY_KS = (8, 20)
KEY_KINDS = ("four", "id5", "id6")
KEY_M = 60


def key_points(kind, rng):
    """KEY_M float points about 0.25 m from the origin with distinct fp64 d².  four: their float keys take
    at most four values; id5 / id6: the keys share every bit above the low 5 / 6 mantissa bits (the id bits
    of the slot-id lists) and differ below."""
    v = unit_vectors(rng, 6000)
    if kind == "four":
        P = (0.25 * v).astype(np.float32).astype(np.float64)
        d2 = imls_np.exact_d2(np.zeros(3), P)
        keys = d2.astype(np.float32)
        vals, counts = np.unique(keys, return_counts=True)
        keep = np.isin(keys, vals[np.argsort(-counts)[:4]])
    else:
        bits = 5 if kind == "id5" else 6
        ulp = 2.0 ** -27                                # of a float in [2⁻⁴, 2⁻³)
        t = 0.0625 + rng.uniform(0.5, 2 ** bits - 0.5, len(v)) * ulp
        P = (np.sqrt(t)[:, None] * v).astype(np.float32).astype(np.float64)
        d2 = imls_np.exact_d2(np.zeros(3), P)
        keys = d2.astype(np.float32)
        keep = (keys >= np.float32(0.0625)) & (keys < np.float32(0.0625 + 2 ** bits * ulp))
    P, d2 = P[keep], d2[keep]
    _, first = np.unique(d2, return_index=True)
    P = P[np.sort(first)][:KEY_M]
    assert len(P) == KEY_M
    return P


@functools.lru_cache(maxsize=None)
def scene_keys(kind, K):
    rng = np.random.default_rng(500 + len(kind))
    P = key_points(kind, rng)
    s = Subject(f"keys-{kind}", np.zeros(3), "valid", dict(keys=kind))
    return build(f"keys-{kind}-K{K}", mp.Par(K=K, r=0.5, h=1.0), [(P, None, [s], True)], 600 + K, deferred=0)


# ---- group 4: the radius --------------------------------------------------------------------------------------------
RADII = (0.5, 0.3)
RADIUS_K = 8
UNDER_IN = 6


def radius_feature(rng, c, r, n_in, name, above_only=False):
    """n_in points between 0.3·r and 0.65·r (dropping the point on the radius then shrinks the bandwidth
    by a third and more: y moves by millimetres), one at d² == r² exactly (inside; left out with above_only),
    one at the next double above r² (outside) and four in (r, 1.05·r] (seen by the widened search only)."""
    r2 = r * r
    inner = shell_points(rng, n_in, c, 0.3 * r, 0.65 * r)
    edge = [on_d2(up(r2), c[0], -1.0, 1.0, -1.0)] + ([] if above_only else [on_d2(r2, c[0])])
    band = shell_points(rng, 4, c, 1.01 * r, 1.045 * r)
    within = n_in + (0 if above_only else 1)
    P = np.concatenate([inner, np.array(edge), band])
    # normals that lean outward (each its own): the height is then a weighted mean distance, which a lost
    # member or another bandwidth moves by millimetres whatever the seed
    N = (P - c) / np.linalg.norm(P - c, axis=1, keepdims=True) + 0.5 * unit_vectors(rng, len(P))
    return (P, N / np.linalg.norm(N, axis=1, keepdims=True),
            [Subject(name, c, "valid", dict(within_r=within, on_r=0 if above_only else 1, above_r=1, band=4))], False)


@functools.lru_cache(maxsize=None)
def scene_radius(r):
    """`under`: fewer than K points inside r, the farthest on the radius; `exact`: exactly K, the K-th on the
    radius; `above`: as `under` without the point on the radius (its twin one double above stays outside)."""
    rng = np.random.default_rng(700 + int(r * 10))
    K = RADIUS_K
    feats = [radius_feature(rng, slot(-2), r, UNDER_IN, "under"),
             radius_feature(rng, slot(0), r, K - 1, "exact"),
             radius_feature(rng, slot(2), r, UNDER_IN, "above", above_only=True)]
    feats[1][2][0].facts["kcut_d2"] = r * r
    return build(f"radius-r{r}", mp.Par(K=K, r=r, h=1.0), feats, 800 + int(r * 10))


@functools.lru_cache(maxsize=None)
def scene_radius_far():
    """The radius at (1e5, −1e5, 512), float spacing 2⁻⁷: neighbours on the axes at d² == r² = 0.25 and one
    spacing outside (d² = 0.25 + 2⁻¹⁴, inside the widened search), inner points on the 2⁻⁷ lattice."""
    rng = np.random.default_rng(900)
    u = 2.0 ** -7
    V, n2 = int_vectors(25, False)
    feats = []
    for name, n_in, c in (("under", UNDER_IN - 1, slot(-2)), ("exact", RADIUS_K - 2, slot(0))):
        lo = V[(n2 >= 60) & (n2 <= 250)] * 2
        inner = lo[rng.permutation(len(lo))[:n_in]]
        on = np.array([[64, 0, 0], [0, -64, 0]])
        out = np.array([[64, 1, 0], [0, 64, -1], [-64, 0, 2], [0, 3, 64]])
        facts = dict(within_r=n_in + 2, on_r=2, band=4)
        if name == "exact":
            facts["kcut_d2"] = 0.25
        feats.append((c + np.concatenate([inner, on, out]) * u, None, [Subject(name, c, "valid", facts)], True))
    return build("radius-far", mp.Par(K=RADIUS_K, r=0.5, h=1.0), feats, 901, shift=FAR)


# ---- group 5: the h gate ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_h():
    """h = 0.2 < r = 0.5: the NN-1 at d² == h² (kept) and at the next double above (too_far)."""
    rng = np.random.default_rng(1000)
    h2 = 0.2 * 0.2
    feats = []
    for name, t, cat, i in (("h-on", h2, "valid", -2), ("h-above", up(h2), "too_far", 2)):
        c = slot(i)
        P = np.concatenate([on_d2(t, c[0])[None], shell_points(rng, 6, c, 0.3, 0.45)])
        feats.append((P, None, [Subject(name, c, cat, dict(d1=t))], False))
    return build("h-gate", mp.Par(K=RADIUS_K, r=0.5, h=0.2), feats, 1001)


@functools.lru_cache(maxsize=None)
def scene_h3r1():
    """h = 3 > r = 1 (on islands): four points at d² == r² and nothing nearer — the NN-1 on the radius is
    kept — and four at the next double above: no NN-1 within r, too_far (Q18), although within h."""
    feats = []
    for name, t, cat, i in (("r-on", 1.0, "valid", 0), ("r-above", up(1.0), "too_far", 2)):
        c = island(i)
        P = np.array([on_d2(t, c[0], sx, sy, sz) for sx, sy, sz in ((1, 1, 1), (1, -1, 1), (-1, 1, -1), (-1, -1, -1))])
        feats.append((P, None, [Subject(name, c, cat, dict(d1=t) if cat == "valid" else dict(within_r=0))], False))
    return build("h-3-r-1", mp.Par(K=RADIUS_K, r=1.0, h=3.0), feats, 1101)


# ---- group 6: NN-1 and the self match ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_self():
    """The query at the origin, K = 8: map points at d² = 0, 1e-16 and DBL_EPSILON exactly (2⁻²⁶ m along −x)
    — skipped by NN-1, kept by the list —, two at d² = 4e-16 with different normals (the NN-1 candidates:
    the lower index gives n), two at 0.1 to 0.15 m and the 8th at 0.45 m (a wide bandwidth: the height is
    centimetres, so another n moves y)."""
    rng = np.random.default_rng(1200)
    tiny = np.array([[0.0, 0.0, 0.0], [1e-8, 0.0, 0.0], [-2.0 ** -26, 0.0, 0.0], [0.0, 2e-8, 0.0], [0.0, 0.0, 2e-8]],
                    np.float32).astype(np.float64)
    P = np.concatenate([tiny, shell_points(rng, 2, np.zeros(3), 0.1, 0.15), shell_points(rng, 1, np.zeros(3), 0.45, 0.45),
                        shell_points(rng, 2, np.zeros(3), 0.47, 0.48)])
    s = Subject("self", np.zeros(3), "valid", dict(nn1_ties=2, skipped=3, on_eps=1, d1=float(np.float32(2e-8)) ** 2))
    return build("self-match", mp.Par(K=8, r=0.5, h=1.0), [(P.astype(np.float32).astype(np.float64), None, [s], True)], 1201)


COPY_KS = (20, 32)
COPIES = 70


@functools.lru_cache(maxsize=None)
def scene_copies(K):
    """Seventy copies of the query's own point and five points at 0.3 m: a full list holds no NN-1
    (need = r²: no list certifies), and the bandwidth point is at d² = 0 (hmax = 0)."""
    rng = np.random.default_rng(1300 + K)
    c = slot(1, 1)
    P = np.concatenate([np.repeat(c[None], COPIES, axis=0), shell_points(rng, 5, c, 0.3, 0.3)])
    s = Subject("copies", c, None, dict(hmax0=True, kcut_count=COPIES))
    return build(f"copies-K{K}", mp.Par(K=K, r=0.5, h=1.0), [(P, None, [s], False)], 1301, deferred=1)


# ---- group 7: the accepted set and Q3 -------------------------------------------------------------------------------
NANS = np.full(3, np.nan)


def ring(rng, c, radii):
    return np.asarray(c) + unit_vectors(rng, len(radii)) * np.asarray(radii)[:, None]


@functools.lru_cache(maxsize=None)
def scene_accepted():
    """K = 8, gate off, list places by distance (0.10, 0.15, … 0.45 m unless named):
    acc-2 / acc-3: two / three finite normals; nan-places: a NaN normal at the first place (a copy of the
    query, so not the NN-1), a middle and the K-th; hmax-0: copies of the query at places 0 to 2, the third
    with a NaN normal, the NN-1 at place 3 and NaN normals behind: nacc = 3 and L[2] is at d² = 0;
    underflow: two NaN-normal copies, the bandwidth point L[2] at 1e-8 m, the others at 0.40 to 0.44 m."""
    rng = np.random.default_rng(1400)
    radii = 0.10 + 0.05 * np.arange(8)
    feats = []

    def feature(name, c, P, finite, cat, facts):
        N = unit_vectors(rng, len(P))
        N[~np.asarray(finite, bool)] = np.nan
        feats.append((P, N, [Subject(name, c, cat, facts)], False))

    c = slot(-2, -2)
    feature("acc-2", c, ring(rng, c, radii), [1, 0, 0, 1, 0, 0, 0, 0], "mls_fail", dict(acc=2))
    c = slot(0, -2)
    feature("acc-3", c, ring(rng, c, radii), [1, 0, 0, 1, 0, 0, 0, 1], "valid", dict(acc=3, acc_mask=0b10001001))
    c = slot(2, -2)
    feature("nan-places", c, np.concatenate([c[None], ring(rng, c, radii[:7])]), [0, 1, 1, 0, 1, 1, 1, 0], "valid",
            dict(acc=5, acc_mask=0b01110110))
    c = slot(-2, 2)
    feature("hmax-0", c, np.concatenate([np.repeat(c[None], 3, axis=0), ring(rng, c, radii[:5])]), [1, 1, 0, 1, 0, 0, 0, 0], None,
            dict(acc=3, hmax0=True))
    c = np.zeros(3)
    near = np.array([[1e-8, 0.0, 0.0]], np.float32).astype(np.float64)
    feature("underflow", c, np.concatenate([np.zeros((2, 3)), near, ring(rng, c, 0.40 + 0.01 * np.arange(5))]), [0, 0, 1, 1, 1, 0, 0, 0], "valid",
            dict(acc=3, hmax=float(np.float32(1e-8)) / 3))
    return build("accepted", mp.Par(K=8, r=0.5, h=1.0), feats, 1401)


@functools.lru_cache(maxsize=None)
def scene_accepted_gate():
    """K = 8 with the 30° angle gate on: places 2, 3 and 4 carry normals 50° to 70° off the query's, the
    others within 20°: nacc = 5, so hmax is read from L[4] — a rejected point at 0.30 m — not from the last
    accepted one at 0.45 m."""
    rng = np.random.default_rng(1500)
    c = slot(0, 0)
    P = ring(rng, c, 0.10 + 0.05 * np.arange(8))
    N = cone_normals(rng, 8, 2.0, 20.0)
    N[2:5] = cone_normals(rng, 3, 50.0, 70.0)
    s = Subject("gate-middle", c, "valid", dict(acc=5, acc_mask=0b11100011))
    return build("accepted-gate", mp.Par(K=8, r=0.5, h=1.0, gate=True), [(P, N, [s], False)], 1501)


# ---- group 8: small and odd maps ----------------------------------------------------------------------------------
SMALL_K = 8
SMALL_MS = (1, 2, 3, SMALL_K - 1, SMALL_K, SMALL_K + 1, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def scene_small(M, outside=False):
    """A map of M points in a 0.4 m box (outside: 5 m away from every query) and 40 queries in and around
    it; no carrier."""
    rng = np.random.default_rng(1600 + M)
    P = rng.uniform(-0.2, 0.2, (M, 3)) + (np.array([5.0, 0.0, 0.0]) if outside else 0.0)
    q = rng.uniform(-0.35, 0.35, (40, 3)).astype(np.float32).astype(np.float64)
    subs = [Subject(f"q{k}", q[k], "too_far" if outside else None) for k in range(len(q))]
    return build(f"small-M{M}" + ("-outside" if outside else ""), mp.Par(K=SMALL_K, r=0.5, h=1.0), [(P, None, subs, False)], 1700 + M,
                 with_carrier=False)


# ---- group 10: plane_ICP --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_picp():
    """picp_r = 0.5: two NN-1 candidates at one d² (the lower index gives p and n), the NN-1 on picp_r² and
    one double above it (no_normal), and a query with nothing near it (no_normal)."""
    rng = np.random.default_rng(1800)
    r2 = 0.25
    feats = []
    c = slot(0, 2)
    tie = c + np.array([[0.125, 0.25, 0.0], [-0.25, 0.125, 0.0], [0.0, -0.125, 0.25]])
    feats.append((np.concatenate([tie, shell_points(rng, 4, c, 0.35, 0.45)]), None, [Subject("picp-tie", c, "valid", dict(nn1_ties=3))], False))
    c = slot(-2)
    feats.append((on_d2(r2, c[0])[None], None, [Subject("picp-on", c, "valid", dict(d1=r2))], False))
    c = slot(2)
    feats.append((on_d2(up(r2), c[0])[None], None, [Subject("picp-above", c, "no_normal", dict(within_r=0))], False))
    feats.append((np.zeros((0, 3)), None, [Subject("picp-none", island(0), "no_normal", dict(within_r=0))], False))
    return build("plane-icp", mp.Par(matcher="picp", picp_r=0.5), feats, 1801)


@functools.lru_cache(maxsize=None)
def scene_picp_proj():
    """Projected-distance mode (candidates ‖p − x‖ < picp_r² and ‖(p − x) × n_s‖ < picp_r_proj): two
    candidates with the same projected distance 0.125 at different heights (the lower index wins), and a
    query with no candidate (too_far)."""
    rng = np.random.default_rng(1900)
    c = slot(0, 2)
    tie = c + np.array([[0.125, 0.0, 0.25], [0.0, 0.125, -0.125], [0.0, -0.125, 0.375]])
    more = c + np.column_stack([unit_vectors(rng, 4)[:, :2] * 0.25, rng.uniform(-0.1, 0.1, 4)])
    feats = [(np.concatenate([tie, more]), None, [Subject("proj-tie", c, "valid", dict(proj_ties=3))], False),
             (np.zeros((0, 3)), None, [Subject("proj-none", island(0), "too_far")], False)]
    return build("plane-icp-proj", mp.Par(matcher="picp_proj", picp_r=0.8, picp_r_proj=0.3), feats, 1901)


# ---- the case lists -----------------------------------------------------------------------------------------------------
# the first six groups: every path runs them
PATH_CASES = ([("cut", scene_cut, (K,)) for K in CUT_KS] + [("shell", scene_shell, (K,)) for K in SHELL_KS]
              + [("keys", scene_keys, (kind, K)) for kind in KEY_KINDS for K in KEY_KS]
              + [("radius", scene_radius, (r,)) for r in RADII]
              + [("h", scene_h, ()), ("h3r1", scene_h3r1, ()), ("self", scene_self, ())]
              + [("copies", scene_copies, (K,)) for K in COPY_KS])
OTHER_CASES = ([("accepted", scene_accepted, ()), ("accepted-gate", scene_accepted_gate, ())]
               + [("small", scene_small, (M,)) for M in SMALL_MS] + [("small-outside", scene_small, (20, True))]
               + [("cut-far", scene_cut, (20, True)), ("radius-far", scene_radius_far, ())]
               + [("picp", scene_picp, ()), ("picp-proj", scene_picp_proj, ())])


def case_id(c):
    return c[0] + "".join(f"-{a}" for a in c[2])


PATH_IDS = [case_id(c) for c in PATH_CASES]
OTHER_IDS = [case_id(c) for c in OTHER_CASES]


# ---- the frame: five iterations over the shell and radius features ------------------------------------------------------
FRAME_K, FRAME_ITERS = 20, 5
COPY_DIR = np.array([0.6, 0.0, 0.8])                # away from the carrier sheet
COPY_TIES = ((1, 1), (3, 1), (2, 2))                # with K − a nearer points, 1+1 and 3+1 end inside a 22-entry list


def cluster(rng, n, centre, half=0.004):
    return np.asarray(centre) + rng.uniform(-half, half, (n, 3))


def copy_feature(rng, c, K, a, b, name):
    """Ties that survive any pose: a + b coincident map points (each its own normal and index) 0.375 m from
    the query along COPY_DIR, K − a distinct points in an 8 mm cluster 0.355 m along the same direction and
    six more 0.40 m along it.  The three groups lie on one ray, so a query that moves by centimetres keeps
    their order (the directions to them differ by < 0.02 rad), the copies stay on the K-th and (K + 1)-th
    place with one d² bit for bit, and — every weight within e⁻⁸ … e⁻⁹ — one copy swapped moves y."""
    P = np.concatenate([cluster(rng, K - a, c + 0.355 * COPY_DIR), np.repeat((c + 0.375 * COPY_DIR)[None], a + b, axis=0),
                        cluster(rng, 6, c + 0.40 * COPY_DIR)])
    # the copies' normals fan out from COPY_DIR to 170° off it, so d·n differs by decimetres between any two:
    # which of them are listed shows in the height whatever the seed
    N = unit_vectors(rng, len(P))
    side = np.cross(COPY_DIR, [0.0, 1.0, 0.0])
    for k in range(a + b):
        t = np.radians(170.0 * k / (a + b - 1))
        N[K - a + k] = np.cos(t) * COPY_DIR + np.sin(t) * side / np.linalg.norm(side)
    return (P, N, [Subject(name, c, "valid", dict(kcut_count=a + b, cut_in=a, every_pose=True))], False)


def copy_nn1_feature(rng, c, K, name):
    """Three coincident points 0.10 m from the query as its NN-1 candidates (the lowest index gives n), K − 2
    in a cluster at 0.30 m: the copies carry nearly all the weight, the height is centimetres, so n moves y."""
    P = np.concatenate([np.repeat((c + 0.10 * COPY_DIR)[None], 3, axis=0), cluster(rng, K - 2, c + 0.30 * COPY_DIR)])
    return (P, None, [Subject(name, c, "valid", dict(nn1_ties=3, every_pose=True))], False)


@functools.lru_cache(maxsize=None)
def scene_frame():
    """One frame of 400 background queries moved by a small rigid motion (K = 20, r = 0.5), with two kinds
    of subject.  Lattice cuts, an integer-sphere shell and radius features stand at their edges at the
    identity pose of iteration 0 alone (the pose then moves the queries by centimetres and the lattice ties
    are gone).  Features of coincident map points keep their ties at every pose — copies on the K-th and
    (K + 1)-th place (1+1 and 3+1 end inside a 22-entry list, so k_finish's own tie rule decides them; 2+2
    fills it), 56 copies behind K − 5 nearer points (no list certifies, at any iteration) and three copies
    as the NN-1 candidates — so the lists that later iterations reuse, prefill or seed hold exact ties."""
    import model_restatement as mr
    K = FRAME_K
    rng = np.random.default_rng(2000)
    feats = [cut_feature(rng, slot(i, j), K, a, b, kind == "centre", f"cut-{kind}-{a}+{b}")
             for (kind, a, b), (i, j) in zip(CUT_TIES[1:5], CUT_SLOTS)]
    V, n2 = int_vectors(25, False)
    vals, counts = np.unique(n2, return_counts=True)
    cut = int(vals[(counts >= 56) & (vals <= 24 * 24)][-1])
    c = slot(1, 1)
    sphere = V[n2 == cut]
    lo = V[(n2 >= 0.88 * cut) & (n2 < cut)]
    feats.append((c + np.concatenate([lo[rng.permutation(len(lo))[:K - SHELL_IN]], sphere[rng.permutation(len(sphere))[:56]]]) * UNIT,
                  None, [Subject("shell-56", c, "valid", dict(kcut_count=56, cut_in=SHELL_IN))], True))
    feats.append(radius_feature(rng, slot(-2), 0.5, UNDER_IN, "under"))
    feats.append(radius_feature(rng, slot(2), 0.5, K - 1, "exact"))
    for (a, b), (i, j) in zip(COPY_TIES, ((0, 2), (2, 2), (0, 0))):
        feats.append(copy_feature(rng, slot(i, j), K, a, b, f"copy-cut-{a}+{b}"))
    feats.append(copy_feature(rng, slot(-1, -1), K, SHELL_IN, 56 - SHELL_IN, "copy-shell"))
    feats.append(copy_nn1_feature(rng, slot(-1, 1), K, "copy-nn1"))
    s = build("frame", mp.Par(K=K, r=0.5, h=1.0), feats, 2001, n_carrier_q=400, deferred=2)
    rows = s.carrier_rows
    s.src[rows] = mr.pose_cloud(s.src[rows], np.linalg.inv(mr.make_pose(yaw=0.004, pitch=-0.002, t=(0.03, -0.02, 0.015))))
    return s


def frame_poses(result):
    """The pose every iteration that ran projects at: identity, then the trace's pose after each iteration."""
    trace = list(result["trace"])
    return ([np.eye(4)] + [np.array(t.pose).reshape(4, 4) for t in trace])[:len(trace)]


# ---- references, cached -----------------------------------------------------------------------------------------------------
_ORACLE, _RESTATED = {}, {}


def _key(scene, pose):
    T = np.eye(4) if pose is None else np.asarray(pose, np.float64).reshape(4, 4)
    return (scene.name, len(scene.src), T.tobytes()), T


def oracle_project(scene, pose=None):
    """oracle_ctypes.project of the scene at `pose` (None: identity): (x, y, n, idx, rej)."""
    import oracle_ctypes as oc
    key, T = _key(scene, pose)
    if key not in _ORACLE:
        _ORACLE[key] = oc.project(soa(scene.src), soa(scene.tgt), T, params(scene))
    return _ORACLE[key]


def restated(scene, pose=None):
    """matcher_np.project of the scene at `pose`: (x, y, n, idx, rej, rows)."""
    key, T = _key(scene, pose)
    if key not in _RESTATED:
        _RESTATED[key] = mp.project(scene.src, scene.tgt, T, scene.par)
    return _RESTATED[key]


def oracle_frame(scene, iters=FRAME_ITERS):
    import oracle_ctypes as oc
    key = ("f", scene.name, iters)
    if key not in _ORACLE:
        _ORACLE[key] = oc.register_frame(soa(scene.src), soa(scene.tgt), params(scene, iters))
    return _ORACLE[key]


def by_row(result):
    """{source row: (y, n)} of a projection result."""
    x, y, n, idx = result[:4]
    return {int(r): (y[k], n[k]) for k, r in enumerate(idx)}


def category(result, row):
    """'valid' or 'rejected' of a source row in a five-tuple result (the oracle counts, it does not list)."""
    return "valid" if row in set(int(r) for r in result[3]) else "rejected"


def compare(got, want, label, y_tol=Y_TOL):
    """A projection `got` against a reference `want` under the project's contract: rej, idx, x and n equal,
    y within y_tol on every row.  Returns the largest |Δy|."""
    x, y, n, idx, rej = got[:5]
    wx, wy, wn, widx, wrej = want[:5]
    assert np.array_equal(np.asarray(rej, np.uint64), np.asarray(wrej, np.uint64)), (label, list(rej), list(wrej))
    assert np.array_equal(np.asarray(idx, np.int64), np.asarray(widx, np.int64)), label
    assert np.array_equal(x, wx), label
    same_n = (n == wn) | (np.isnan(n) & np.isnan(wn))
    assert same_n.all(), (label, idx[~same_n.all(axis=1)][:5])
    dy = float(np.abs(y.astype(np.float64) - wy.astype(np.float64)).max()) if len(idx) else 0.0
    assert dy <= y_tol, (label, dy)
    return dy
