"""The IMLS matcher restated with no tree: ProjSourcePtToSurface and plane_ICP_proj (direct and
projected-distance mode) in numpy, from the oracle's description (oracle/imls_oracle.h, Q1 … Q18), not from
the kernels.  TEST INFRASTRUCTURE ONLY.

Per query x = float(pose · p): the exact distances imls_np.exact_d2 to the whole filtered map, the masks
d² ≤ r² and — for NN-1 only — d² > DBL_EPSILON, the order np.lexsort((index, d²))[:K], then the gates in the
reference's order: no NN-1 → too_far (Q18), d1 > h² → too_far, the NN-1's normal not finite →
invalid_normal, the angle gate (NaN passes, Q8) → normal_constraint, fewer than 3 accepted list members →
mls_fail, h_max = √d²(L[nacc − 1]) / 3 (Q3: an index into the list, not into the accepted set), the sums in
list order, height = Σ / (Σw + 1e-5) (Q4), not finite → nan_inf_height, y = float(x − height · n_NN).

project() also returns what the premises of test_matcher_cases.py need, per query: the K-cut distance, the
number of map points on it, the number within r, the NN-1 index, the accepted set as a bit mask over list
places, and h_max.  variant= selects one wrong matcher (VARIANTS) for the sensitivity proofs.
"""
import math
from dataclasses import dataclass

import numpy as np

import imls_np

EPS = float(np.finfo(np.float64).eps)
NO_NORMAL, TOO_FAR, INVALID_NORMAL, NORMAL_CONSTRAINT, MLS_FAIL, NAN_INF = range(6)
VARIANTS = ("r_lt", "h_ge", "self_ge", "no_self_rule", "ties_position", "ties_highest", "q3_last", "nacc2",
            "cut_unstable", "list_nocert")


@dataclass
class Par:
    """The matcher's parameters (a plain mirror of the fields of ImlsParams that the matcher reads)."""
    K: int = 20
    r: float = 0.5
    h: float = 1.0
    gate: bool = False
    thr: float = 30.0
    matcher: str = "imls"           # imls | picp | picp_proj
    picp_r: float = 1.5
    picp_r_proj: float = 0.8
    picp_gate: bool = False
    picp_thr: float = 30.0


@dataclass
class Row:
    cat: int                        # −1 valid, else the reject category
    x: np.ndarray                   # float32 query
    y: np.ndarray = None
    n: np.ndarray = None
    nn1: int = -1                   # filtered index of the NN-1 (−1: none)
    d1: float = np.inf
    kcut_d2: float = np.inf         # the K-th list distance (∞: fewer than K within r)
    kcut_count: int = 0             # map points at exactly that distance
    within_r: int = 0
    listed: np.ndarray = None       # the list (filtered indices), (d², index) order
    acc_mask: int = 0               # bit j: list place j accepted
    hmax: float = np.nan


def angle_reject(ns, n, thr):
    dot = (ns[0] * n[0] + ns[1] * n[1]) + ns[2] * n[2]
    a = math.sqrt((ns[0] * ns[0] + ns[1] * ns[1]) + ns[2] * ns[2])
    b = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    with np.errstate(all="ignore"):
        ca = np.float64(dot) / np.float64(a * b)
        ang = np.arccos(ca) * 180.0 / math.pi
    return bool(ang > thr)          # NaN: False, the neighbour passes


def position_rank(P):
    """An order by position unrelated to the index order (a 3 × 10-bit Morton code, ties by −index)."""
    lo, hi = P.min(axis=0), P.max(axis=0)
    g = np.minimum(((P - lo) / np.maximum(hi - lo, 1e-30) * 1024).astype(np.int64), 1023)
    code = np.zeros(len(P), np.int64)
    for b in range(10):
        for a in range(3):
            code |= ((g[:, a] >> b) & 1) << (3 * b + a)
    rank = np.empty(len(P), np.int64)
    rank[np.lexsort((-np.arange(len(P)), code))] = np.arange(len(P))
    return rank


def transform(T, p):
    return np.array([((T[r, 0] * p[0] + T[r, 1] * p[1]) + T[r, 2] * p[2]) + T[r, 3] for r in range(3)]).astype(np.float32)


def filtered(rows):
    rows = np.asarray(rows, np.float32).reshape(-1, 6)
    return rows[np.isfinite(rows[:, :3]).all(axis=1)]


def project(src, tgt, pose, par, variant=None, kl=None):
    """src (N, 6), tgt (M, 6) float32 rows.  Returns (x, y, n, idx, rej, rows): the first five as
    oracle_ctypes.project, rows = [Row] of every filtered source row.  variant: one of VARIANTS
    (list_nocert takes kl, the list length)."""
    assert variant is None or variant in VARIANTS
    S, G = filtered(src), filtered(tgt)
    P, NR = G[:, :3].astype(np.float64), G[:, 3:].astype(np.float64)
    M = len(P)
    T = np.eye(4) if pose is None else np.asarray(pose, np.float64).reshape(4, 4)
    index = np.arange(M)
    tie = index
    if variant == "ties_highest":
        tie = -index
    elif variant in ("ties_position", "list_nocert") and M:
        tie = position_rank(P)
    elif variant == "cut_unstable":
        tie = np.random.default_rng(7).permutation(M)
    r2 = par.r * par.r
    rej = np.zeros(6, np.uint64)
    rows = []
    for i in range(len(S)):
        xf = transform(T, S[i, :3].astype(np.float64))
        x = xf.astype(np.float64)
        ns = S[i, 3:].astype(np.float64)
        row = Row(-1, xf)
        rows.append(row)
        d2 = imls_np.exact_d2(x, P) if M else np.zeros(0)
        if par.matcher != "imls":
            _plane(row, x, ns, d2, P, NR, index, par)
        else:
            _imls(row, x, ns, d2, P, NR, index, tie, r2, par, variant, kl)
        if row.cat >= 0:
            rej[row.cat] += 1
    ok = [k for k, w in enumerate(rows) if w.cat < 0]
    as3 = lambda a: np.asarray(a, np.float32).reshape(-1, 3)
    return (as3([rows[k].x for k in ok]), as3([rows[k].y for k in ok]), as3([rows[k].n for k in ok]),
            np.asarray(ok, np.uint32), rej, rows)


def _imls(row, x, ns, d2, P, NR, index, tie, r2, par, variant, kl):
    inr = (d2 < r2) if variant == "r_lt" else (d2 <= r2)
    row.within_r = int(inr.sum())
    cand = np.nonzero(inr)[0]
    order = cand[np.lexsort((tie[cand], d2[cand]))]
    if variant == "list_nocert" and len(order) > kl:
        # the float traversal's list: the best kl by distance, ties in arrival order; taken for the answer
        # without asking whether a point outside it ties with its bound
        order = order[:kl]
        order = order[np.lexsort((index[order], d2[order]))]
    # NN-1: no self match
    if variant == "no_self_rule":
        nn = order
    elif variant == "self_ge":
        nn = order[d2[order] >= EPS]
    else:
        nn = order[d2[order] > EPS]
    if len(nn) == 0:
        row.cat = TOO_FAR               # Q18
        return
    row.nn1, row.d1 = int(nn[0]), float(d2[nn[0]])
    h2 = par.h * par.h
    if (row.d1 >= h2) if variant == "h_ge" else (row.d1 > h2):
        row.cat = TOO_FAR
        return
    nn_n = NR[row.nn1]
    if not np.isfinite(nn_n).all():
        row.cat = INVALID_NORMAL
        return
    if par.gate and angle_reject(ns, nn_n, par.thr):
        row.cat = NORMAL_CONSTRAINT
        return
    L = order[:par.K]
    row.listed = L
    if len(L) == par.K:
        row.kcut_d2 = float(d2[L[-1]])
        row.kcut_count = int((d2 == row.kcut_d2).sum())
    acc = []
    for j, m in enumerate(L):
        if not np.isfinite(NR[m]).all():
            continue
        if par.gate and angle_reject(ns, NR[m], par.thr):
            continue
        acc.append(m)
        row.acc_mask |= 1 << j
    if len(acc) < (2 if variant == "nacc2" else 3):
        row.cat = MLS_FAIL
        return
    with np.errstate(all="ignore"):
        dsel = d2[acc[-1]] if variant == "q3_last" else d2[L[len(acc) - 1]]          # Q3
        hmax = np.float64(math.sqrt(dsel)) / 3
        row.hmax = float(hmax)
        ws = ps = np.float64(0.0)
        for m in acc:
            d = x - P[m]
            dn = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            w = np.exp(-dn / hmax / hmax)
            ps = ps + (((w * d[0]) * NR[m, 0] + (w * d[1]) * NR[m, 1]) + (w * d[2]) * NR[m, 2])
            ws = ws + w
        height = ps / (ws + 1e-5)                                                     # Q4
    if not math.isfinite(height):
        row.cat = NAN_INF
        return
    row.y = (x - height * nn_n).astype(np.float32)
    row.n = nn_n.astype(np.float32)


def _plane(row, x, ns, d2, P, NR, index, par):
    """plane_ICP_proj: NN-1 within picp_r (no self match; unfound → no_normal) or, in projected-distance
    mode, the smallest ‖(p − x) × n_s‖ (then the lower index) among ‖p − x‖ < picp_r² — the reference's
    swapped gate — and ‖(p − x) × n_s‖ < picp_r_proj (none → too_far); no h gate; y = x − ((x − p)·n)·n."""
    if par.matcher == "picp_proj":
        d = P - x
        c = np.stack([d[:, 1] * ns[2] - d[:, 2] * ns[1], d[:, 2] * ns[0] - d[:, 0] * ns[2], d[:, 0] * ns[1] - d[:, 1] * ns[0]], axis=1)
        pr = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        dn = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        cand = np.nonzero((dn < par.picp_r * par.picp_r) & (pr < par.picp_r_proj))[0]
        if len(cand) == 0:
            row.cat = TOO_FAR
            return
        best = int(cand[np.lexsort((index[cand], pr[cand]))][0])
    else:
        cand = np.nonzero((d2 <= par.picp_r * par.picp_r) & (d2 > EPS))[0]
        row.within_r = len(cand)
        if len(cand) == 0:
            row.cat = NO_NORMAL
            return
        best = int(cand[np.lexsort((index[cand], d2[cand]))][0])
    row.nn1, row.d1 = best, float(d2[best])
    n = NR[best]
    if not np.isfinite(n).all():
        row.cat = INVALID_NORMAL
        return
    if par.picp_gate and angle_reject(ns, n, par.picp_thr):
        row.cat = NORMAL_CONSTRAINT
        return
    v = x - P[best]
    pd = (v[0] * n[0] + v[1] * n[1]) + v[2] * n[2]
    row.y = (x - pd * n).astype(np.float32)
    row.n = n.astype(np.float32)
