"""numpy restatement of the pose-info report (include/imls_gpu.h `struct imls_pose_info`), the DRPM
probabilities (degeneracy.h:14-131 as oracle/imls_oracle.cpp solve_drpm states them) and the RANSAC
inlier selection (solver.cpp:222-364 as the oracle's solve_ransac), for tests/test_pose_info_model.py
(CPU) and tests/test_gpu_pose_info.py (device).  No GPU imports.

Every per-row expression is evaluated in the order the solver uses (solver.cpp:95-110: the products
of a row are added left to right), so a row's a, b, |r₁| and residual carry the same bits as on the
device; only the association of the sums over rows differs, which is what the tests' bounds allow.
"""
import math

import numpy as np

import oracle_ctypes as oc
from planetary_lidar_odometry_amd import _abi

EPS = 2.2e-16
RANK_RELTOL = _abi.IMLS_INFO_RANK_RELTOL


def rows_ab(s, d, n):
    """(a (N,6), b (N,)) of the point-to-plane rows, as Rows::get / plane_row evaluate them."""
    s, d, n = (np.asarray(v, dtype=np.float64).reshape(-1, 3) for v in (s, d, n))
    a = np.empty((len(s), 6))
    a[:, 0] = n[:, 2] * s[:, 1] - n[:, 1] * s[:, 2]
    a[:, 1] = n[:, 0] * s[:, 2] - n[:, 2] * s[:, 0]
    a[:, 2] = n[:, 1] * s[:, 0] - n[:, 0] * s[:, 1]
    a[:, 3:] = n
    b = n[:, 0] * (d[:, 0] - s[:, 0])
    b = b + n[:, 1] * (d[:, 1] - s[:, 1])
    b = b + n[:, 2] * (d[:, 2] - s[:, 2])
    return a, b


def dot_seq(a, x):
    """a·x per row, the products added left to right (solver.cpp:110)."""
    v = a[:, 0] * x[0]
    for k in range(1, 6):
        v = v + a[:, k] * x[k]
    return v


def solve_x(a, b, w=None):
    """The least-squares x of the (√w-scaled) rows by the oracle's column-pivoted Householder QR."""
    if w is not None:
        sw = np.sqrt(w)
        a, b = a * sw[:, None], b * sw
    return oc.colpiv_qr_solve(a, b)


def trim_ranks(n_rows, t):
    lo = int(t * float(n_rows))
    hi = min(int((1 - t) * float(n_rows)), n_rows - 1)
    return lo, hi


def trim_members(a, b, x0, t):
    """Rows of ranks ⌊t·N⌋ … min(⌊(1−t)·N⌋, N−1) in the order (|r₁|, row), ascending by row; and the
    sorted |r₁| with the two ranks (for the premise checks)."""
    r1 = np.abs(dot_seq(a, x0) - b)
    order = np.lexsort((np.arange(len(b)), r1))
    lo, hi = trim_ranks(len(b), t)
    return np.sort(order[lo:hi + 1]), r1[order], lo, hi


def boundary_gap(sorted_r1, lo, hi, scale=None):
    """The smallest gap between a boundary rank's |r₁| and its neighbours, relative to median |r₁|
    (scale None) or to `scale`."""
    gaps = []
    for k in (lo, hi):
        if k - 1 >= 0:
            gaps.append(sorted_r1[k] - sorted_r1[k - 1])
        if k + 1 < len(sorted_r1):
            gaps.append(sorted_r1[k + 1] - sorted_r1[k])
    return (min(gaps) / (np.median(sorted_r1) if scale is None else scale)) if gaps else np.inf


def row_scale(a, b, x0):
    """The magnitude at which a rounding-level change of x₀ moves a row's residual: median of
    Σ|a_k·x₀_k| + |b|.  A gap measured against median |r₁| says nothing when the first solve fits its
    rows exactly (N = 6: every |r₁| is rounding noise, and so is their order)."""
    return float(np.median(np.abs(a * x0[None, :]).sum(1) + np.abs(b)))


def sym_eig(H, rel_tol=1e-30):
    """The oracle's cyclic Jacobi (imls_oracle.cpp sym_eig, DRPM's relative stop), operation for
    operation in Python floats: (ascending eigenvalues, U with U[k] = vector k)."""
    n = 6
    a = [[float(H[r][c]) for c in range(n)] for r in range(n)]
    v = [[1.0 if r == c else 0.0 for c in range(n)] for r in range(n)]
    fro = 0.0
    for r in range(n):
        for c in range(n):
            fro += a[r][c] * a[r][c]
    stop = max(1e-300, rel_tol * fro)
    for _ in range(100):
        off = 0.0
        for p in range(n):
            for q in range(p + 1, n):
                off += a[p][q] * a[p][q]
        if off < stop:
            break
        for p in range(n):
            for q in range(p + 1, n):
                apq = a[p][q]
                if apq == 0:
                    continue
                theta = (a[q][q] - a[p][p]) / (2 * apq)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1))
                c = 1 / math.sqrt(t * t + 1)
                s = t * c
                for k in range(n):
                    akp, akq = a[k][p], a[k][q]
                    a[k][p] = c * akp - s * akq
                    a[k][q] = s * akp + c * akq
                for k in range(n):
                    apk, aqk = a[p][k], a[q][k]
                    a[p][k] = c * apk - s * aqk
                    a[q][k] = s * apk + c * aqk
                for k in range(n):
                    vkp, vkq = v[k][p], v[k][q]
                    v[k][p] = c * vkp - s * vkq
                    v[k][q] = s * vkp + c * vkq
    diag = [a[k][k] for k in range(n)]
    order = sorted(range(n), key=lambda k: (diag[k], k))
    ev = np.array([diag[k] for k in order])
    U = np.array([[v[r][k] for r in range(n)] for k in order])
    return ev, U


def pin_sign(U):
    """Each vector's largest-magnitude component positive, the first such component on a tie."""
    U = np.array(U, dtype=np.float64, copy=True)
    for k in range(6):
        j = int(np.argmax(np.abs(U[k])))          # argmax returns the first maximum
        if U[k, j] < 0:
            U[k] = -U[k]
    return U


def spectrum(H, rss, n_rows):
    """eigenvalues, sign-pinned eigenvectors, rank, sigma2, covariance and the rank / dof flags of §1."""
    ev, U = sym_eig(H)
    U = pin_sign(U)
    kept = ev > RANK_RELTOL * ev[5]
    rank = int(kept.sum())
    flags = _abi.IMLS_INFO_VALID
    if rank < 6:
        flags |= _abi.IMLS_INFO_RANK_DEFICIENT
    sigma2, cov = 0.0, np.zeros((6, 6))
    if n_rows <= rank:
        flags |= _abi.IMLS_INFO_NO_DOF
    else:
        sigma2 = rss / (n_rows - rank)
        for k in range(6):
            if kept[k]:
                cov += np.outer(U[k], U[k]) / ev[k]
        cov *= sigma2
    return dict(eigenvalues=ev, eigenvectors=U, rank=rank, sigma2=sigma2, covariance=cov, flags=flags)


def sums(a, b, w, x):
    """hessian, gradient, btb, rss, weight_sum, n_rows over the given rows, and for each the sum of
    the absolute terms (`abs_*`: what the tests' 2·n·ε·Σ w|term| bounds are taken from)."""
    w = np.ones(len(b)) if w is None else np.asarray(w, dtype=np.float64)
    wa = w[:, None] * a
    terms_h = wa[:, :, None] * a[:, None, :]
    terms_g = wa * b[:, None]
    res = dot_seq(a, x) - b
    return dict(hessian=terms_h.sum(0), abs_hessian=np.abs(terms_h).sum(0),
                gradient=terms_g.sum(0), abs_gradient=np.abs(terms_g).sum(0),
                btb=float(((w * b) * b).sum()), rss=float(((w * res) * res).sum()),
                weight_sum=float(w.sum()), n_rows=len(b))


def report(a, b, w, x):
    """The whole restated report over rows that are already the final system's."""
    out = sums(a, b, w, x)
    out.update(spectrum(out["hessian"], out["rss"], out["n_rows"]))
    out["x"] = np.asarray(x, dtype=np.float64)
    out["drpm_probability"] = np.zeros(6)
    return out


def restate_ls(s, d, n, t):
    a, b = rows_ab(s, d, n)
    x0 = solve_x(a, b)
    keep, sorted_r1, lo, hi = trim_members(a, b, x0, t)
    x = solve_x(a[keep], b[keep])
    out = report(a[keep], b[keep], None, x)
    out.update(members=keep, x0=x0, gap=boundary_gap(sorted_r1, lo, hi),
               gap_scale=boundary_gap(sorted_r1, lo, hi, row_scale(a, b, x0)), trimmed=len(keep) < len(b))
    return out


def restate_ls_members(s, d, n, members):
    """The report of the second solve over the given rows (for a case whose trim order is rounding
    noise: the test finds the kept rows among the subsets)."""
    a, b = rows_ab(s, d, n)
    members = np.asarray(members)
    x = solve_x(a[members], b[members])
    out = report(a[members], b[members], None, x)
    out["members"] = members
    return out


def restate_wls(s, d, n, w=None):
    a, b = rows_ab(s, d, n)
    x = solve_x(a, b, w)
    out = report(a, b, w, x)
    out["members"] = np.arange(len(b))
    return out


# ---- DRPM (degeneracy.h:14-131 through oracle/imls_oracle.cpp solve_drpm) ---------------------------
def _skew(v):
    z = np.zeros(len(v))
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1), np.stack([v[:, 2], z, -v[:, 0]], 1),
                     np.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def drpm(s, d, n, w, threshold, sp, sn):
    """(probabilities in eigenvalue order, x, degenerate, H, g, eigenvalues, U) of solve_drpm."""
    s, d, n = (np.asarray(v, dtype=np.float64).reshape(-1, 3) for v in (s, d, n))
    w = np.ones(len(s)) if w is None else np.asarray(w, dtype=np.float64)
    a, b = rows_ab(s, d, n)
    sw = np.sqrt(w)
    aw, bw = a * sw[:, None], b * sw
    H = np.einsum("ir,ic->rc", aw, aw)
    g = aw.T @ bw
    ev, U = sym_eig(H)
    nx, px = _skew(n), _skew(s)
    N = len(s)
    B = np.zeros((N, 6, 6))
    B[:, :3, :3] = -nx
    B[:, :3, 3:] = px @ nx
    B[:, 3:, 3:] = nx
    nd = np.array([sp * sp] * 3 + [sn * sn] * 3)
    Cm = np.einsum("irk,k,ick->irc", B, nd, B) * w[:, None, None]
    mean = Cm.sum(0)
    v6 = np.concatenate([np.einsum("irk,ik->ir", px, n), n], 1) * sw[:, None]
    prob = np.zeros(6)
    for k in range(6):
        u = U[k]
        aa = np.einsum("r,irc,c->i", u, Cm, u)
        bb = v6 @ u
        var = float((2 * aa * aa + 4 * aa * bb * bb).sum())
        meas = float(u @ H @ u)
        exp_noise = float(u @ mean @ u)
        sd = math.sqrt(var) if var >= 0 else float("nan")
        tp = meas / (1.0 + 10.0)
        if any(math.isnan(v) for v in (exp_noise, sd, tp)):
            prob[k] = 0.0
        else:
            prob[k] = 0.5 * math.erfc(-(tp - exp_noise) / (sd * math.sqrt(2.0))) if sd > 0 else (1.0 if tp >= exp_noise else 0.0)
    degenerate = bool(prob.min() < threshold)
    if degenerate:
        dps = np.where(np.abs(ev) > 1e-10, prob / np.where(ev == 0, 1.0, ev), 0.0)
        x = U.T @ (dps * (U @ g))
    else:
        x = oc.colpiv_qr_solve(aw, bw)
    return dict(prob=prob, x=x, degenerate=degenerate, H=H, g=g, ev=ev, U=U)


def restate_drpm(s, d, n, w, p):
    r = drpm(s, d, n, w, p.drpm_threshold, p.drpm_stdev_points, p.drpm_stdev_normals)
    a, b = rows_ab(s, d, n)
    out = report(a, b, w, r["x"])
    out["drpm_probability"] = r["prob"]
    out["flags"] |= _abi.IMLS_INFO_DRPM_RAN | (_abi.IMLS_INFO_DRPM_DEGENERATE if r["degenerate"] else 0)
    out["members"] = np.arange(len(b))
    return out


# ---- RANSAC's inliers (solver.cpp:222-364 as the oracle's solve_ransac states them) -----------------
def ransac_inliers(s, d, n, p, state=None):
    """(inlier rows, their weights w / Σw, hypotheses drawn): the hypothesis loop on the glibc rand()
    stream `state` (int32[34], advanced in place; None: a fresh stream from p.ransac_seed)."""
    s, d, n = (np.asarray(v, dtype=np.float64).reshape(-1, 3) for v in (s, d, n))
    N = len(s)
    st = oc.rand_state(p.ransac_seed) if state is None else state
    nxt, ptr = oc.lib().oracle_rand_next, oc._ptr(st)
    a, b = rows_ab(s, d, n)

    def dist_all(T):
        tp = [((T[r, 0] * s[:, 0] + T[r, 1] * s[:, 1]) + T[r, 2] * s[:, 2]) + T[r, 3] for r in range(3)]
        return np.abs(((tp[0] - d[:, 0]) * n[:, 0] + (tp[1] - d[:, 1]) * n[:, 1]) + (tp[2] - d[:, 2]) * n[:, 2])

    def pdist(i):
        dx, dy, dz = s[:, 0] - s[i, 0], s[:, 1] - s[i, 1], s[:, 2] - s[i, 2]
        return np.sqrt((dx * dx + dy * dy) + dz * dz)

    min_inliers = int(p.ransac_min_inliers_percentage * float(N))
    best, bestT, draws = 0, np.eye(4), 0
    for _ in range(p.ransac_max_iterations):
        first = nxt(ptr) % N
        draws += 1
        ids = [first]
        md = pdist(first)
        for _k in range(2):
            m = md.copy()
            m[ids] = -np.inf
            far = int(np.argmax(m))               # the first maximum, as the oracle's strict >
            ids.append(far)
            md = np.minimum(md, pdist(far))
        x = oc.colpiv_qr_solve(a[ids], b[ids])
        T = oc.delta_from_x(x)
        cnt = int((dist_all(T) < p.ransac_distance_threshold).sum())
        if cnt > best:
            best, bestT = cnt, T
        if best > min_inliers:
            break
    dist = dist_all(bestT)
    inl = np.flatnonzero(dist < p.ransac_distance_threshold)
    h2 = p.ransac_huber_threshold * p.ransac_distance_threshold
    ar = np.exp(-np.abs(dist[inl]))
    w = np.where(np.sqrt(ar) < h2, ar, 2 * h2 * np.sqrt(ar) - h2 * h2)
    ws = w.sum()
    if ws > 0:
        w = w / ws
    return inl, w, draws


def restate_ransac(s, d, n, p, state=None):
    """The report of RANSAC → LS / weighted LS / DRPM on rows (s, d, n)."""
    s, d, n = (np.asarray(v, dtype=np.float64).reshape(-1, 3) for v in (s, d, n))
    inl, w, _ = ransac_inliers(s, d, n, p, state)
    si, di, ni = s[inl], d[inl], n[inl]
    if p.ransac_final_method == _abi.IMLS_FINAL_LS:
        out = restate_ls(si, di, ni, p.ransac_ls_threshold)
    elif p.ransac_final_method == _abi.IMLS_FINAL_WEIGHTED_LS:
        out = restate_wls(si, di, ni, w)
    else:
        out = restate_drpm(si, di, ni, w, p)
    out["inliers"] = inl
    out["members"] = inl[out["members"]]
    return out


# ---- poses ------------------------------------------------------------------------------------------
def exp_pose(xi):
    """Δ(ξ) as the solver forms it (solver.cpp:140-163): R = Rodrigues(ω), t = ξ[3:]."""
    return oc.delta_from_x(np.asarray(xi, dtype=np.float64))


def log_pose(T):
    """The inverse of exp_pose for rotations below π."""
    R, t = T[:3, :3], T[:3, 3]
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn = np.linalg.norm(v)
    ang = math.atan2(sn, (np.trace(R) - 1) / 2)
    w = v * (ang / sn) if sn > 1e-300 else v
    return np.concatenate([w, t])
