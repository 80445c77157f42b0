"""csrc/normals.hip restated in numpy with no tree of any kind: the recomputed ("count mode") normal of
every map point, get_normals = 0 and recompute_normal_count_mode = 1 (ComputeNormal, imls_icp.cpp:753-794,
over the kNN-search_number_normal within r_normal of the point itself, self match excluded).

For map point i of the NaN-filtered map P (float32 rows, the index's numbering):
  neighbours  d² = imls_np.exact_d2(P[i], P) — ((dx²+dy²)+dz²) in double from the floats — masked by
              d² ≤ r² (inclusive, r² = r·r in double) and d² > DBL_EPSILON (the self match and every exact
              copy of the point), ordered by np.lexsort((index, d²)), the first K taken;
  too few     fewer than K neighbours: the normal is (∞, ∞, ∞);
  moments     the fp64 mean (the sum in list order, / K) and the covariance (outer products summed in
              list order, / K);
  normal      np.linalg.eigh — LAPACK, not the Jacobi sweeps the device and the oracle share — the unit
              eigenvector of the smallest eigenvalue, flipped to z ≥ 0.

The neighbour lists are the independent evidence (brute force); the eigenvector is evidence where the
two smallest eigenvalues are separated: an error E of the covariance moves it by about ‖E‖ / (λ1 − λ0),
so with fp64 moments (‖E‖ of a few eps·λ2) a relative gap (λ1 − λ0) / λ2 ≥ GAP = 1e-6 leaves 1e-9 or
less, far under the float32 rounding of the result (half an ulp at 1.0, 2⁻²⁴).  Where the gap is
smaller (K = 1: C = 0; K = 2 and collinear lists: λ0 = λ1 = 0) every unit vector of the span of the two
smallest eigenvectors is as good an answer; what can be held against any n there is residual():
‖C·n‖ ≤ λ1 + λ2·(√3·2⁻²⁴ + 64·eps) — a unit vector of that span has ‖C·n‖ ≤ λ1, its rounding to float32
moves it by at most √3·2⁻²⁴ (half an ulp per component, components below 1), which C stretches by at
most λ2, and 64·eps·λ2 stands for the fp64 sweeps.
"""
import numpy as np

import imls_np

DBL_EPS = np.finfo(np.float64).eps
GAP = 1e-6
ULP1 = 2.0 ** -23               # one float32 ulp at 1.0


def neighbour_lists(P, K, r, highest_index_first=False, strict_radius=False):
    """[K-or-fewer indices] per map point, ordered (d², index).  The two flags are the mutations the
    CPU tests hold the cases against (ties by the highest index; d² < r²), never used otherwise."""
    P = np.ascontiguousarray(np.asarray(P, np.float32)[:, :3])
    P64 = P.astype(np.float64)
    r2 = float(r) * float(r)
    idx = np.arange(len(P))
    out = []
    for i in range(len(P)):
        d2 = imls_np.exact_d2(P[i], P64)
        m = ((d2 < r2) if strict_radius else (d2 <= r2)) & (d2 > DBL_EPS)
        ii, dd = idx[m], d2[m]
        if len(ii) > 4 * K:                 # beyond the K-th distance nothing enters the first K
            keep = dd <= np.partition(dd, K - 1)[K - 1]
            ii, dd = ii[keep], dd[keep]
        o = np.lexsort((-ii if highest_index_first else ii, dd))[:K]
        out.append(ii[o])
    return out


def moments(P, lists, K):
    """(mean (M, 3), covariance (M, 3, 3)) in fp64, summed in list order; rows with a short list: NaN."""
    P64 = np.asarray(P, np.float32)[:, :3].astype(np.float64)
    M = len(P64)
    mu, C = np.full((M, 3), np.nan), np.full((M, 3, 3), np.nan)
    for i, li in enumerate(lists):
        if len(li) < K:
            continue
        s = np.zeros(3)
        for j in li:
            s = s + P64[j]
        s = s / K
        c = np.zeros((3, 3))
        for j in li:
            v = P64[j] - s
            c = c + np.outer(v, v)
        mu[i], C[i] = s, c / K
    return mu, C


def map_normals(P, K, r, lists=None, **mutation):
    """(normals (M, 3) float64 — ∞ rows where fewer than K neighbours —, neighbour lists, eigenvalues
    (M, 3) ascending — NaN on the ∞ rows —, covariances (M, 3, 3)).  lists: neighbour lists to use in
    place of neighbour_lists(P, K, r) (the CPU tests' mutations)."""
    if lists is None:
        lists = neighbour_lists(P, K, r, **mutation)
    _, C = moments(P, lists, K)
    M = len(lists)
    nrm, lam = np.full((M, 3), np.inf), np.full((M, 3), np.nan)
    ok = np.array([len(li) >= K for li in lists], bool)
    if ok.any():
        w, V = np.linalg.eigh(C[ok])
        n = V[:, :, 0]
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
        n = np.where(n[:, 2:3] < 0, -n, n)
        nrm[ok], lam[ok] = n, w
    return nrm, lists, lam, C


def rel_gap(lam):
    """(λ1 − λ0) / λ2 per row (0 where λ2 is 0; NaN rows stay NaN)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(lam[:, 2] > 0, (lam[:, 1] - lam[:, 0]) / lam[:, 2], 0.0 * lam[:, 2])


def residual(C, lam, n):
    """(‖C·n‖, its bound λ1 + λ2·(√3·2⁻²⁴ + 64·eps)) per row, for normals n of any origin."""
    Cn = np.einsum("mij,mj->mi", C, np.asarray(n, np.float64))
    l1, l2 = np.maximum(lam[:, 1], 0.0), np.maximum(lam[:, 2], 0.0)
    return np.linalg.norm(Cn, axis=1), l1 + l2 * (np.sqrt(3.0) * 2.0 ** -24 + 64 * DBL_EPS)
