"""CPU proofs for tv_cases.py: on the numpy restatement and the CPU oracle alone, every case reaches the
edge it is named for, every query's voted normal is visible (valid, or counted as no_normal), the
tolerance of the normal comparison holds between the two CPU references, and each wrong variant of the
restatement moves a named subject query by more than 100 × its tolerance or flips its found flag — which
is why test_gpu_tv_edges.py would fail on a kernel that is wrong in that way.  No GPU.

Tolerance of a normal's component: 2⁻²⁴ + B_q, B_q = 2·(Σ_voters 4ε‖S_j‖_F + 8ε‖A‖_F) / gap — the sum's
difference under an exp() off by an ulp or two, the 3×3 Jacobi's backward error, over the distance from
the picked eigenvalue to the nearest other one (doubled: sin θ ≤ ‖E‖ / (gap − ‖E‖), and |Δn| ≤ θ).

Figures of this file (the oracle's float32 n against the numpy restatement's double): largest
|Δn| / (2⁻²⁴ + B_q) 0.50 — the float rounding of the oracle's n — over the 2,307 valid rows of the 14
projection cases; B_q ≤ 1.1e-13 on every row; no carrier row fails the premises of the comparison."""
import numpy as np
import pytest

import imls_np
import oracle_ctypes as oc
import tv_cases as tc

ALL = list(range(len(tc.CASE_LIST)))


def case(i):
    fn, a, k = tc.CASE_LIST[i]
    return fn(*a), k


def angle(a, b):
    return np.arccos(np.clip(np.abs((a * b).sum(axis=-1)), 0.0, 1.0))


# ---- the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder,k", [(tc.scene_misc, tc.MISC_K), (tc.scene_threshold, 6), (tc.scene_self, tc.SELF_K)])
def test_vote_is_imls_np_tv_normals(builder, k):
    """vote() without a switch is oracle/imls_np.py::tv_normals (cKDTree candidates, its own loop)."""
    s = builder()
    p = dict(tensor_sigma=s.sigma, tensor_distance_threshold=s.thr, tensor_k=k)
    rows = [sub.row for sub in s.subjects] + list(s.carrier_rows[:20])
    nrm, found, acc = imls_np.tv_normals(tc.soa(s.tgt), tc.soa(s.ten), np.ascontiguousarray(s.src[rows, :3].T), p)
    v = tc.votes(s, k)
    for j, r in enumerate(rows):
        assert bool(found[j]) == v[r].found, (s.name, r)
        assert np.allclose(acc[j], v[r].acc, rtol=0, atol=1e-14 * max(1.0, np.abs(acc[j]).max())), (s.name, r)
        assert np.abs(nrm[j] - v[r].n).max() <= 1e-12, (s.name, r)


def test_cut_model_without_a_switch_is_the_knn_list():
    """cut_walk() with the tie rule and the slack gives the k best (d², index) whatever the arrival order."""
    s = tc.scene_ties()
    P, _ = s.filtered()
    for arr in arrival_orders(s, s.subject("cut-sphere")).values():
        for name in ("cut-point", "cut-centre", "cut-sphere", "cut-near"):
            x = s.src[s.subject(name).row, :3]
            for k in tc.TIE_KS:
                assert np.array_equal(tc.cut_walk(x, P, k, s.rho, arr), tc.knn_list(x, P, k)), (name, k)


# ---- every case: visibility, categories, the tolerance between the two CPU references ----------------------------
@pytest.mark.parametrize("i", ALL, ids=tc.CASE_IDS)
def test_case_premises(i):
    s, k = case(i)
    assert len(s.tgt) <= 4200 and len(s.src) <= 400
    v = tc.votes(s, k)
    x, y, n, idx, rej = tc.oracle_project(s, k)
    nrm, found, acc = tc.oracle_votes(s, k)
    # every query is valid or has no normal (the NaN-tensor variant: a normal that is not finite)
    want = {"no_normal": 0, "invalid_normal": 0}
    for sub in s.subjects:
        if sub.category != "valid":
            want[sub.category] += 1
            assert sub.row not in idx, sub.name
        else:
            assert sub.row in idx, sub.name
        assert v[sub.row].found == (sub.category != "no_normal"), sub.name
    assert [int(r) for r in rej] == [want["no_normal"], 0, want["invalid_normal"], 0, 0, 0], rej
    assert len(idx) + int(rej.sum()) == len(s.src)
    assert np.array_equal(x, s.src[idx, :3])                     # identity pose: x is the query
    # the named ball counts, restated (dist < thr, the self match left out)
    P, _ = s.filtered()
    for sub in s.subjects:
        if sub.count is not None:
            d2 = imls_np.exact_d2(s.src[sub.row, :3].astype(np.float64), P)
            assert int(((np.sqrt(d2) / s.sigma < s.thr) & (d2 > tc.EPS)).sum()) == sub.count, sub.name
    # oracle against the restatement: found flags, sums, and n within the tolerance; the premises of the
    # n comparison hold for every subject and (the condition) for ≥ 95 % of the valid rows
    for r in range(len(s.src)):
        assert bool(found[r]) == v[r].found, r
    worst, left = tc.compare_normals(n, [v[r] for r in idx], s.name)
    for sub in s.subjects:
        if sub.category == "valid":
            assert tc.comparable(v[sub.row]), (sub.name, v[sub.row].bound, v[sub.row].stable, v[sub.row].n)
    assert left <= 0.05 * len(idx), (left, len(idx))
    assert worst <= 1.0, worst
    # the carrier is curved and its tensors differ: queries adjacent in source order have other normals
    rows = [r for r in s.carrier_rows if v[r].found]
    adj = angle(np.array([v[r].n for r in rows[:-1]]), np.array([v[r].n for r in rows[1:]]))
    tol = max(tc.tol_of(v[r]) for r in rows if tc.comparable(v[r]))
    assert np.median(adj) >= 1000.0 * tol, (np.median(adj), tol)
    print(f"{s.name}/k{k}: M {len(s.tgt)} N {len(s.src)} valid {len(idx)} rej {[int(r) for r in rej]} "
          f"|Δn|/tol {worst:.3f} left out {left} median adjacent angle {np.median(adj):.3f}")


# ---- ties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("name", ["tie-point", "tie-centre", "cut-point", "cut-centre", "cut-sphere"])
@pytest.mark.parametrize("k", tc.TIE_KS)
def test_ties_straddle_k(name, k, nan):
    """The k-th and (k+1)-th candidates have equal d² bits and different indices (the oracle's own kNN
    list says so too); the cut subjects hold more than 256 ball members; breaking the tie by position or
    in reverse index order moves the normal by more than 100 × tolerance."""
    s = tc.scene_ties(nan)
    P, T = s.filtered()
    sub = s.subject(name)
    x = s.src[sub.row, :3]
    d2 = imls_np.exact_d2(x.astype(np.float64), P)
    lst = tc.knn_list(x, P, k + 1)
    assert d2[lst[k - 1]].tobytes() == d2[lst[k]].tobytes() and lst[k - 1] < lst[k]
    od2, oidx = oc.knn(tc.soa(s.tgt), np.ascontiguousarray(x.reshape(3, 1)), k + 1, np.inf, False)
    assert np.array_equal(oidx[0], lst) and od2[0, k - 1] == od2[0, k]
    ball = int(((np.sqrt(d2) < s.rho) & (d2 > tc.EPS)).sum())
    assert (ball > tc.CAP) == name.startswith("cut"), ball
    base = tc.votes(s, k)[sub.row]
    for order in (tc.morton_rank(P), "reverse"):
        assert tc.moved(base, tc.vote(x, P, T, k, s.sigma, s.thr, order=order)), (name, k)


def test_nan_rows_renumber_the_ties():
    """The NaN variant: rows ahead of, inside and behind the lattices are filtered, so the filtered index
    (the tie order, and the tensor's row) is not the input index; the geometry and the normals are those of
    the plain variant."""
    a, b = tc.scene_ties(False), tc.scene_ties(True)
    bad = np.nonzero(~np.isfinite(b.tgt[:, :3]).all(axis=1))[0]
    assert list(bad) == [0, 900, len(b.tgt) - 1]
    Pa, Ta = a.filtered()
    Pb, Tb = b.filtered()
    assert np.array_equal(Pa, Pb) and np.array_equal(Ta, Tb)
    assert not np.array_equal(b.ten[: len(Tb)], Tb.astype(np.float32))     # reading tensors by filtered row is wrong


def arrival_orders(s, sub):
    """Two leaf orders for the cut model: leaves of 64 in Morton order, and the same leaves nearest first."""
    P, _ = s.filtered()
    mort = np.argsort(tc.morton_rank(P))
    d2 = imls_np.exact_d2(s.src[sub.row, :3].astype(np.float64), P)
    leaves = [mort[a:a + 64] for a in range(0, len(mort), 64)]
    return {"morton": mort, "nearest": np.concatenate(sorted(leaves, key=lambda l: d2[l].min()))}


# ---- the threshold, the self match ----------------------------------------------------------------------------
def test_threshold_edge():
    s = tc.scene_threshold()
    P, T = s.filtered()
    sub = s.subject("thr")
    x = s.src[sub.row, :3]
    assert not x.any()
    pts = {nm: int(np.nonzero((P == np.float32(p).astype(np.float64)).all(axis=1))[0][0])
           for nm, p in (("below", [0, tc.F32_BELOW, 0]), ("on", [0.25, 0, 0]), ("above", [0, 0, tc.F32_ABOVE]))}
    nr = np.sqrt(imls_np.exact_d2(np.zeros(3), P))
    assert nr[pts["on"]] / s.sigma == s.thr and nr[pts["below"]] / s.sigma < s.thr < nr[pts["above"]] / s.sigma
    assert tc.screen_d2(P[pts["above"]], x) <= tc.r2s_of(s.rho)          # inside the fp32 screen's slack
    v7 = tc.votes(s, 7)[sub.row]
    assert {pts["on"], pts["above"]} == set(v7.listed) - set(v7.voters)  # the slots that do not vote: exactly these
    assert pts["below"] in v7.voters and len(v7.voters) == tc.THR_NEAR + 1
    # k = nearer + 1: `on` holds the last slot and pushes nothing out; one slot fewer: it is cut itself
    v6, v5 = tc.votes(s, 6)[sub.row], tc.votes(s, 5)[sub.row]
    assert v6.listed[-1] == pts["on"] and pts["on"] not in v5.listed and np.array_equal(v5.voters, v6.voters)
    for k in tc.THR_KS:
        nrm, found, acc = tc.oracle_votes(s, k)
        assert np.allclose(acc[sub.row], tc.votes(s, k)[sub.row].acc, rtol=0, atol=1e-14)   # the oracle skips them too
    # sensitivity: `>` for `≥` votes the edge point
    for k in (6, 7):
        assert tc.moved(tc.votes(s, k)[sub.row], tc.vote(x, P, T, k, s.sigma, s.thr, ge=False)), k


def test_self_match():
    s = tc.scene_self()
    P, T = s.filtered()
    sub = s.subject("self")
    x = s.src[sub.row, :3]
    idx = [int(np.nonzero((P == np.float32(p).astype(np.float64)).all(axis=1))[0][0])
           for p in ([0, 0, 0], [1e-8, 0, 0], [0, 2e-8, 0])]
    d2 = imls_np.exact_d2(np.zeros(3), P)
    assert d2[idx[0]] == 0.0 and 0.0 < d2[idx[1]] <= tc.EPS < d2[idx[2]]
    od2, oidx = oc.knn(tc.soa(s.tgt), np.ascontiguousarray(x.reshape(3, 1)), tc.SELF_K, np.inf, False)
    assert idx[2] in oidx[0] and idx[0] not in oidx[0] and idx[1] not in oidx[0]
    base = tc.votes(s, tc.SELF_K)[sub.row]
    assert idx[2] in base.voters and len(base.voters) == tc.SELF_K
    # sensitivity: the self matches given slots push the two farthest voters out
    assert tc.moved(base, tc.vote(x, P, T, tc.SELF_K, s.sigma, s.thr, self_slot=True))


# ---- the zero test and the decomposition ------------------------------------------------------------------------
def test_zero_test_variants():
    s = tc.scene_misc()
    v = tc.votes(s, tc.MISC_K)
    nrm, found, acc = tc.oracle_votes(s, tc.MISC_K)
    big = {nm: float(np.abs(acc[s.subject(nm).row]).max()) for nm in ("zero-empty", "zero-tensors", "zero-below", "zero-above")}
    assert big["zero-empty"] == 0.0 and big["zero-tensors"] == 0.0 and len(v[s.subject("zero-tensors").row].voters) == 5
    assert 0.35e-12 <= big["zero-below"] <= 0.71e-12 and 1.4e-12 <= big["zero-above"] <= 2.84e-12
    assert big["zero-above"] == 4.0 * big["zero-below"]                     # a factor of two each side of 1e-12
    flags = {sub.name: bool(found[sub.row]) for sub in s.subjects}
    assert flags == {sub.name: sub.category != "no_normal" for sub in s.subjects}
    rej = tc.oracle_project(s, tc.MISC_K)[4]
    assert int(rej[tc.REJ_NO_NORMAL]) == int((found == 0).sum()) == 3
    # a NaN entry: the sum is NaN, the zero test fails, the normal is not finite and the query is rejected for it
    s = tc.scene_nan_tensor()
    nrm, found, acc = tc.oracle_votes(s, tc.MISC_K)
    row = s.subject("nan-tensor").row
    assert found[row] == 1 and np.isnan(acc[row]).any() and not np.isfinite(nrm[row]).all()
    assert int(tc.oracle_project(s, tc.MISC_K)[4][tc.REJ_INVALID]) == 1


def test_abs_smallest_lower_triangle_flip():
    s = tc.scene_misc()
    P, T = s.filtered()
    k = tc.MISC_K
    v = tc.votes(s, k)
    # argmin |λ| is not argmin λ, and the two eigenvectors are far apart
    sub = s.subject("abs-smallest")
    b = v[sub.row]
    assert b.pick != 0 and b.lam[0] < 0 and abs(b.lam[0]) > 2.0 * abs(b.lam[b.pick]) and len(b.voters) == 1
    assert tc.moved(b, tc.vote(s.src[sub.row, :3], P, T, k, s.sigma, s.thr, pick="min"))
    # the sum is visibly non-symmetric: the upper triangle gives another normal
    sub = s.subject("lower-triangle")
    b = v[sub.row]
    assert np.abs(b.acc - b.acc.T).max() > 1e-3 * np.abs(b.acc).max()
    assert tc.moved(b, tc.vote(s.src[sub.row, :3], P, T, k, s.sigma, s.thr, uplo="U"))
    # the overhang: the voted direction is the plates' (0.6, 0, −0.8), returned with n_z > 0
    b = v[s.subject("flip").row]
    assert b.n @ tc.OVERHANG < -0.9 and b.n[2] > 0.5
    n = tc.oracle_votes(s, k)[0][s.subject("flip").row]
    assert n[2] > 0.5 and np.abs(n - b.n).max() <= tc.tol_of(b)
    # duplicates: one equal-d² group larger than k
    sub = s.subject("duplicates")
    d2 = imls_np.exact_d2(s.src[sub.row, :3].astype(np.float64), P)
    b = v[sub.row]
    assert int((d2 == d2[b.listed[0]]).sum()) == 70 > k and np.all(d2[b.listed] == d2[b.listed[0]])
    assert np.array_equal(b.listed, np.nonzero(d2 == d2[b.listed[0]])[0][:k])   # the k lowest indices
    assert tc.moved(b, tc.vote(s.src[sub.row, :3], P, T, k, s.sigma, s.thr, order="reverse"))


# ---- the cut ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", tc.TIE_KS)
def test_cut_that_forgets_the_tie_rule_moves_the_sphere(k):
    """cut-sphere: 390 exactly tied members, so the first cut's bound (bk, bi) lies inside the shell and
    members arriving later must be admitted by index; a cut that compares d² alone refuses them all."""
    s = tc.scene_ties()
    P, T = s.filtered()
    sub = s.subject("cut-sphere")
    x = s.src[sub.row, :3]
    d2 = imls_np.exact_d2(x.astype(np.float64), P)
    assert int((d2 == d2[tc.knn_list(x, P, 1)[0]]).sum()) == len(tc.integer_sphere()) > tc.CAP
    base = tc.votes(s, k)[sub.row]
    for name, arr in arrival_orders(s, sub).items():
        wrong = tc.cut_walk(x, P, k, s.rho, arr, tie_rule=False)
        assert tc.moved(base, tc.vote(x, P, T, k, s.sigma, s.thr, listed=wrong)), (k, name)


def test_cut_bound_without_slack_moves_the_near_shell():
    """cut-near: 400 points at 0.25 m in float32 — distinct d² within 2e-7 of each other, where the fp32
    screen distance has four values; after a cut, float(bk) without slack refuses members that beat bk."""
    s = tc.scene_ties()
    P, T = s.filtered()
    sub = s.subject("cut-near")
    x = s.src[sub.row, :3]
    k = 50
    d2 = imls_np.exact_d2(x.astype(np.float64), P)
    ball = np.nonzero((np.sqrt(d2) < s.rho) & (d2 > tc.EPS))[0]
    assert len(ball) == tc.NEAR_M > tc.CAP and len(np.unique(d2[ball])) > 0.9 * tc.NEAR_M
    assert len(np.unique(tc.screen_d2(P[ball], x))) <= 8
    base = tc.votes(s, k)[sub.row]
    for name, arr in arrival_orders(s, sub).items():
        wrong = tc.cut_walk(x, P, k, s.rho, arr, slack=False)
        assert tc.moved(base, tc.vote(x, P, T, k, s.sigma, s.thr, listed=wrong)), name


# ---- frames: the skin lists ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame():
    s = tc.scene_frame()
    r = tc.oracle_frame(s)
    poses = tc.frame_poses(r)
    return s, r, poses, [tc.frame_queries(s, T) for T in poses]


def test_frame_runs_and_every_query_is_visible(frame):
    s, r, poses, xs = frame
    assert r["iters"] == tc.FRAME_ITERS >= 3 and len(s.tgt) <= 4200
    for it, T in enumerate(poses):
        x, y, n, idx, rej = tc.oracle_project(s, tc.FRAME_K, T, tc.FRAME_ITERS)
        assert [int(v) for v in rej[1:]] == [0] * 5 and len(idx) + int(rej[0]) == len(s.src)
        assert np.array_equal(x, xs[it][idx])
        assert list(r["trace"][it].reject) == [int(v) for v in rej] and r["trace"][it].n_valid == len(idx)
        votes = tc.bounds_at(s, tc.FRAME_K, x)
        worst, left = tc.compare_normals(n, votes, f"frame it {it}")
        assert worst <= 1.0 and left <= 0.05 * len(idx), (it, worst, left)
        for sub in s.subjects:
            assert sub.row in idx and tc.comparable(votes[list(idx).index(sub.row)]), (it, sub.name)


def test_frame_list_sizes(frame):
    """The skin ball of list-64 / list-65 at iteration 0 (the stored one) by the kernel's float32 expression:
    64 fits kTvList, 65 does not; no point lies between 0.8 and 1.2 of the skin radius.  The overflow
    subjects at skin 0.3: skin ball above 256 with the ball proper below (overflow-ball) and above."""
    s, r, poses, xs = frame
    P, _ = s.filtered()
    for skin in (0.01, 0.03):
        rs = float(tc.skin_radius(s.rho, skin)[0])
        for n in (64, 65):
            x = xs[0][s.subject(f"list-{n}").row]
            assert tc.skin_count(x, P, s.rho, skin) == n and (n <= tc.LIST) == (n == 64)
            d = np.sqrt(imls_np.exact_d2(x.astype(np.float64), P))
            assert not ((d > 0.8 * rs) & (d < 1.2 * rs)).any() and int((d <= 0.8 * rs).sum()) == n
    for name, proper in (("overflow-ball", False), ("overflow-cut", True)):
        x = xs[0][s.subject(name).row]
        d2 = imls_np.exact_d2(x.astype(np.float64), P)
        assert tc.skin_count(x, P, s.rho, 0.3) > tc.CAP
        assert (int((tc.screen_d2(P, x) <= tc.r2s_of(s.rho)).sum()) > tc.CAP) == proper
        assert (int(((np.sqrt(d2) < s.rho) & (d2 > tc.EPS)).sum()) > tc.CAP) == proper


def test_frame_rewalk_and_reuse(frame):
    """From the oracle's own poses: at skins 0.01 and 0.03 some query moves farther than the skin since its
    stored reference at some iteration (a walk) and less at a later one (a reuse); at 0.3 and 1.0 every
    iteration after the first reuses; at 0 every iteration walks."""
    s, r, poses, xs = frame
    for skin in (0.01, 0.03):
        w = tc.reuse_plan(xs, skin)
        assert any(w[a, q] and not w[b, q] for q in range(w.shape[1]) for a in range(1, len(w)) for b in range(a + 1, len(w)))
    for skin in (0.3, 1.0):
        assert not tc.reuse_plan(xs, skin)[1:].any()
    assert tc.reuse_plan(xs, 0.0).all()


def test_frame_self_then_voter(frame):
    """The source row `self` equals a target point at iteration 0 (no slot) and has moved off it at
    iteration 1 (a slot and a vote); it moved less than 0.03 m, so skin 0.03 reuses the list stored at
    iteration 0 — which must hold the self match: a stored set without it moves the normal."""
    s, r, poses, xs = frame
    P, T = s.filtered()
    sub = s.subject("self")
    c = int(np.nonzero((P == xs[0][sub.row].astype(np.float64)).all(axis=1))[0][0])
    lists = [oc.knn(tc.soa(s.tgt), np.ascontiguousarray(xs[it][sub.row].reshape(3, 1)), tc.FRAME_K, np.inf, False)[1][0]
             for it in (0, 1)]
    assert c not in lists[0] and c in lists[1]
    assert not tc.reuse_plan(xs, 0.03)[1, sub.row] and tc.skin_count(xs[0][sub.row], P, s.rho, 0.03) <= tc.LIST
    x1 = xs[1][sub.row]
    base = tc.vote(x1, P, T, tc.FRAME_K, s.sigma, s.thr)
    assert c in base.voters
    stored = tc.knn_list(x1, P, tc.FRAME_K)
    assert tc.moved(base, tc.vote(x1, P, T, tc.FRAME_K, s.sigma, s.thr, listed=stored[stored != c]))


# ---- the other shapes ---------------------------------------------------------------------------------------------
def test_big_small_and_batch_scenes():
    big = tc.scene_big()
    assert len(big.src) > 4096 and len(big.src) <= 4300
    x, y, n, idx, rej = tc.oracle_project(big, tc.FRAME_K)
    assert not rej.any() and len(idx) == len(big.src)
    v = tc.bounds_at(big, tc.FRAME_K, x[::10])                       # every tenth row on the CPU
    worst, left = tc.compare_normals(n[::10], v, "big")
    assert worst <= 1.0 and left <= 0.05 * len(v)
    for n_ in tc.SMALL_N:
        assert len(tc.scene_small(n_).src) == n_
    sizes = [len(b.src) for b in tc.batch_scenes()]
    assert sizes == [3, 257, 601]
    tg = [b.tgt.tobytes() for b in tc.batch_scenes()]
    assert len(set(tg)) == 3
