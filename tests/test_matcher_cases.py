"""Premises of test_gpu_matcher_edges.py, on numpy and the CPU oracle alone: every scene of
matcher_cases.py reaches the edge it is named for, the oracle and the tree-less restatement
(matcher_np.py) agree on every case, every projection compares at least 95 % of its background rows, and
a matcher wrong in one of the named ways changes a named subject — its reject category (so idx), or y by
more than 100 × the 1e-5 m the GPU test allows.  The five-iteration frame is proved at the identity pose and,
for its features of coincident map points, at each of the oracle's iteration poses: their ties survive the
pose, and a wrong tie rule changes them at every iteration.  The list lengths and the small-frame threshold
that the scenes are sized against are read from the library's sources.

The oracle and the restatement give the same bits on every case, y included (both are fp64 in the
reference's order; measured: no difference on any row).  Where many map points coincide (copies-K20,
copies-K32: seventy copies of one point; hmax-0) the oracle's kd-tree is not independent evidence of the
order among the copies — they are equal in every coordinate, so any order among them gives the same list
distances — and the restatement alone names which copies are listed; the category and y do not depend on
it.
"""
import numpy as np
import pytest

import imls_np
import matcher_cases as mc
import matcher_np as mp

CATS = ("no_normal", "too_far", "invalid_normal", "normal_constraint", "mls_fail", "nan_inf_height")
ALL = mc.PATH_CASES + mc.OTHER_CASES
ALL_IDS = mc.PATH_IDS + mc.OTHER_IDS


def cat_name(c):
    return "valid" if c < 0 else CATS[c]


def scene_of(case):
    return case[1](*case[2])


def d2_of(scene, sub):
    G = mp.filtered(scene.tgt)
    return imls_np.exact_d2(sub.q, G[:, :3].astype(np.float64))


# ---- every named equality and count ----------------------------------------------------------------------------------
def check_facts(s, pose=None, every_pose=False):
    """The named facts of the scene's subjects, from the restatement at `pose` (None: identity) and the exact
    distances of the transformed query.  every_pose: only the subjects whose facts hold at any pose."""
    rows = mc.restated(s, pose)[5]
    a = s.par
    r2 = a.r * a.r
    G = mp.filtered(s.tgt)
    seen = 0
    for sub in s.subjects:
        if every_pose and not sub.facts.get("every_pose"):
            continue
        seen += 1
        w, f = rows[sub.row], sub.facts
        d2 = imls_np.exact_d2(w.x.astype(np.float64), G[:, :3].astype(np.float64))
        if pose is None:
            assert np.array_equal(w.x.astype(np.float64), sub.q), sub.name       # the query is a float: x = q
        if sub.cat is not None:
            assert cat_name(w.cat) == sub.cat, (sub.name, cat_name(w.cat))
        if "kcut_d2" in f:
            assert w.kcut_d2 == f["kcut_d2"], (sub.name, w.kcut_d2)
        if "kcut_count" in f:
            assert w.kcut_count == f["kcut_count"] == int((d2 == w.kcut_d2).sum()), (sub.name, w.kcut_count)
        if "cut_in" in f:
            inside = int((d2[w.listed] == w.kcut_d2).sum())
            assert inside == f["cut_in"] and int((d2 < w.kcut_d2).sum()) == a.K - inside < a.K, sub.name
            tied = np.nonzero(d2 == w.kcut_d2)[0]
            assert f["kcut_count"] > inside                                          # the K-th and the (K + 1)-th tie
            assert set(w.listed[-inside:]) == set(np.sort(tied)[:inside]), sub.name    # … broken by index
        if "within_r" in f:
            assert w.within_r == f["within_r"] == int((d2 <= (a.picp_r ** 2 if a.matcher == "picp" else r2)).sum()), (sub.name, w.within_r)
        if "on_r" in f:
            assert int((d2 == r2).sum()) == f["on_r"], sub.name
        if "above_r" in f:
            assert int((d2 == mc.up(r2)).sum()) == f["above_r"], sub.name
        if "band" in f:
            assert int(((d2 > r2) & (d2 <= 1.05 * 1.05 * r2)).sum()) == f["band"] + f.get("above_r", 0), sub.name
        if "d1" in f:
            assert w.d1 == f["d1"], (sub.name, w.d1)
        if "nn1_ties" in f:
            tied = np.nonzero(d2 == w.d1)[0]
            assert len(tied) == f["nn1_ties"] and w.nn1 == tied.min(), sub.name
            G = mp.filtered(s.tgt)
            assert len(np.unique(G[tied, 3:], axis=0)) == len(tied), sub.name            # their normals differ
        if "skipped" in f:
            assert int((d2[w.listed] <= mc.EPS).sum()) == f["skipped"], sub.name
        if "on_eps" in f:
            assert int((d2 == mc.EPS).sum()) == f["on_eps"], sub.name
        if "acc" in f:
            assert bin(w.acc_mask).count("1") == f["acc"], (sub.name, bin(w.acc_mask))
        if "acc_mask" in f:
            assert w.acc_mask == f["acc_mask"], (sub.name, bin(w.acc_mask))
        if f.get("hmax0"):
            n_acc = bin(w.acc_mask).count("1")
            assert n_acc >= 3 and d2[w.listed[n_acc - 1]] == 0.0 and w.hmax == 0.0, sub.name
        if "hmax" in f:
            assert w.hmax == f["hmax"], (sub.name, w.hmax)
        if "proj_ties" in f:
            d = mp.filtered(s.tgt)[:, :3].astype(np.float64) - sub.q
            pr = np.sqrt(d[:, 1] ** 2 + d[:, 0] ** 2)                                # n_s = (0, 0, 1)
            pr[np.sqrt((d * d).sum(axis=1)) >= a.picp_r ** 2] = np.inf              # the reference's swapped gate
            assert int((pr == pr[w.nn1]).sum()) == f["proj_ties"] and pr[w.nn1] == pr.min() < a.picp_r_proj, sub.name
            assert w.nn1 == np.nonzero(pr == pr.min())[0].min(), sub.name
        if "keys" in f:
            near = np.sort(d2[d2 <= 0.07])
            keys = near.astype(np.float32)
            assert len(near) == mc.KEY_M == len(np.unique(near)), sub.name          # distinct in fp64
            assert a.K < mc.KEY_M and mc.KEY_M > max(mc.LONE_KL.values())
            if f["keys"] == "four":
                assert len(np.unique(keys)) <= 4, sub.name
            else:
                idm = np.uint32(31 if f["keys"] == "id5" else 63)
                bits = keys.view(np.uint32)
                assert len(np.unique(bits & ~idm)) == 1 and len(np.unique(bits & idm)) > 8, sub.name
                # the cut falls between two keys that differ in the id bits alone
                assert (bits[a.K - 1] & ~idm) == (bits[a.K] & ~idm), sub.name
    return seen


@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_named_facts(case):
    s = scene_of(case)
    assert check_facts(s) == len(s.subjects)


def test_named_facts_of_the_frame():
    """The frame's subjects reach their edges at the identity pose of iteration 0; the features of coincident
    map points keep theirs at every pose of the oracle's five iterations: more than one map point on the
    K-cut distance, the cut decided by index, three NN-1 candidates at one d² — while the lattice ties are
    gone from iteration 1 on (asserted: this is why the coincident features are there)."""
    s = mc.scene_frame()
    assert check_facts(s) == len(s.subjects)
    poses = mc.frame_poses(mc.oracle_frame(s))
    assert len(poses) == mc.FRAME_ITERS
    for it, T in enumerate(poses):
        assert check_facts(s, T, every_pose=True) == len(mc.COPY_TIES) + 2, it
        assert mc.compare(mc.restated(s, T), mc.oracle_project(s, T), ("frame", it), y_tol=0.0) == 0.0
        if it:
            assert np.abs(T - np.eye(4)).max() > 0.01                              # the queries have moved
            rows = mc.restated(s, T)[5]
            assert all(rows[sub.row].kcut_count == 1 for sub in s.subjects if sub.name.startswith(("cut-", "shell-")))
    for K in (mc.FRAME_K,):
        for (a, b) in mc.COPY_TIES[:2]:
            assert K - a + a + b < mc.LIST_KL[K]                                    # the tie ends inside the list
        a, b = mc.COPY_TIES[2]
        assert K + b == mc.LIST_KL[K] and 56 > mc.LONE_KL[K]


def test_shells_outgrow_every_list():
    for K in mc.SHELL_KS:
        s = mc.scene_shell(K)
        small, big = (s.subject(f"shell-{n}").facts["kcut_count"] for n in mc.SHELL_SIZES)
        assert 40 <= small <= 60 and small > mc.LIST_KL[K]
        assert 40 <= big <= 60 and big > mc.LONE_KL[K]
        assert s.deferred == 2
    for K in mc.COPY_KS:
        assert mc.COPIES > mc.LONE_KL[K]


def test_h_above_is_the_next_double():
    assert mc.scene_h().subject("h-above").facts["d1"] == np.nextafter(0.2 * 0.2, 1.0)


def test_list_tables_are_the_librarys():
    """matcher_cases.LIST_KL, LONE_KL and BIG_FRAME restate with_list_sizes, lone_kl (project_common.h) and
    kSmallRows (internal.h); 'larger than the list' and 'above kSmallRows' mean what they say only while
    they agree, so the sources are read here: a rung or a threshold that moves fails this test."""
    import pathlib
    import re
    csrc = pathlib.Path(__file__).resolve().parent.parent / "planetary-lidar-odometry_amd" / "csrc"
    common, internal = (csrc / "project_common.h").read_text(), (csrc / "internal.h").read_text()
    body = common[common.index("void with_list_sizes(int K, F&& f) {"):]
    body = body[:body.index("\n}\n")]
    b_kl = int(re.search(r"#define IMLS_B_KL (\d+)", common).group(1))
    rungs = re.findall(r"(?:if \(K <= (\d+)\) |else )f\(KSizes<(\w+), (\d+)>\{\}\);", body)
    assert len(rungs) == 4 == body.count("KSizes<")
    table = {int(kcap): (b_kl if kl == "IMLS_B_KL" else int(kl)) for _, kl, kcap in rungs}
    assert [int(k) for k, _, _ in rungs[:3]] == [8, 16, 20] and rungs[3][0] == ""
    assert table == mc.LIST_KL
    extra = int(re.search(r"#define IMLS_LONE_EXTRA (\d+)", common).group(1))
    max_kl = int(re.search(r"constexpr int kMaxKL = (\d+);", internal).group(1))
    assert "return KL + IMLS_LONE_EXTRA <= kMaxKL ? KL + IMLS_LONE_EXTRA : kMaxKL;" in common
    assert {k: min(kl + extra, max_kl) for k, kl in table.items()} == mc.LONE_KL
    assert int(re.search(r"constexpr int kSmallRows = (\d+);", internal).group(1)) == mc.BIG_FRAME
    assert "return use_qwave(kp, N) && N <= kSmallRows;" in common               # fused_stage


def test_far_scenes_are_float_exact():
    for s in (mc.scene_cut(20, True), mc.scene_radius_far()):
        assert np.abs(s.tgt[:, :3]).max() > 9e4
        for sub in s.subjects:
            assert np.array_equal(np.float32(sub.q).astype(np.float64), sub.q)
    near, far = mc.scene_cut(20), mc.scene_cut(20, True)
    for a, b in zip(near.subjects, far.subjects):
        assert a.facts == b.facts                                                  # the same shells, bit for bit


def test_small_maps():
    for M in mc.SMALL_MS:
        s = mc.scene_small(M)
        assert len(mp.filtered(s.tgt)) == M
    s = mc.scene_small(20, True)
    rej = mc.restated(s)[4]
    assert int(rej[mp.TOO_FAR]) == len(s.src) and int(rej.sum()) == len(s.src)


# ---- the oracle and the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_oracle_equals_restatement(case):
    s = scene_of(case)
    dy = mc.compare(mc.restated(s), mc.oracle_project(s), s.name, y_tol=0.0)
    assert dy == 0.0


def test_oracle_equals_restatement_big_source():
    s = mc.with_big_source(mc.scene_shell(20))
    assert len(s.src) > mc.BIG_FRAME
    assert mc.compare(mc.restated(s), mc.oracle_project(s), s.name, y_tol=0.0) == 0.0


def test_nan_height_is_a_reject():
    """Read from the oracle, not assumed: a bandwidth point at d² = 0 gives exp(−0/0/0) = NaN, the height is
    NaN and the row is counted in nan_inf_height."""
    for s, name in ((mc.scene_accepted(), "hmax-0"), (mc.scene_copies(20), "copies"), (mc.scene_copies(32), "copies")):
        sub = s.subject(name)
        o = mc.oracle_project(s)
        assert sub.row not in set(int(i) for i in o[3])
        assert mc.restated(s)[5][sub.row].cat == mp.NAN_INF
        without = mc.restated(s)[4].copy()
        assert np.array_equal(o[4], without) and int(o[4][mp.NAN_INF]) >= 1


# ---- coverage: a condition of every GPU projection ---------------------------------------------------------------
def coverage(s, result):
    return float(np.isin(s.carrier_rows, result[3]).mean())


@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_background_rows_are_compared(case):
    s = scene_of(case)
    if len(s.carrier_rows):
        assert coverage(s, mc.oracle_project(s)) >= mc.COVERAGE, s.name
    # every subject is valid or in the category its case names: nothing the case is about goes unseen
    rows = mc.restated(s)[5]
    for sub in s.subjects:
        assert sub.cat is None or cat_name(rows[sub.row].cat) == sub.cat


def test_background_rows_big_and_frame():
    for case in mc.PATH_CASES:
        s = mc.with_big_source(scene_of(case))
        assert coverage(s, mc.oracle_project(s)) >= mc.COVERAGE, s.name
    s = mc.scene_frame()
    want = mc.oracle_frame(s)
    assert want["iters"] == mc.FRAME_ITERS
    for T in mc.frame_poses(want):
        assert coverage(s, mc.oracle_project(s, T)) >= mc.COVERAGE


# ---- every wrong variant changes a named subject ----------------------------------------------------------------------
def changed(s, variant, kl=None, pose=None):
    """The subjects whose category changes, or whose y moves by more than mc.MOVES, under the variant."""
    ref = mc.restated(s, pose)[5]
    got = mp.project(s.src[[sub.row for sub in s.subjects]], s.tgt, pose, s.par, variant=variant, kl=kl)[5]
    out = []
    for sub, g in zip(s.subjects, got):
        w = ref[sub.row]
        if g.cat != w.cat or (w.cat < 0 and np.abs(g.y.astype(np.float64) - w.y).max() > mc.MOVES):
            out.append(sub.name)
    return out


WRONG = [
    ("r_lt", lambda: mc.scene_radius(0.5), ("under", "exact")),
    ("r_lt", lambda: mc.scene_radius(0.3), ("under", "exact")),
    ("r_lt", mc.scene_radius_far, ("under", "exact")),
    ("r_lt", mc.scene_h3r1, ("r-on",)),
    ("h_ge", mc.scene_h, ("h-on",)),
    ("self_ge", mc.scene_self, ("self",)),
    ("no_self_rule", mc.scene_self, ("self",)),
    ("ties_position", mc.scene_self, ("self",)),
    ("ties_highest", mc.scene_self, ("self",)),
    ("q3_last", mc.scene_accepted_gate, ("gate-middle",)),
    ("q3_last", mc.scene_accepted, ("acc-3", "nan-places")),
    ("nacc2", mc.scene_accepted, ("acc-2",)),
]


@pytest.mark.parametrize("variant,fn,names", WRONG, ids=[f"{v}-{i}" for i, (v, _, _) in enumerate(WRONG)])
def test_wrong_variant_is_seen(variant, fn, names):
    s = fn()
    got = changed(s, variant)
    assert set(names) <= set(got), (variant, s.name, got)


@pytest.mark.parametrize("variant", ["ties_position", "ties_highest", "cut_unstable"])
@pytest.mark.parametrize("K", mc.CUT_KS + ("far",))
def test_wrong_tie_rule_is_seen_at_the_cut(K, variant):
    s = mc.scene_cut(20, True) if K == "far" else mc.scene_cut(K)
    got = changed(s, variant)
    assert len(got) >= 2, (K, variant, got)


@pytest.mark.parametrize("variant", ["ties_position", "ties_highest", "cut_unstable"])
def test_wrong_tie_rule_is_seen_in_the_frame(variant):
    """At the identity pose the lattice subjects see a wrong tie rule; at every later pose of the oracle's
    iterations — where lists are reused, prefilled and seeded — the coincident features do: each of them
    changes under ties_position and ties_highest (among equal points both pick the highest index), and at
    least three of the five under an unstable order."""
    s = mc.scene_frame()
    poses = mc.frame_poses(mc.oracle_frame(s))
    assert len([n for n in changed(s, variant) if n.startswith(("cut-", "shell-"))]) >= 2
    copies = {sub.name for sub in s.subjects if sub.facts.get("every_pose")}
    assert len(copies) == 5
    for it, T in enumerate(poses):
        got = copies & set(changed(s, variant, pose=T))
        assert len(got) >= 3 if variant == "cut_unstable" else got == copies, (variant, it, got)


def test_uncertified_list_is_seen_in_the_frame():
    s = mc.scene_frame()
    for T in mc.frame_poses(mc.oracle_frame(s)):
        for kl in (mc.LIST_KL[mc.FRAME_K], mc.LONE_KL[mc.FRAME_K]):
            assert "copy-shell" in changed(s, "list_nocert", kl, pose=T), kl


@pytest.mark.parametrize("K", mc.SHELL_KS)
def test_uncertified_list_is_seen(K):
    """A list of KL entries taken for the answer although its bound ties with the cut: the shell's members
    in it are the first to arrive, not the lowest indices."""
    s = mc.scene_shell(K)
    for kl in (mc.LIST_KL[K], mc.LONE_KL[K]):
        got = changed(s, "list_nocert", kl)
        assert "shell-56" in got, (K, kl, got)
    assert "shell-42" in changed(s, "list_nocert", mc.LIST_KL[K])
    seen = [set(changed(s, variant)) for variant in ("ties_position", "ties_highest", "cut_unstable")]
    assert all(seen) and set.union(*seen) == {"shell-42", "shell-56"}, seen


def test_wrong_tie_rule_is_seen_by_plane_icp():
    s = mc.scene_picp()
    ref = mc.restated(s)[5][s.subject("picp-tie").row]
    # plane_ICP's NN-1 goes through _plane, which has no variants: every other tied candidate is tried here
    d2 = d2_of(s, s.subject("picp-tie"))
    tied = np.sort(np.nonzero(d2 == ref.d1)[0])
    G = mp.filtered(s.tgt)
    x = s.subject("picp-tie").q
    ys = []
    for j in tied:
        n, v = G[j, 3:].astype(np.float64), x - G[j, :3].astype(np.float64)
        ys.append(x - ((v[0] * n[0] + v[1] * n[1]) + v[2] * n[2]) * n)
    assert ref.nn1 == tied[0] and np.abs(ys[0].astype(np.float32) - ref.y).max() == 0.0
    assert all(np.abs(y - ys[0]).max() > mc.MOVES for y in ys[1:])
    s = mc.scene_picp_proj()
    sub = s.subject("proj-tie")
    ref = mc.restated(s)[5][sub.row]
    G = mp.filtered(s.tgt)
    d = G[:, :3].astype(np.float64) - sub.q
    pr = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)
    pr[np.sqrt((d * d).sum(axis=1)) >= s.par.picp_r ** 2] = np.inf
    ys = []
    for j in np.nonzero(pr == pr.min())[0]:
        n, v = G[j, 3:].astype(np.float64), sub.q - G[j, :3].astype(np.float64)
        ys.append(sub.q - ((v[0] * n[0] + v[1] * n[1]) + v[2] * n[2]) * n)
    assert all(np.abs(y - ys[0]).max() > mc.MOVES for y in ys[1:])
    assert np.abs(ys[0].astype(np.float32) - ref.y).max() == 0.0
