"""CPU proofs for map_normals_cases.py: on numpy and the CPU oracle alone, every case reaches the edge it
is named for, its census is complete, and the four mutations of csrc/normals.hip / api_map.hip that
test_gpu_map_normals.py must catch each change what one of its assertions compares.

Figures of this file (oracle against map_normals_np, float32 normals): 0 on every healthy case — the
oracle's Jacobi and LAPACK's eigh round to the same float on all 23,789 census rows of the 26 cases."""
import numpy as np
import pytest

import imls_np
import map_normals_cases as mc
import map_normals_np as mn

ALL = list(mc.CASES)


def case(name):
    c = mc.CASES[name]
    return c, mc.case_reference(c)


# ---- the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ties-K13", "radius-edge-K4", "size-M6", "islands"])
def test_neighbour_lists_equal_a_full_stable_sort(name):
    """The cut at the K-th distance before the lexsort loses nothing: the lists equal a full stable
    argsort by d² (stable: ascending index within equal d²) of the masked map."""
    c, ref = case(name)
    P64 = ref.P.astype(np.float64)
    for i in range(0, len(ref.P), 7):
        d2 = imls_np.exact_d2(ref.P[i], P64)
        ok = np.nonzero((d2 <= c.r * c.r) & (d2 > mn.DBL_EPS))[0]
        want = ok[np.argsort(d2[ok], kind="stable")][: c.K]
        assert np.array_equal(ref.lists[i], want), (name, i)
        assert i not in ref.lists[i]


def test_moments_are_the_plain_definition():
    """mean and covariance / K of the listed points (np.cov with bias), to fp64 rounding; K = 1: zero."""
    c, ref = case("rung-K9")
    mu, C = mn.moments(ref.P, ref.lists, c.K)
    for i in (0, 17, 1499):
        Q = ref.P[ref.lists[i]].astype(np.float64)
        assert np.allclose(mu[i], Q.mean(axis=0), rtol=0, atol=1e-15 * 8)
        assert np.allclose(C[i], np.cov(Q.T, bias=True), rtol=0, atol=1e-15)
    _, ref1 = case("rung-K1")
    assert not ref1.C.any() and not ref1.lam.any()


# ---- every case: the census is sound and complete ---------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_census_premises(name):
    """δ² > DBL_EPSILON survives the float rounding of every query (the self match is excluded, not the
    point), and the query's NN-1 is its own point (the lowest index among exact copies)."""
    c, ref = case(name)
    assert mc.DELTA ** 2 > mn.DBL_EPS and np.log2(mc.DELTA) == round(np.log2(mc.DELTA))
    d = ref.src[:, :3].astype(np.float64) - ref.P.astype(np.float64)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert (d2 > mn.DBL_EPS).all() and d2.max() <= (2 * mc.DELTA) ** 2
    assert np.array_equal(mc.nn1_of_queries(ref.P, ref.src), mc.first_copy(ref.P))


@pytest.mark.parametrize("name", ALL)
def test_case_reaches_its_edge_and_its_census_is_complete(name):
    """From the oracle alone: its census rows are the finite-normal points (≥ 95 %: the condition), its
    invalid-normal count is the restated ∞ count, its normals are the restated ones to one float32 ulp
    where the eigenvalue gap is healthy and within the residual bound elsewhere."""
    c, ref = case(name)
    if c.n_inf is not None:
        assert ref.n_inf == c.n_inf
    if c.healthy:
        assert ref.min_gap >= mn.GAP, ref.min_gap
    else:
        assert mn.rel_gap(ref.lam)[ref.finite].max() < mn.GAP      # no row of it has a direction to compare
    x, y, n, idx, rej = mc.oracle_census(ref.P, c.K, c.r, c.gate)
    assert np.array_equal(x, ref.src[idx, :3])                       # identity pose: x is the query
    err = mc.check_against_restatement(ref, n, idx, rej, c.healthy, name)
    print(f"{name}: M {len(ref.P)} finite {int(ref.finite.sum())} valid {len(idx)} rej {list(map(int, rej))} "
          f"min gap {ref.min_gap:.2e} oracle-restatement {err:.3e}")


def test_k3_needs_the_gate_off():
    """The reason rung-K3 runs without the angle gate: with it the census loses more than 5 %."""
    import oracle_ctypes as oc
    c, ref = case("rung-K3")
    x, y, n, idx, rej = oc.project(np.ascontiguousarray(ref.src.T), np.ascontiguousarray(mc.map_rows(ref.P).T), np.eye(4),
                                   mc.params(c.K, c.r, True))
    assert len(idx) < mc.COVERAGE * len(ref.P) and rej[mc.REJ_MLS_FAIL] > 0


# ---- rungs ---------------------------------------------------------------------------------------------------
def test_rungs_sit_on_both_sides_of_every_register_capacity():
    ks = sorted(c.K for c in mc.CASES.values() if c.name.startswith("rung-"))
    for kc in mc.KC_RUNGS:
        assert kc in ks                                             # K = KC: no sentinel slot
    for kc in mc.KC_RUNGS[:-1]:
        assert kc + 1 in ks                                         # the next rung's first K: KC' − K sentinels
    assert ks[0] == 1 and ks[-1] == mc.KC_RUNGS[-1]


@pytest.mark.parametrize("name", ["rung-K3", "rung-K9", "rung-K17", "ties-K6", "ties-K13", "duplicates-K12", "size-M6"])
def test_mutation_sentinel_off_by_one(name):
    """normals.hip `j < KC − K` written `j < KC − K − 1` (a capacity of K + 1): where K is inside a rung
    the census normals change on most points (assertion 2 of the GPU file fires), and every point with
    exactly K neighbours turns ∞ (assertion 3: size-M6, all of them)."""
    c, ref = case(name)
    nrm, _, _, _ = mn.map_normals(ref.P, c.K, c.r, lists=mc.sentinel_short_lists(ref))
    changed = (np.abs(nrm.astype(np.float32) - ref.nrm.astype(np.float32)) > mn.ULP1).any(axis=1) | (np.isfinite(nrm[:, 0]) != ref.finite)
    if name == "size-M6":
        assert not np.isfinite(nrm).any() and ref.finite.all()
    assert changed.sum() >= 0.5 * len(ref.P), changed.sum()


@pytest.mark.parametrize("name", ["rung-K8", "rung-K16", "rung-K32"])
def test_mutation_sentinel_is_invisible_on_a_rung(name):
    """… and why K = KC alone would not do: no slot is a sentinel there."""
    c, ref = case(name)
    assert all(np.array_equal(a, b) for a, b in zip(mc.sentinel_short_lists(ref), ref.lists))


# ---- ties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ties-K6", "ties-K13", "ties-shifted-K6", "ties-shifted-K13"])
def test_mutation_ties_by_the_highest_index(name):
    """Breaking equal d² by the highest index changes the normal of at least 50 lattice points."""
    c, ref = case(name)
    nrm, lists, _, _ = mn.map_normals(ref.P, c.K, c.r, highest_index_first=True)
    changed = (np.abs(nrm.astype(np.float32) - ref.nrm.astype(np.float32)) > mn.ULP1).any(axis=1)
    print(f"{name}: {int(changed.sum())} normals depend on the tie order")
    assert changed.sum() >= 50


@pytest.mark.parametrize("K", [6, 13])
def test_shifted_lattice_is_the_same_lattice(K):
    """(1e5, −1e5, 512) keeps every coordinate exact in float: the same lists, d² and normals."""
    _, a = case(f"ties-K{K}")
    _, b = case(f"ties-shifted-K{K}")
    assert np.array_equal(b.P.astype(np.float64) - a.P.astype(np.float64), np.broadcast_to([1e5, -1e5, 512.0], a.P.shape))
    assert all(np.array_equal(x, y) for x, y in zip(a.lists, b.lists))
    assert np.abs(a.nrm - b.nrm).max() <= 1e-9                      # fp64 moments about another mean
    na = mc.oracle_census(a.P, K, 1.0)[2]
    nb = mc.oracle_census(b.P, K, 1.0)[2]
    assert np.abs(na.astype(np.float64) - nb).max() <= mn.ULP1


# ---- radius ----------------------------------------------------------------------------------------------------
def test_radius_edge_is_exact():
    """Flat lattice, r = 0.25: the axis neighbours sit at d² = r² bit for bit; inside points have exactly
    four neighbours, so K = 4 is finite inside only, K = 5 nowhere, and the next double below 0.25 nowhere."""
    c, ref = case("radius-edge-K4")
    P64 = ref.P.astype(np.float64)
    counts = np.array([len(li) for li in ref.lists])
    inner = ((ref.P[:, :2] > 0) & (ref.P[:, :2] < 0.25 * 23)).all(axis=1)
    assert np.array_equal(counts == 4, inner) and np.array_equal(ref.finite, inner)
    for i in np.nonzero(inner)[0][::37]:
        assert (imls_np.exact_d2(ref.P[i], P64[ref.lists[i]]) == c.r * c.r).all()
    assert np.array_equal(ref.nrm[inner], np.broadcast_to([0.0, 0.0, 1.0], (inner.sum(), 3)))
    assert mc.R_BELOW < 0.25 and mc.R_BELOW * mc.R_BELOW < 0.0625
    for name in ("radius-edge-K5", "radius-below-K4"):
        assert not case(name)[1].finite.any()


def test_mutation_strict_radius():
    """`d² < r²` for `≤`: radius-edge-K4 loses every normal (assertion 3 fires: 576 ∞ for 92)."""
    c, ref = case("radius-edge-K4")
    nrm, _, _, _ = mn.map_normals(ref.P, c.K, c.r, strict_radius=True)
    assert not np.isfinite(nrm).any() and ref.finite.sum() == 22 * 22


def test_whole_map_inside_the_ball():
    """r = 1e3: no box and no point is ever outside the radius — the list's K-th distance alone prunes —
    and the lists are those of r = 1 (K = 13 reaches 0.56 m on the lattice)."""
    c, ref = case("radius-1e3-K13")
    _, near = case("ties-K13")
    assert np.linalg.norm(ref.P.max(axis=0) - ref.P.min(axis=0)) < c.r
    assert all(np.array_equal(a, b) for a, b in zip(ref.lists, near.lists))


def test_radius_decides_on_the_plane():
    c, ref = case("radius-plane-K10-r0.3")
    assert 0.25 * len(ref.P) < ref.n_inf < 0.75 * len(ref.P)
    wide = mn.neighbour_lists(ref.P, c.K, 1.0)
    assert sum(not np.array_equal(a, b) for a, b in zip(wide, ref.lists)) == ref.n_inf


# ---- duplicates --------------------------------------------------------------------------------------------------
def test_duplicates_share_one_normal():
    """Each point is stored three times: its copies are left out as self matches (d² = 0), a neighbour's
    three copies take consecutive list slots in index order, and the three copies get one normal."""
    c, ref = case("duplicates-K12")
    first = mc.first_copy(ref.P)
    assert (np.bincount(first, minlength=len(ref.P))[np.unique(first)] == 3).all()
    for i in range(0, len(ref.P), 41):
        li = ref.lists[i]
        assert (first[li] != first[i]).all()
        groups = first[li].reshape(4, 3)
        assert (groups == groups[:, :1]).all() and (np.diff(li.reshape(4, 3), axis=1) > 0).all()
    assert np.array_equal(ref.nrm, ref.nrm[first])
    assert len(ref.P) > mc.BIG_FRAME                                # the large-frame kernels project this census


# ---- sizes -------------------------------------------------------------------------------------------------------
def test_size_cases():
    K = mc.SIZES_K
    for M in (1, K, K + 1, 127, 128, 129):
        c, ref = case(f"size-M{M}")
        assert len(ref.P) == M and c.K == K
        d = ref.P[:, None, :].astype(np.float64) - ref.P[None, :, :]
        assert np.sqrt((d * d).sum(axis=2)).max() < c.r              # compact: every pair within r
        assert ref.finite.all() if M > K else not ref.finite.any()
    assert (mc.NRM_BLOCK - 1, mc.NRM_BLOCK, mc.NRM_BLOCK + 1) == (127, 128, 129)
    for leaf in mc.LEAVES:
        assert any(len(case(n)[1].P) % leaf for n in mc.LEAF_CASES)
        assert len(case("islands")[1].P) % leaf and 129 % leaf and 6 % leaf


def test_islands():
    """Fewer than K + 1 points farther than r from the rest: ∞ each, the large patch all finite."""
    c, ref = case("islands")
    far = ref.P[:, 0] > 5
    assert 0 < far.sum() < c.K + 1 and np.array_equal(ref.finite, ~far)
    d = ref.P[far][:, None, :].astype(np.float64) - ref.P[~far][None, :, :]
    assert np.sqrt((d * d).sum(axis=2)).min() > c.r


# ---- map kinds and batches -----------------------------------------------------------------------------------------
def test_consecutive_map_kinds_share_no_normal():
    """No float32 normal of one stage's map is a normal of the stage before it, and consecutive stages
    have as many normals to confuse (or fewer: the buffer is not regrown): normals left from the map
    before cannot pass for the map after.  This is what catches `rnr_valid` left set by any of the map
    calls (the mutation: not cleared in api_map.hip fifo_set_target — stages fifo, posed, rebased and
    cleared go through it): the census of the new map would read the old map's buffer."""
    maps = mc.kind_maps()
    assert [s for s, _ in maps] == ["host", "device", "fifo", "posed", "rebased", "voxel1", "voxel2", "cleared"]
    prev = None
    for stage, P in maps:
        ref = mc.reference(P, mc.KIND_K, mc.KIND_R)
        assert ref.finite.sum() >= 0.95 * len(P), stage
        rows = {r.tobytes() for r in ref.nrm[ref.finite].astype(np.float32)}
        if prev is not None:
            assert not (rows & prev), stage
        prev = rows
        x, y, n, idx, rej = mc.oracle_census(P, mc.KIND_K, mc.KIND_R)
        mc.check_against_restatement(ref, n, idx, rej, ref.min_gap >= mn.GAP, stage)
    assert len(maps[-1][1]) == len(maps[-2][1])                     # "a new map of the same size"
    g = mc.kind_inputs()
    assert np.isnan(g["host"]).any() and len(maps[0][1]) == len(g["host"]) - 2
    # the lattice's ties cross the FIFO's runs: some point's equal-distance neighbours lie in two runs
    lat = mc.reference(maps[2][1], mc.KIND_K, mc.KIND_R)
    run = np.searchsorted(np.cumsum([len(r) for r in g["runs"]]), np.arange(len(lat.P)), side="right")
    P64 = lat.P.astype(np.float64)
    crossing = 0
    for i, li in enumerate(lat.lists):
        d2 = imls_np.exact_d2(lat.P[i], P64[li])
        crossing += any(d2[a] == d2[a + 1] and run[li[a]] != run[li[a + 1]] for a in range(len(li) - 1))
    assert crossing >= 100, crossing
    # the second voxel update drops the whole first map
    assert len(maps[6][1]) == 600 and len(maps[5][1]) == 600


def test_batch_cases():
    maps = mc.batch_maps()
    sizes = [len(P) for P in maps]
    assert len(set(sizes)) == 3 and min(sizes) < mc.NRM_BLOCK < max(sizes)
    assert mc.BATCH_K not in mc.KC_RUNGS
    for P in maps + list(mc.failed_batch_maps()):
        ref = mc.reference(P, mc.BATCH_K, mc.BATCH_R)
        x, y, n, idx, rej = mc.oracle_census(P, mc.BATCH_K, mc.BATCH_R)
        mc.check_against_restatement(ref, n, idx, rej, ref.min_gap >= mn.GAP, len(P))
        assert ref.min_gap >= mn.GAP
    old, new, _ = mc.failed_batch_maps()
    a, b = mc.reference(old, mc.BATCH_K, mc.BATCH_R), mc.reference(new, mc.BATCH_K, mc.BATCH_R)
    assert len(old) == len(new)                                      # the normals' buffer is not regrown
    assert not ({r.tobytes() for r in a.nrm[a.finite].astype(np.float32)} & {r.tobytes() for r in b.nrm[b.finite].astype(np.float32)})
