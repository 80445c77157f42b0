"""CPU: the premises of tests/producer_offdefault_cases.py, on the C++ oracle and numpy alone — every
case does what it is named for (the branch it takes, the loop trip it forces, the row it flips), and
the oracle's own result moves with the value, so a device that ignored it could not agree.  The GPU
comparison is tests/test_gpu_producer_offdefault.py."""
import numpy as np
import pytest

import oracle_ctypes as oc
import producer_offdefault_cases as pc
from planetary_lidar_odometry_amd import _abi, synth

NORMAL, MAJOR = _abi.IMLS_SAMPLE_NORMAL, _abi.IMLS_SAMPLE_MAJOR_AXIS
FPS, RANDOM = _abi.SAMPLE_FPS, _abi.SAMPLE_RANDOM


def front(name):
    raw, fp = pc.front_case(name)
    return (raw, fp) + tuple(oc.scan_front_end(raw, fp))


# ---- A: front end ------------------------------------------------------------------------------

@pytest.mark.parametrize("name,branch,switches", [("frac04", "<pi", False), ("rev16", ">3pi", True), ("no_switch", "none", False),
                                                  ("period:16:0.05", "none", True)])
def test_front_branch_and_switch(name, branch, switches):
    """endOri − startOri and the halfPassed switch recomputed in numpy from the oracle's survivors."""
    raw, fp, ox, oidx, ors = front(name)
    s, start, span, got = pc.front_state_np(raw, fp)
    assert got == branch, (span / np.pi, got)
    sw = pc.switch_index_np(raw, start, oidx.astype(np.int64)[np.argsort(oidx)])
    assert (sw is not None) == switches
    ring = np.repeat(np.arange(fp.n_scans), ors)
    rel = (ox[:, 3].astype(np.float64) - ring) / fp.scan_period
    if name == "rev16":       # span 1.2π after 905-908: the first 0.6 revolution runs 0 … 1, what follows folds back below 0
        assert rel.max() > 0.99 and rel.min() < -0.2
    else:
        assert rel.min() > -1e-3 and rel.max() < 1 + 1e-3
    if not switches:                                       # one branch of 1029-1045 only: relTime below (π + step) / span
        assert rel.max() < 0.5


def test_reference_end_points_are_correctly_rounded():
    """The floor "nearly every intensity bit-equal" of test_front_end_matches_oracle needs the device's
    startOri / endOri (correctly rounded atan2) to be the reference's (glibc atan2f): true of every cut
    in FRONT_CASES, not of the two *_ulp cuts, which are there for the tolerance alone."""
    for name in pc.FRONT_CASES:
        raw, fp = pc.front_case(name)
        if name in ("empty", "dense_nan_first"):
            continue
        assert all(pc.end_points_correctly_rounded(raw, fp)), name
    for name in pc.FRONT_ULP_CASES:
        assert not all(pc.end_points_correctly_rounded(*pc.front_case(name))), name
    raw, fp = pc.front_case("rev16_ulp")
    assert pc.front_state_np(raw, fp)[3] == ">3pi"


@pytest.mark.parametrize("ns", [16, 32, 64])
def test_scan_period_moves_the_intensity(ns):
    a, b = (front(f"period:{ns}:{sp}") for sp in pc.SCAN_PERIODS)
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    ring = np.repeat(np.arange(ns), a[4])
    ra, rb = ((x[2][:, 3].astype(np.float64) - ring) / sp for x, sp in zip((a, b), pc.SCAN_PERIODS))
    assert np.abs(ra - rb).max() < 1e-4 and rb.max() > 0.99            # relTime is the same, the scale is not
    # a device with scan_period fixed at 0.1 is off by up to |0.1 − period| ≫ the tolerance
    assert 0.05 * rb.max() > 1e3 * pc.front_tolerance(a[2][:, 3], 0.05).max()


@pytest.mark.parametrize("ns", [16, 64])
def test_ends_without_a_ring_still_define_the_orientations(ns):
    raw, fp, ox, oidx, ors = front(f"noring_ends:{ns}")
    assert 0 not in oidx and len(raw) - 1 not in oidx
    s, start, span, _ = pc.front_state_np(raw, fp)
    assert s[0] == 0 and s[-1] == len(raw) - 1                          # they pass both filters
    ix, iidx, irs = oc.scan_front_end(raw[1:-1], fp)                    # the same sweep without them
    assert np.array_equal(iidx + 1, oidx) and np.array_equal(irs, ors)
    assert np.abs(ix[:, 3] - ox[:, 3]).max() > 0.01                     # another startOri / endOri


def test_on_axis_points():
    axis = {(0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)}
    for ns, kept_rings in ((16, None), (64, None), (32, {(0.0, 0.0, 0.0): 0, (0.0, 0.0, 1.0): 26, (0.0, 0.0, -1.0): 0})):
        raw, fp, ox, oidx, ors = front(f"on_axis:{ns}")
        assert fp.minimum_range == 0
        on = np.nonzero((raw[:, 0] == 0) & (raw[:, 1] == 0))[0]
        assert len(on) == 6 and {tuple(map(float, r)) for r in raw[on]} == axis
        if kept_rings is None:                                          # NaN / ±90° have no ring at 16 and 64 lines
            assert not np.isin(on, oidx).any()
        else:                                                           # 32 lines: the NaN angle lands in ring 0
            ring = np.repeat(np.arange(ns), ors)
            for i in on:
                assert ring[np.nonzero(oidx == i)[0][0]] == kept_rings[tuple(map(float, raw[i]))]
    raw, fp, ox, oidx, ors = front("on_axis_first")
    assert oidx[0] == 0 and np.all(ox[0, :3] == 0) and np.isfinite(ox[:, 3]).all()


def test_empty_dense_and_small_sweeps():
    raw, fp, ox, oidx, ors = front("empty")
    assert len(ox) == 0 and np.linalg.norm(raw, axis=1).min() > fp.maximum_range
    raw, fp, ox, oidx, ors = front("dense_nan:32")
    nan_in = np.isnan(raw).any(axis=1).sum()
    assert fp.is_dense == 1 and nan_in > 0 and np.isnan(ox[:, 0]).sum() == nan_in
    assert np.isin(np.nonzero(np.isnan(raw).any(axis=1))[0], front("dense_nan:16")[3]).sum() == 0
    raw, fp, ox, oidx, ors = front("dense_nan_first")
    assert np.isnan(raw[0]).all() and len(ox) == len(raw) and np.isnan(ox[:, 3]).all()
    for n in pc.FRONT_SIZES:
        assert len(front(f"size:{n}")[2]) == n
    raw, fp, ox, oidx, ors = front("single")
    assert list(oidx) == [5] and ox[0, 3] == np.floor(ox[0, 3])         # relTime 0 of the only survivor


# ---- B: ring PCA -------------------------------------------------------------------------------

def test_windows_move_the_oracle():
    seen = set()
    for w, st in pc.WINDOWS:
        o = pc.pca_oracle(f"window:{w}:{st}")
        assert 9315 <= len(o["index"]) <= 9380 and 1868 <= o["pca_failure"] <= 1933
        seen.add((len(o["index"]), o["pca_failure"], o["plane_invalid"], int((o["flags"] & 2 > 0).sum())))
    assert len(seen) == len(pc.WINDOWS)
    for name in ("window:0:1", "window:3:7"):                           # 3 / 6 window points: λ3 is rounding noise
        o = pc.pca_oracle(name)
        assert o["plane_invalid"] == 0 and 4000 < (o["evals"][:, 2] < 0).sum() < 5500
    # `k += st` and `num` separately: (3, 2) against (3, 1) changes the rows' values, not only the counts
    a, b = pc.pca_oracle("window:3:2"), pc.pca_oracle("shipped")
    common, ia, ib = np.intersect1d(a["index"], b["index"], return_indices=True)
    assert len(common) > 9000 and np.mean(np.abs(a["evals"][ia, 0] - b["evals"][ib, 0]) > 1e-6) > 0.5


@pytest.mark.parametrize("w,st", [(4, 1), (3, 2), (6, 1), (8, 3)])
def test_index_mode_failures_from_the_line_ends(w, st):
    xyz, sizes, p = pc.pca_case(f"index_plane:{w}:{st}")
    assert p.neighbor_scan == 1
    want = pc.expected_index_failures(sizes, w, st)
    assert pc.pca_oracle(f"index_plane:{w}:{st}")["pca_failure"] == want
    assert (want > 0) == (w >= 6)
    # unequal lines: the neighbour windows clip where the lines are shorter
    assert pc.pca_oracle(f"index_unequal:{w}:{st}")["pca_failure"] > want


def test_index_mode_on_unequal_lines():
    assert pc.pca_oracle("index_unequal:3:1")["pca_failure"] > pc.pca_oracle("index_plane:3:1")["pca_failure"] == 0
    a, b = pc.pca_oracle("index_vlp"), pc.pca_oracle("shipped")      # "index" against "kdtree" on the sweep
    assert a["pca_failure"] < b["pca_failure"] and len(a["index"]) > len(b["index"])


def test_knn_thresholds():
    t = pc.knn_thresholds()
    d2 = pc.nn_sq_distances("vlp")[:, 3]
    assert abs(np.mean(d2 < t["q25"]) - 0.25) < 0.01 and abs(np.mean(d2 < t["q75"]) - 0.75) < 0.01
    fails = [pc.pca_oracle(f"knn:{k}")["pca_failure"] for k in ("q25", "exact", "q75")]
    assert fails[0] > fails[1] > fails[2] > pc.pca_oracle("shipped")["pca_failure"]
    at, above = pc.pca_oracle("knn:exact"), pc.pca_oracle("knn:above")
    assert at["pca_failure"] == above["pca_failure"] + 1                 # strict <: d² == threshold fails the row
    xyz, sizes, _ = pc.pca_case("knn:exact")
    i, j = t["row"]
    row = int(np.concatenate([[0], np.cumsum(sizes)])[i]) + 5 + j
    assert np.array_equal(np.setdiff1d(above["index"], at["index"]), [row])


def test_thresholds_move_the_oracle():
    base = pc.pca_oracle("shipped")
    sig = lambda o: (o["plane_invalid"], int((o["flags"] & _abi.IMLS_PCA_CANDIDATE > 0).sum()))
    for group in (["distance:0.0", "distance:0.005", "distance:inf"], ["valid_points:0.0", "valid_points:0.5", "valid_points:1.0"],
                  ["planarity:-1.0", "planarity:0.3", "planarity:1.0"]):
        sigs = [sig(pc.pca_oracle(n)) for n in group]
        assert len(set(sigs)) == len(group), sigs
    assert sig(pc.pca_oracle("distance:0.0"))[0] == len(base["index"])      # dist < 0 never holds
    assert sig(pc.pca_oracle("distance:inf"))[0] == 0
    assert sig(pc.pca_oracle("valid_points:1.01"))[0] == len(base["index"])  # more valid points than the window has
    assert sig(pc.pca_oracle("valid_points:0.0"))[0] == 0
    # planarity −1 and 0 keep the same candidates: every valid row's planarity is positive
    assert sig(pc.pca_oracle("planarity:-1.0")) == sig(pc.pca_oracle("planarity:0.0"))
    assert sig(pc.pca_oracle("planarity:1.0"))[1] == 0
    assert len(pc.pca_oracle("drop_invalid")["index"]) == 1064
    for n in (265, 266, 267):                                                # 255, 256, 257 visited centres: one block, two
        assert len(pc.pca_oracle(f"guarded:{n}")["index"]) == n - 10


@pytest.mark.parametrize("name", pc.PCA_CASES)
def test_flip_bands_are_thin(name):
    o = pc.pca_oracle(name)
    _, _, p = pc.pca_case(name)
    plane, cand = pc.pca_bands(o, p)
    assert plane.sum() <= 0.01 * max(len(plane), 100) and cand.sum() <= 0.01 * max(len(cand), 100), (plane.sum(), cand.sum())


# ---- C: samplers -------------------------------------------------------------------------------

@pytest.mark.parametrize("az,el", pc.MANY_BINS)
def test_many_bins_hold_a_job(az, el):
    """More than 256 bins are sampled down (a job each), and bins beyond index 256 are among them:
    k_sw_plan's and k_sw_boff's loops go round again."""
    xyz, nrm, cand, last, p = pc.bins_case(az, el, NORMAL, FPS)
    sz = np.bincount(pc.bin_ids(nrm[cand], az, el), minlength=az * el)
    over = np.nonzero(sz > p.max_points_per_bin)[0]
    assert len(over) > 256 and over.max() > 256 and (sz > 0).sum() > 2000
    s, _ = oc.sample_point_cloud(xyz, nrm, cand, last, p)
    assert len(s) == np.minimum(sz[sz >= p.min_points_per_bin], p.max_points_per_bin).sum()
    xyz, nrm, cand, last, p = pc.bins_case(az, el, MAJOR, FPS)
    _, w = oc.sample_point_cloud(xyz, nrm, cand, last, p)
    assert (w > 0).sum() > 256


def test_edge_normals_land_in_bin_of():
    names = []
    for name, nrm, (az, el) in pc.edge_normals():
        xyz, nn, cand, last = pc.edge_scene(nrm)
        _, w = oc.sample_point_cloud(xyz, nn, cand, last, pc.edge_params(az, el))
        assert list(np.nonzero(w > 0)[0]) == [pc.bin_ids(nn[:1], az, el)[0]], name
        names.append(name)
    assert len(names) == 9 + 3 * (4 + 6)
    # the cases are edges: −x with −0 falls one azimuth bin below −x, 2π clamps to the last bin
    b = {n: pc.bin_ids(v[None], *bins)[0] for n, v, bins in pc.edge_normals()}
    assert b["-x"] == 4 * 8 + 4 and b["-x,-0"] == 3 * 8 + 4 and b["az→2π"] == 7 * 8 + 4 and b["+z"] == 7 and b["-z"] == 0
    straddle = 0
    for el in (5, 7):       # nz = −cos(kπ/EL) and its two float neighbours: on the edge k, mostly on both sides of it
        for k in range(1, el):
            got = {v for n, v in b.items() if n.startswith(f"el {k}/{el} ")}
            assert got <= {k - 1, k}, (k, el, got)
            straddle += len(got) == 2
    assert straddle >= 8


@pytest.mark.parametrize("n", pc.FPS_SIZES)
def test_fps_first_index_slots(n):
    seeds = pc.fps_seeds(n)
    last = (n - 1) // pc.FPS_BLOCK
    assert set(seeds) == {"slot0"} | ({"last"} if last >= 1 else set()) | ({"middle"} if last >= 2 else set())
    for slot, seed in seeds.items():
        first = int(oc.rand_sequence(seed, 1)[0]) % n
        assert {"slot0": first < pc.FPS_BLOCK, "middle": pc.FPS_BLOCK <= first < last * pc.FPS_BLOCK,
                "last": first >= last * pc.FPS_BLOCK}[slot]
        xyz, nrm = pc.one_bin_cloud(n)
        for method in (NORMAL, MAJOR):
            s, w = oc.sample_point_cloud(xyz, nrm, np.arange(n), pc.fps_last(xyz), pc.fps_params(method, seed))
            assert len(s) == 64 and s[0] == first and len(set(s.tolist())) == 64
            assert method == NORMAL or w[0] == 1.0


@pytest.mark.parametrize("n", [513, 8193])
def test_fps_farthest_point_property(n):
    """Every next sample is the farthest from the ones before (test_normal_sampling_bins_and_fps' check)."""
    xyz, nrm = pc.one_bin_cloud(n)
    for seed in pc.fps_seeds(n).values():
        s, _ = oc.sample_point_cloud(xyz, nrm, np.arange(n), None, pc.fps_params(NORMAL, seed))
        pts, allp = xyz[s].astype(np.float64), xyz.astype(np.float64)
        for k in (1, 10, 50):
            dmin = np.min(np.linalg.norm(allp[:, None] - pts[None, :k], axis=2), axis=1)
            assert np.isclose(np.linalg.norm(pts[k][None] - pts[:k], axis=1).min(), dmin.max())


def test_fps_ties():
    # copies: every distance is 0, the strict > scan takes the lowest index not yet taken
    xyz, nrm = pc.one_bin_cloud(600, "copies")
    p = pc.fps_params(NORMAL, 5)
    first = pc.fps_first_index(5, 600)
    s, _ = oc.sample_point_cloud(xyz, nrm, np.arange(600), None, p)
    assert first >= 63 and list(s) == [first] + list(range(63))
    # lattice: at most steps several points are equally far
    xyz, nrm = pc.one_bin_cloud(1200, "lattice")
    s, _ = oc.sample_point_cloud(xyz, nrm, np.arange(1200), None, p)
    pts, allp, tied = xyz[s].astype(np.float64), xyz.astype(np.float64), 0
    for k in range(1, 64):
        dmin = np.min(np.linalg.norm(allp[:, None] - pts[None, :k], axis=2), axis=1)
        far = np.nonzero(dmin == dmin.max())[0]
        assert s[k] == far.min()                           # the lowest index among the farthest
        tied += len(far) > 1
    assert tied > 30
    # duplicates: a duplicated point is taken through its lower index, its copy never
    xyz, nrm = pc.one_bin_cloud(9000, "duplicates")
    s, _ = oc.sample_point_cloud(xyz, nrm, np.arange(9000), None, pc.fps_params(NORMAL, 5, k=256))
    _, inv, cnt = np.unique(xyz, axis=0, return_inverse=True, return_counts=True)
    dup = cnt[inv.ravel()] > 1
    assert dup.sum() == 600 and dup[s[1:]].sum() >= 3
    for i in s[1:][dup[s[1:]]]:
        twin = np.nonzero((xyz == xyz[i]).all(axis=1))[0]
        assert i == twin.min() and twin.max() not in s


@pytest.mark.parametrize("r,r_proj", pc.BRUTE_RADII)
def test_major_axis_weights_by_brute_force(r, r_proj):
    xyz, nrm, cand, last, p = pc.radius_case(r, r_proj)
    _, w = oc.sample_point_cloud(xyz, nrm, cand, last, p)
    want = pc.major_weights_np(xyz, nrm, cand, last, p)
    assert np.array_equal(np.isnan(w), np.isnan(want))
    if (r, r_proj) in ((0.0, 1.5), (0.05, 1.5), (0.5, 0.05)):
        assert np.isnan(w).all() and len(w) == 64
    else:
        assert np.abs(w - want).max() <= 1e-5 * want.max() and (w > 0).sum() >= 4
        assert np.all(np.abs(w - want)[want > 0] <= 1e-5 * want[want > 0])


def test_radii_move_the_weights():
    ws = {}
    for r, r_proj in pc.RADII:
        _, w = oc.sample_point_cloud(*pc.radius_case(r, r_proj))
        ws[(r, r_proj)] = w
    live = [k for k, w in ws.items() if not np.isnan(w).any()]
    assert len(live) == 5
    for a in live:
        for b in live:
            if a < b and not {a, b} == {(5.0, 1.5), (float("inf"), 1.5)}:
                assert np.abs(ws[a] - ws[b]).max() > 1e-3, (a, b)
    # the box cull (r_proj · (1 + 1e-4)): a tenth narrower would lose neighbours the gate accepts — pairs
    # between 0.9 and 1.0 of r_proj² exist in numbers
    xyz, nrm, cand, last, p = pc.radius_case(0.5, 1.5)
    d2 = ((xyz[cand][:200, None, :].astype(np.float64) - last[None].astype(np.float64)) ** 2).sum(2)
    assert ((d2 > 0.9 * 2.25) & (d2 < 2.25)).sum() > 100


@pytest.mark.parametrize("shift", [False, True])
def test_strict_gate_scene(shift):
    xyz, nrm, cand, last, p = pc.gate_scene("at", shift)
    assert np.all(last[60:90, 2] - xyz[:30, 2] == np.float32(p.r_proj))       # exactly r_proj, exactly representable
    s, w = oc.sample_point_cloud(xyz, nrm, cand, last, p)
    floor_bin, wall_bin = pc.bin_ids(nrm[[0, 30]], 8, 8)
    assert w[floor_bin] == 0 and w[wall_bin] == 1                              # 2 neighbours: no weight
    xyz, nrm, cand, last, p = pc.gate_scene("below", shift)
    s, w = oc.sample_point_cloud(xyz, nrm, cand, last, p)
    assert abs(w[floor_bin] - 0.6) < 1e-5 and abs(w[wall_bin] - 0.4) < 1e-5   # 3 neighbours: (0.25 + 0.5 + 1.5) / 3 against 0.5


def test_previous_cloud_sizes_and_limits():
    for m in pc.PREV_SIZES:
        xyz, nrm, cand, last, p = pc.prev_size_case(m)
        assert len(last) == m and (m + 63) // 64 == (64 if m <= 4096 else 65)
        _, w = oc.sample_point_cloud(xyz, nrm, cand, last, p)
        assert (w > 0).sum() == 2
    sizes = {}
    for name in pc.LIMIT_CASES:
        for method in (NORMAL, MAJOR):
            s, _ = oc.sample_point_cloud(*pc.limit_case(name, method, FPS))
            sizes[(name, method)] = len(s)
    (x0, _, _), (x1, n1, c1) = pc.frames()
    shipped = len(oc.sample_point_cloud(x1, n1, c1, x0, pc.sample_params(MAJOR))[0])
    assert sizes[("max_total_100", MAJOR)] < shipped < sizes[("max_total_20000", MAJOR)] == len(c1)
    assert sizes[("bin_1_513", NORMAL)] > 800 and sizes[("bin_1_10000", NORMAL)] == len(c1)


# ---- D: the chain ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pc.CHAINS)
def test_chain_parameters_move_the_oracle_chain(name):
    """The first sweep through the oracle's front end and PCA under the chain's parameters: other rows
    and other candidates than the shipped chain's."""
    kw = pc.chain_kwargs(name)
    raw = pc.chain_raws()[0]
    ox, _, ors = oc.scan_front_end(raw, pc.front_params(16))
    o = oc.ring_pca(ox[:, :3], ors, kw["pca_params"])
    d = oc.ring_pca(ox[:, :3], ors, _abi.default_pca_params())
    assert len(o["index"]) > 5000 and not np.array_equal(o["evals"], d["evals"])
    cand = np.nonzero(o["flags"] & _abi.IMLS_PCA_CANDIDATE)[0]
    assert len(cand) > 500 and len(cand) != (d["flags"] & _abi.IMLS_PCA_CANDIDATE > 0).sum()
    sp = kw["normal_params"]
    assert (sp.azimuth_bins, sp.elevation_bins) in ((17, 16), (7, 5))
    s, _ = oc.sample_point_cloud(ox[:, :3][o["index"]], o["normal"], cand, None, sp)
    assert len(s) > 100
