"""CPU tests of the producer-method restatements (tests/producer_methods_np.py) the GPU parity tests
compare against — known answers worked out by hand — of the conditions those GPU tests rely on
(asserted on their inputs), and of config.producer_from_config (lazy: no GPU needed)."""
import copy

import numpy as np
import pytest

import oracle_ctypes as oc
import producer_methods_np as pm
from planetary_lidar_odometry_amd import _abi, config, producer


# ---- curvature -------------------------------------------------------------------------------

def test_straight_ring_has_zero_curvature():
    xyz, sizes = pm.line_rings([30, 30, 30])
    for w in (5, 3):
        assert np.array_equal(pm.curvature_np(xyz, sizes, w), np.zeros(90, np.float32))


def test_one_displaced_point():
    xyz, sizes = pm.line_rings([30])
    xyz[15, 2] = 0.25
    c = pm.curvature_np(xyz, sizes, 5)
    # j = 15: ten neighbours each 0.25 below → dz = −2.5, dx = dy = 0 → 6.25;
    # j within 5 of it: one neighbour 0.25 above → 0.0625; visited range is [5, 24)
    want = np.zeros(30, np.float32)
    want[10:21] = 0.0625
    want[15] = 6.25
    assert np.array_equal(c, want)
    # a threshold equal to a point's curvature excludes it (strict >)
    idx, fl = pm.all_rows(xyz)
    assert list(pm.curvature_candidates_np(c, idx, fl, 0.0625)) == [15]
    assert list(pm.curvature_candidates_np(c, idx, fl, 0.06)) == list(range(10, 21))
    fl = fl.copy()
    fl[15] = _abi.IMLS_PCA_PLANE_INVALID
    assert 15 not in pm.curvature_candidates_np(c, idx, fl, 0.06)


def test_visit_range_and_window_bounds():
    # rings under 12 points are never visited; 12 → one point; the first ring's leading points with j < w get 0
    xyz, sizes = pm.noisy_rings([0, 11, 12, 13, 40], seed=1)
    c = pm.curvature_np(xyz, sizes, 7)
    off = np.concatenate([[0], np.cumsum(sizes)])
    visited = np.zeros(len(xyz), bool)
    for i, s in enumerate(sizes):
        visited[off[i] + 5: max(off[i] + s - 6, off[i] + 5)] = True
    assert visited.sum() == 0 + 0 + 1 + 2 + 29
    assert np.all(c[~visited] == 0)
    assert np.all(c[visited & (np.arange(len(xyz)) >= 7) & (np.arange(len(xyz)) < len(xyz) - 7)] > 0)
    # N <= 2w: no point has a full window
    xyz, sizes = pm.noisy_rings([14], seed=2)
    assert np.all(pm.curvature_np(xyz, sizes, 7) == 0)
    # the last ring ends within w of N: j >= N − w gets 0 although visited
    xyz, sizes = pm.noisy_rings([30, 30], seed=3)
    c = pm.curvature_np(xyz, sizes, 9)
    assert np.all(c[51:54] == 0) and np.all(c[35:51] > 0)


def test_window_uses_global_indices():
    # w = 9 > 5: the windows of a ring's first and last visited points reach into the neighbouring ring
    xyz, sizes = pm.noisy_rings([30, 30, 30], seed=4)
    c = pm.curvature_np(xyz, sizes, 9)
    j = 35                                           # ring 1, local index 5: window [26, 44] starts in ring 0
    d = np.zeros(3, np.float32)
    for k in range(-9, 10):
        d += xyz[j + k] - xyz[j]
    assert c[j] == (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    ring = xyz[30:60]                                # a ring-local window would clamp or wrap: a different value
    dl = np.zeros(3, np.float32)
    for k in range(-5, 10):
        dl += ring[5 + k] - ring[5]
    assert c[j] != (dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]


# ---- three_axis ------------------------------------------------------------------------------

def test_equal_keys_put_the_larger_index_first():
    xyz = np.array([[1, 2, 3], [1, 2, 3]], np.float32)
    nrm = np.array([[0, 0.6, 0.8], [0, 0.6, 0.8]], np.float32)
    ev = np.array([[0.5, 0.2, 0.01], [0.5, 0.2, 0.01]], np.float32)
    s, nan = pm.three_axis_np(xyz, nrm, ev, [0, 1], 200)
    assert nan == 0 and list(s) == [1, 0] * 9
    s, _ = pm.three_axis_np(xyz, nrm, ev, [0, 1], 1)
    assert list(s) == [1] * 9


def test_three_axis_known_values():
    # p = (1, 0, 0), n = (0, 0, 1): c = p × n = (0, −1, 0); λ = (1, 0.25, 0) → aD = 0.5, a2D = 0.25
    xyz = np.array([[1, 0, 0], [2, 0, 0]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, 1]], np.float32)
    ev = np.array([[1, 0.25, 0], [1, 0.25, 0]], np.float32)
    v = pm.three_axis_values_np(xyz, nrm, ev, [0, 1])
    assert np.array_equal(v[0], np.array([0, 0, -0.25, 0.25, 0, 0, 0, 0, 0.25], np.float32))
    assert np.array_equal(v[1], np.array([0, 0, -0.5, 0.5, 0, 0, 0, 0, 0.25], np.float32))
    s, nan = pm.three_axis_np(xyz, nrm, ev, [0, 1], 1)
    # lists 0, 1, 4-7: all values ±0 → larger idx; list 2: −0.25 > −0.5 → 0; list 3: 1; list 8: tie → 1
    assert nan == 0 and list(s) == [1, 1, 0, 1, 1, 1, 1, 1, 1]


def test_nan_keys_rank_last_by_descending_index():
    xyz, nrm, ev = pm.synthetic_cloud(10, seed=5)
    ev[[2, 7, 4], 2] = -1e-3                          # sqrt of a negative λ3 → NaN in all nine lists
    s, nan = pm.three_axis_np(xyz, nrm, ev, np.arange(10), 10)
    assert nan == 27
    for l in range(9):
        assert list(s[10 * l + 7: 10 * l + 10]) == [7, 4, 2]


# ---- the conditions the GPU tests rely on -----------------------------------------------------

def test_vlp16_sweep_counts_and_conditions():
    st = pm.sweep_stage("vlp16", 0)
    assert len(st["xyz"]) == 12954 and len(st["index"]) == 9373 and len(st["geo"]) == 2908
    curv = pm.curvature_np(st["xyz"], st["sizes"], 5)
    cc = pm.curvature_candidates_np(curv, st["index"], st["flags"], 0.02)
    assert len(cc) == 2978
    assert np.isfinite(st["normal"]).all()
    for cand in (st["geo"], cc):
        assert len(cand) > 200                       # n_cand > points_per_list where the test means it
        assert not np.isnan(pm.three_axis_values_np(st["fxyz"], st["normal"], st["evals"], cand)).any()
    # w = 7: the first ring's leading visited points have j < w
    assert st["sizes"][0] >= 12 and np.all(pm.curvature_np(st["xyz"], st["sizes"], 7)[5:7] == 0)


def test_hdl64_sweep_has_no_nan_key():
    st = pm.sweep_stage("hdl64", 0)
    assert len(st["xyz"]) == 126532 and len(st["geo"]) == 71347
    assert not np.isnan(pm.three_axis_values_np(st["fxyz"], st["normal"], st["evals"], st["geo"])).any()


def test_synthetic_three_axis_inputs():
    xyz, nrm, ev = pm.synthetic_cloud(600, seed=6, zero_components=True, duplicates=True)
    assert np.isfinite(nrm).all() and (ev > 0).all()
    v = pm.three_axis_values_np(xyz, nrm, ev, np.arange(600))
    assert not np.isnan(v).any()
    assert all((v[:, l] == 0).any() for l in (6, 7, 8))                         # zero keys in lists 6-8
    assert np.array_equal(v[:300], v[300:])                                     # duplicated points: equal keys


# ---- random ----------------------------------------------------------------------------------

def _oracle_random(cand, max_points, seed):
    """samplePointCloud "random" through the oracle: normalSampling on one bin, min_points 0, random
    strategy — one randomSampling call over all candidates with the seed's generator."""
    n = int(max(cand.max(), 0)) + 1 if len(cand) else 1
    xyz = np.zeros((n, 3), np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    p = _abi.default_sample_params(_abi.IMLS_SAMPLE_NORMAL)
    p.azimuth_bins = p.elevation_bins = 1
    p.min_points_per_bin, p.max_points_per_bin = 0, max_points
    p.sampling_strategy, p.shuffle_seed = _abi.SAMPLE_RANDOM, seed
    return oc.sample_point_cloud(xyz, nrm, cand, None, p)[0]


def expected_random(cand, max_points, seed):
    """What imls_sample_random must return, from the oracle alone: for n_cand > max_points the
    oracle call; else the call at max_points_per_bin = n_cand − 1 plus the one remaining candidate."""
    cand = np.asarray(cand, np.int32)
    if len(cand) == 0 or max_points == 0:
        return np.zeros(0, np.int32)
    if len(cand) > max_points:
        return _oracle_random(cand, max_points, seed)
    head = _oracle_random(cand, len(cand) - 1, seed) if len(cand) > 1 else np.zeros(0, np.int32)
    rest = np.setdiff1d(cand, head)
    assert len(head) == len(cand) - 1 and len(rest) == 1
    return np.concatenate([head, rest]).astype(np.int32)


def test_oracle_random_call_is_the_shuffle_prefix():
    cand = (np.arange(300) * 3 + 1).astype(np.int32)
    a = _oracle_random(cand, 100, 9)
    b = _oracle_random(cand, 299, 9)
    assert len(a) == 100 and len(b) == 299 and np.array_equal(b[:100], a)
    assert len(set(b.tolist())) == 299 and set(b.tolist()) <= set(cand.tolist())
    assert not np.array_equal(_oracle_random(cand, 100, 10), a)
    assert sorted(expected_random(cand, 2000, 9).tolist()) == cand.tolist()


# ---- producer_from_config ---------------------------------------------------------------------

def _cfg(**over):
    """The reference's scan_registration key paths with the shipped values, then overrides given as
    'a.b.c' = value."""
    cfg = copy.deepcopy(config.load())
    cfg["scan_registration"] = {
        "compute_normal_method": {"format": "pointcloud", "method": "pca",
                                  "pca": {"window_size": 3, "iter_step": 1, "knn_distance_threshold": 10,
                                          "neighbor_scan": "kdtree",
                                          "plane_constraint": {"distance_threshold": 0.02, "valid_points_threshold": 0.8}}},
        "presample_method": {"method": "geometric_features", "tensor_voting": {"k": 50, "sigma": 0.2},
                             "geometric_features": {"planarity_threshold": 0.05},
                             "curvature": {"curvature_threshold": 0.02, "window_size": 5}},
        "sample_method": {"method": "major_axis", "three_axis": {"points_per_list": 200}, "random": {"max_points": 2000},
                          "normal": {"azimuth_bins": 8, "elevation_bins": 8, "min_points_per_bin": 20,
                                     "max_points_per_bin": 100, "sampling_strategy": "random"},
                          "major_axis": {"r": 0.5, "r_proj": 1.5, "max_total_points": 2000, "azimuth_bins": 8,
                                         "elevation_bins": 8, "min_points_per_bin": 20, "max_points_per_bin": 200,
                                         "sampling_strategy": "FPS"}},
        "model": {"use_all_points": True}}
    for path, v in over.items():
        node = cfg["scan_registration"]
        keys = path.split(".")
        for k in keys[:-1]:
            node = node[k]
        node[keys[-1]] = v
    return cfg


def _fields(p):
    return {f: getattr(p, f) for f, _ in p._fields_}


def test_producer_from_config_shipped_file_and_values():
    for cfg in (config.load(), _cfg()):
        sr = config.producer_from_config(cfg)
        assert isinstance(sr, producer.ScanRegistration) and sr._ctx is None   # lazy: no context yet
        assert (sr.presample_method, sr.sample_method) == ("geometric_features", "major_axis")
        assert _fields(sr.pca_params) == _fields(_abi.default_pca_params())
        assert _fields(sr.curvature_params) == _fields(_abi.default_curvature_params())
        assert (sr.points_per_list, sr.max_points) == (200, 2000)
        for frame, m in ((1, _abi.IMLS_SAMPLE_NORMAL), (2, _abi.IMLS_SAMPLE_MAJOR_AXIS)):
            sr.frame = frame
            got, want = _fields(sr.sample_params()), _fields(_abi.default_sample_params(m))
            got.pop("shuffle_seed"), got.pop("rand_seed"), want.pop("shuffle_seed"), want.pop("rand_seed")
            assert got == want


@pytest.mark.parametrize("name", ["three_axis", "random", "normal", "major_axis"])
def test_producer_from_config_sample_methods(name):
    sr = config.producer_from_config(_cfg(**{"sample_method.method": name}))
    assert sr.sample_method == name


def test_producer_from_config_reads_every_block():
    sr = config.producer_from_config(_cfg(**{
        "presample_method.method": "curvature", "presample_method.curvature.curvature_threshold": 0.5,
        "presample_method.curvature.window_size": 7, "presample_method.geometric_features.planarity_threshold": 0.1,
        "sample_method.method": "three_axis", "sample_method.three_axis.points_per_list": 64,
        "sample_method.random.max_points": 500, "sample_method.normal.max_points_per_bin": 33,
        "sample_method.normal.sampling_strategy": "FPS", "sample_method.major_axis.r": 0.75,
        "compute_normal_method.pca.window_size": 4, "compute_normal_method.pca.neighbor_scan": "index",
        "compute_normal_method.pca.plane_constraint.valid_points_threshold": 0.5, "model.use_all_points": False}))
    assert (sr.presample_method, sr.sample_method, sr.points_per_list, sr.max_points) == ("curvature", "three_axis", 64, 500)
    assert sr.curvature_params.window_size == 7 and sr.curvature_params.curvature_threshold == 0.5
    p = sr.pca_params
    assert (p.window_size, p.neighbor_scan, p.use_all_points) == (4, 1, 0)
    assert p.valid_points_threshold == 0.5 and p.planarity_threshold == np.float32(0.1)
    assert sr.normal_params.max_points_per_bin == 33 and sr.normal_params.sampling_strategy == _abi.SAMPLE_FPS
    assert sr.major_axis_params.r == 0.75


@pytest.mark.parametrize("path,value", [
    ("compute_normal_method.method", "cross_product"), ("compute_normal_method.method", "FALS"),
    ("compute_normal_method.method", "SRI"), ("compute_normal_method.format", "range_image"),
    ("presample_method.method", "tensor_voting"), ("presample_method.method", "bogus_presample"),
    ("sample_method.method", "bogus_sample"), ("compute_normal_method.method", "bogus_normal"),
    ("sample_method.three_axis.points_per_list", 4097)])
def test_producer_from_config_rejects(path, value):
    with pytest.raises(config.ConfigError, match=str(value)):
        config.producer_from_config(_cfg(**{path: value}))


def test_scan_registration_constructor_keeps_its_defaults_and_validates():
    sr = producer.ScanRegistration()
    assert (sr.sample_method, sr.presample_method, sr.shuffle_seed, sr.rand_seed, sr.frame) == (
        "major_axis", "geometric_features", 0, 1, 1)
    with pytest.raises(ValueError):
        producer.ScanRegistration(sample_method="FALS")
    with pytest.raises(ValueError):
        producer.ScanRegistration(presample_method="tensor_voting")
