"""GPU parity of the producer methods added behind the C ABI — imls_presample_curvature
(scan_registration.cpp:1071-1113, 1462-1473, 1481-1489), imls_sample_three_axis (492-533) and
imls_sample_random (566-582, 779-781) — against the numpy restatements of tests/producer_methods_np.py
and, for the shuffle, the C++ oracle.  EXACT everywhere: np.array_equal on indices, and on the
curvature as uint32 views (the device evaluates the same float operations in the same order).  The
end-to-end test runs the curvature → three_axis producer on raw sweeps and registers its clouds
with the shipped parameters against the oracle (pose within 1e-6, as tests/test_gpu_stream.py).
Parity unpinned vs the reference itself (PCL's zeroed curvature field is inferred; std::sort on NaN
is undefined there and defined here: see include/imls_gpu.h)."""
import numpy as np
import pytest

import oracle_ctypes as oc
import producer_methods_np as pm
from planetary_lidar_odometry_amd import _abi, config, imls_icp, producer, synth
from test_producer_methods import expected_random

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with imls_icp.ImlsContext(device=0) as c:
        yield c


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- curvature -------------------------------------------------------------------------------

def check_curvature(ctx, xyz, sizes, index, flags, w, thr):
    p = _abi.default_curvature_params()
    p.window_size, p.curvature_threshold = w, thr
    want = pm.curvature_np(xyz, sizes, w)
    want_c = pm.curvature_candidates_np(want, index, flags, thr)
    got, got_c = ctx.presample_curvature(xyz, sizes, index, flags, p)
    assert np.array_equal(u32(got), u32(want))
    assert np.array_equal(got_c, want_c)
    return want, want_c


@pytest.mark.parametrize("w", [5, 7])       # w = 7: the first ring's leading visited points have j < w
def test_curvature_vlp16_sweep(ctx, w):
    st = pm.sweep_stage("vlp16", 0)
    c, cand = check_curvature(ctx, st["xyz"], st["sizes"], st["index"], st["flags"], w, 0.02)
    assert (c > 0).sum() > 9000 and len(cand) > 2000
    if w == 5:
        assert len(cand) == 2978


def test_curvature_invalid_rows_are_erased(ctx):
    st = pm.sweep_stage("vlp16", 0)
    flags = st["flags"].copy()
    flags[::3] |= _abi.IMLS_PCA_PLANE_INVALID        # as under use_all_points
    _, cand = check_curvature(ctx, st["xyz"], st["sizes"], st["index"], flags, 5, 0.02)
    assert len(cand) > 0 and not np.any(cand % 3 == 0)


CURV_CASES = {
    "last_ring_ends_within_w_of_N": ([30, 30], 9),
    "ring_sizes_0_11_12_13_mixed": ([40, 0, 11, 12, 300, 13, 0, 257, 11], 5),
    "N_le_2w": ([14], 7),
    "N_lt_w": ([3, 2], 7),
    "window_straddles_rings": ([30, 45, 30, 600], 9),     # ring offsets 0, 30, 75, 105: w > 5 reaches across
    "two_blocks_of_256": ([255, 256, 257], 5),
    "w_zero": ([40, 40], 0),
}


@pytest.mark.parametrize("name", sorted(CURV_CASES))
def test_curvature_ring_layouts(ctx, name):
    sizes, w = CURV_CASES[name]
    xyz, sizes = pm.noisy_rings(sizes, seed=len(name))
    index, flags = pm.all_rows(xyz)
    c, _ = check_curvature(ctx, xyz, sizes, index, flags, w, 0.02)
    if name == "window_straddles_rings":
        assert c[35] > 0 and c[35 + 18] > 0          # ring 1's first visited points: windows start in ring 0
    if name in ("N_le_2w", "N_lt_w", "w_zero"):
        assert not c.any()


def test_curvature_threshold_is_strict(ctx):
    xyz, sizes = pm.noisy_rings([60, 60], seed=11)
    index, flags = pm.all_rows(xyz)
    c = pm.curvature_np(xyz, sizes, 5)
    j = int(np.argsort(c)[len(c) * 3 // 4])           # a point in the upper quarter
    assert c[j] > 0
    _, cand = check_curvature(ctx, xyz, sizes, index, flags, 5, float(c[j]))
    assert j not in cand and len(cand) > 0
    _, cand = check_curvature(ctx, xyz, sizes, index, flags, 5, float(np.nextafter(c[j], np.float32(0))))
    assert j in cand


def test_curvature_empty_and_bad_arguments(ctx):
    got, cand = ctx.presample_curvature(np.zeros((0, 3), np.float32), [0, 0], np.zeros(0, np.uint32), np.zeros(0, np.uint8))
    assert len(got) == 0 and len(cand) == 0
    xyz, sizes = pm.noisy_rings([20], seed=0)
    got, cand = ctx.presample_curvature(xyz, sizes, np.zeros(0, np.uint32), np.zeros(0, np.uint8))   # no rows
    assert np.array_equal(u32(got), u32(pm.curvature_np(xyz, sizes, 5))) and len(cand) == 0
    with pytest.raises(_abi.ImlsError) as e:
        ctx.presample_curvature(xyz, sizes, np.array([20], np.uint32), np.zeros(1, np.uint8))       # row index = N
    assert e.value.status == _abi.IMLS_ERR_ARG
    p = _abi.default_curvature_params()
    p.window_size = -1
    with pytest.raises(_abi.ImlsError):
        ctx.presample_curvature(xyz, sizes, *pm.all_rows(xyz), p)


# ---- three_axis ------------------------------------------------------------------------------

def check_three_axis(ctx, xyz, nrm, ev, cand, ppl, nan_expected=0):
    want, want_nan = pm.three_axis_np(xyz, nrm, ev, cand, ppl)
    got, got_nan = ctx.sample_three_axis(xyz, nrm, ev, cand, ppl)
    assert want_nan == nan_expected and got_nan == nan_expected
    assert len(got) == 9 * min(ppl, len(cand))
    assert np.array_equal(got, want)
    return got


@pytest.mark.parametrize("presample", ["geometric_features", "curvature"])
def test_three_axis_vlp16_sweep(ctx, presample):
    st = pm.sweep_stage("vlp16", 0)
    if presample == "curvature":
        cand = pm.curvature_candidates_np(pm.curvature_np(st["xyz"], st["sizes"], 5), st["index"], st["flags"], 0.02)
    else:
        cand = st["geo"]
    assert len(cand) > 200
    s = check_three_axis(ctx, st["fxyz"], st["normal"], st["evals"], cand, 200)
    assert len(s) == 1800 and set(s.tolist()) <= set(cand.tolist())


# Sizes on both sides of every tile the shipped kernels use: points_per_list 200; the 256-thread
# blocks of k_ta_keys; the 1024-thread select block; powers of two around the bitonic sort's padding;
# 4096 = the LDS survivor buffer (at most 4096 candidates are sorted directly, more are narrowed by
# the radix passes first).
@pytest.mark.parametrize("n_cand", [0, 1, 2, 199, 200, 201, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 4095, 4096, 4097])
def test_three_axis_candidate_counts(ctx, n_cand):
    xyz, nrm, ev = pm.synthetic_cloud(5000, seed=21)
    cand = np.random.default_rng(n_cand).permutation(5000)[:n_cand]     # distinct, unordered
    check_three_axis(ctx, xyz, nrm, ev, cand, 200)


@pytest.mark.parametrize("n,ppl", [(600, 200), (9000, 200), (9000, 4096)])
def test_three_axis_duplicated_points_and_zero_components(ctx, n, ppl):
    # pairs of identical points (equal keys in all nine lists → larger idx first) and normals with a
    # zero component of either sign (±0 keys in lists 6-8, equal under std::greater)
    xyz, nrm, ev = pm.synthetic_cloud(n, seed=22, zero_components=True, duplicates=True)
    check_three_axis(ctx, xyz, nrm, ev, np.arange(n), ppl)


def test_three_axis_all_values_equal(ctx):
    # 6000 copies of one point: every list is decided by idx alone, so the select has to narrow
    # through all 64 bits of the composite
    xyz, nrm, ev = (np.repeat(a[:1], 6000, 0) for a in pm.synthetic_cloud(1, seed=23))
    cand = np.random.default_rng(3).permutation(6000)
    s = check_three_axis(ctx, xyz, nrm, ev, cand, 200)
    assert list(s[:200]) == list(range(5999, 5799, -1))


@pytest.mark.parametrize("ppl", [1, 4096])
def test_three_axis_points_per_list_bounds(ctx, ppl):
    st = pm.sweep_stage("vlp16", 0)
    check_three_axis(ctx, st["fxyz"], st["normal"], st["evals"], st["geo"], ppl)    # 2908 candidates: 4096 takes all
    xyz, nrm, ev = pm.synthetic_cloud(9000, seed=24)
    check_three_axis(ctx, xyz, nrm, ev, np.arange(9000), ppl)


def test_three_axis_points_per_list_out_of_range(ctx):
    xyz, nrm, ev = pm.synthetic_cloud(10, seed=25)
    for ppl in (4097, 0):
        with pytest.raises(_abi.ImlsError) as e:
            ctx.sample_three_axis(xyz, nrm, ev, np.arange(10), ppl)
        assert e.value.status == _abi.IMLS_ERR_UNSUPPORTED
    with pytest.raises(_abi.ImlsError) as e:
        ctx.sample_three_axis(xyz, nrm, ev, np.array([10]), 200)        # candidate index = n
    assert e.value.status == _abi.IMLS_ERR_ARG


@pytest.mark.parametrize("n", [500, 6000])
def test_three_axis_nan_keys(ctx, n):
    # negative λ3 on three rows: all nine of their values are NaN; they rank after every other entry
    # of their list, by descending idx (the documented definition), and are counted
    xyz, nrm, ev = pm.synthetic_cloud(n, seed=26)
    rows = [7, n // 2, n - 3]
    ev[rows, 2] = -1e-3
    s = check_three_axis(ctx, xyz, nrm, ev, np.arange(n), 4096, nan_expected=27)
    k = min(4096, n)
    if k == n:
        for l in range(9):
            assert list(s[l * k + k - 3: l * k + k]) == sorted(rows, reverse=True)


# ---- random ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_cand,max_points", [(300, 100), (2908, 2000), (300, 2000), (300, 300), (300, 299), (1, 2000),
                                               (0, 2000), (5, 0)])
def test_random_matches_the_oracle_shuffle(ctx, n_cand, max_points):
    cand = (np.random.default_rng(n_cand).permutation(4000)[:n_cand]).astype(np.int32)
    for seed in (0, 12345):
        got = ctx.sample_random(cand, max_points, seed)
        assert np.array_equal(got, expected_random(cand, max_points, seed))
    if n_cand >= 300 and max_points > 0:
        assert not np.array_equal(ctx.sample_random(cand, max_points, 1), ctx.sample_random(cand, max_points, 2))


# ---- end to end ------------------------------------------------------------------------------

def test_curvature_three_axis_producer_end_to_end():
    sc, poses = synth.make_scene(3), synth.trajectory(6, 2003)
    fp = _abi.default_front_params(16)
    fp.minimum_range, fp.maximum_range = 0.5, 100.0
    frames = []
    with imls_icp.ImlsContext(device=0) as c:
        sr = producer.ScanRegistration(ctx=c, presample_method="curvature", sample_method="three_axis")
        for k in range(2):
            raw = synth.raw_sweep(sc, synth.vlp16(), poses[2 + k], 40 + k, start_deg=15.0 * k)
            filtered, flat = sr.process_raw(raw, fp)
            xyz, _, _, sizes = c.scan_front_end(raw, fp)          # the same stage outputs, for the restatements
            o = sr.last_pca
            curv = pm.curvature_np(xyz, sizes, 5)
            cand = pm.curvature_candidates_np(curv, o["index"], o["flags"], 0.02)
            fxyz = xyz[o["index"]]
            want, nan = pm.three_axis_np(fxyz, o["normal"], o["evals"], cand, 200)
            assert nan == 0 and len(cand) > 200
            assert np.array_equal(sr.last_candidates, cand) and np.array_equal(sr.last_sampled, want)
            assert np.array_equal(u32(filtered["curvature"]), u32(curv[o["index"]]))
            assert np.array_equal(filtered["x"], fxyz[:, 0]) and np.array_equal(filtered["normal_z"], o["normal"][:, 2])
            assert len(flat) == 1800 and flat.tobytes() == filtered[want].tobytes()
            frames.append((filtered, flat))
    p = config.params_from_config(config.load())                  # the shipped parameters (RANSAC → DRPM)
    tgt, src = frames[0][0], frames[1][1]
    with imls_icp.ImlsContext(p, device=0) as c:
        c.set_target(tgt)
        c.set_source(src)
        r = c.register_frame()
    want = oc.register_frame(synth.soa(src), synth.soa(tgt), p)
    print("status", r["status"], want["status"], "iters", r["iters"], want["iters"], "pose |Δ|",
          np.abs(r["pose"] - want["pose"]).max())
    assert r["status"] == want["status"] and r["iters"] == want["iters"]
    assert np.abs(r["pose"] - want["pose"]).max() < 1e-6
