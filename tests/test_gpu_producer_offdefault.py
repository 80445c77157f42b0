"""GPU: the producer AWAY from the shipped config.json — the cases of tests/producer_offdefault_cases.py
(their premises: tests/test_producer_offdefault_cases.py) on the device against the C++ oracle.

  A  imls_scan_front_end: indices, ring sizes and xyz exact, intensity within 2 ulp + 2e-8·(scan_period / 0.1)
     (test_front_end_matches_oracle's derivation: the azimuth's ulp through relTime scales with scan_period)
  B  imls_ring_normals_pca: test_gpu_scanreg_pca.py's assert_parity (row indices and pca_failure exact,
     |dot| > 1 − 1e-6, λ rtol 1e-5 / atol 1e-9, planarity atol 1e-5, NaN equal to NaN); a plane-check
     flip only where the oracle's margin < 1e-6, a candidate-bit flip only where the oracle's planarity
     is within 1e-6 of the threshold, and no more flips than rows in those bands
  C  imls_sample_point_cloud, imls_sample_point_cloud_device and the oracle all equal: indices exact,
     weights as bit patterns (test_gpu_sweep.py's check)
  D  imls_sweep_process against the host chain on a second context byte for byte, and against the
     oracle chain

Figures measured on the MI355X (largest |device − oracle| beside the tolerance) are printed by the
tests (pytest -s) on lines starting with MEASURED."""
import numpy as np
import pytest

import oracle_ctypes as oc
import producer_offdefault_cases as pc
from planetary_lidar_odometry_amd import _abi, imls_icp, producer
from test_gpu_scanreg_pca import assert_parity
from test_gpu_sweep import _check_transfers, check, dev_sample

pytestmark = pytest.mark.gpu
NORMAL, MAJOR = _abi.IMLS_SAMPLE_NORMAL, _abi.IMLS_SAMPLE_MAJOR_AXIS
FPS, RANDOM = _abi.SAMPLE_FPS, _abi.SAMPLE_RANDOM
PLANE, CAND = _abi.IMLS_PCA_PLANE_INVALID, _abi.IMLS_PCA_CANDIDATE


@pytest.fixture(scope="module")
def ctx():
    with imls_icp.ImlsContext(device=0) as c:
        yield c


@pytest.fixture(scope="module")
def ctx2():
    with imls_icp.ImlsContext(device=0) as c:
        yield c


# ---- A: front end ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pc.FRONT_CASES + pc.FRONT_ULP_CASES)
def test_front_end(ctx, name):
    """test_front_end_matches_oracle's assertions.  The *_ulp cuts (the reference's atan2f of an end
    point is an ulp off the correctly rounded value: see producer_offdefault_cases.py) meet the same
    tolerance; their floor of bit-equal rows is asked of rings ≥ 1, where an ulp of startOri moves
    scan_period·relTime by ~3e-9 against an intensity ulp of 1.2e-7 or more (under 3 % of the rows)."""
    raw, fp = pc.front_case(name)
    gx, gi, gidx, grs = ctx.scan_front_end(raw, fp)
    ox, oidx, ors = oc.scan_front_end(raw, fp)
    assert np.array_equal(grs, ors) and np.array_equal(gidx, oidx)
    assert np.array_equal(gx, ox[:, :3], equal_nan=True)
    fin = np.isfinite(ox[:, 3])
    assert np.array_equal(np.isfinite(gi), fin)
    if name in ("empty", "dense_nan_first"):
        assert not fin.any()
        return
    d = np.abs(gi[fin].astype(np.float64) - ox[fin, 3])
    tol = pc.front_tolerance(ox[fin, 3], fp.scan_period)
    print(f"\nMEASURED A {name}: n {fin.sum()} max |d| {d.max():.3e} max d/tol {np.max(d / tol):.3f} exact {np.mean(d == 0):.4f}")
    assert np.all(d <= tol), (d.max(), float(np.max(d / tol)))
    if name in pc.FRONT_ULP_CASES:
        upper = np.repeat(np.arange(fp.n_scans), ors)[fin] >= 1
        assert (d[upper] == 0).mean() > 0.95 and upper.sum() > 0.9 * len(d)
    else:
        assert (d == 0).mean() > 0.95


# ---- B: ring PCA -------------------------------------------------------------------------------

def _rows(d, k):
    return {key: (v[k] if isinstance(v, np.ndarray) else v) for key, v in d.items()}


def pca_parity(g, o, p):
    """assert_parity with the two kinds of flag flip told apart and NaN equal to NaN.  → (plane-check
    flips, candidate-bit flips, largest relative λ difference, largest planarity difference)."""
    assert np.array_equal(g["index"], o["index"]), "row indices"
    assert g["pca_failure"] == o["pca_failure"]
    diff = g["flags"] ^ o["flags"]
    plane_flip = (diff & PLANE) != 0
    cand_flip = ((diff & CAND) != 0) & ~plane_flip
    assert not (diff & ~np.uint8(PLANE | CAND)).any()
    plane_band, cand_band = pc.pca_bands(o, p)
    assert np.all(plane_band[plane_flip]), "plane-check flips away from the distance threshold"
    assert np.all(cand_band[cand_flip]), "candidate flips away from the planarity threshold"
    assert plane_flip.sum() <= plane_band.sum() and cand_flip.sum() <= cand_band.sum()
    assert abs(g["plane_invalid"] - o["plane_invalid"]) <= int(plane_flip.sum())
    same = np.nonzero(~(plane_flip | cand_flip))[0]
    gg, oo = _rows(g, same), _rows(o, same)
    gg["plane_invalid"] = oo["plane_invalid"]
    for key in ("evals", "features"):                      # NaN equal to NaN, then assert_parity on the rest
        ng, no = np.isnan(gg[key]), np.isnan(oo[key])
        cols = slice(None) if key == "evals" else 5
        assert np.array_equal(ng[:, cols], no[:, cols]), f"NaN positions of {key}"
        gg[key], oo[key] = np.where(ng | no, 0, gg[key]), np.where(ng | no, 0, oo[key])
    assert assert_parity(gg, oo) == 0
    ok = (oo["flags"] & PLANE) == 0
    lam = np.abs(gg["evals"][ok] - oo["evals"][ok]) / np.maximum(np.abs(oo["evals"][ok]), 1e-4)
    pl = np.abs(gg["features"][ok, 5] - oo["features"][ok, 5])
    return int(plane_flip.sum()), int(cand_flip.sum()), float(lam.max()) if lam.size else 0.0, float(pl.max()) if pl.size else 0.0


@pytest.mark.parametrize("name", pc.PCA_CASES)
def test_ring_pca(ctx, name):
    xyz, sizes, p = pc.pca_case(name)
    o = pc.pca_oracle(name)
    g = ctx.ring_normals_pca(xyz, sizes, p)
    assert len(o["index"]) > 0
    if not p.use_all_points:
        # a plane-check flip drops or keeps a row: only rows inside the band may differ; the rest compares
        full = pc.pca_oracle_all_rows(name)
        in_band = full["index"][full["margin"] < pc.BAND]
        odd = np.setxor1d(g["index"], o["index"])
        assert np.isin(odd, in_band).all() and len(odd) <= len(in_band)
        assert g["pca_failure"] == o["pca_failure"]
        _, gi, oi = np.intersect1d(g["index"], o["index"], return_indices=True)
        g, o = _rows(g, gi), _rows(o, oi)
        g["plane_invalid"] = o["plane_invalid"]
    pf, cf, lam, pl = pca_parity(g, o, p)
    plane_band, cand_band = pc.pca_bands(o, p)
    print(f"\nMEASURED B {name}: rows {len(o['index'])} flips plane {pf} (band {plane_band.sum()}) candidate {cf} "
          f"(band {cand_band.sum()}) max rel λ {lam:.3e} (1e-5) max |planarity| {pl:.3e} (1e-5)")


@pytest.mark.parametrize("field,value", [("window_size", -1), ("iter_step", 0)])
def test_ring_pca_rejects_a_bad_window(ctx, field, value):
    xyz, sizes, p = pc.pca_case("index_plane:3:1")
    setattr(p, field, value)
    with pytest.raises(_abi.ImlsError) as e:
        ctx.ring_normals_pca(xyz, sizes, p)
    assert e.value.status == _abi.IMLS_ERR_ARG


# ---- C: samplers -------------------------------------------------------------------------------

@pytest.mark.parametrize("strategy", [FPS, RANDOM])
@pytest.mark.parametrize("method", [NORMAL, MAJOR])
@pytest.mark.parametrize("az,el", pc.BINS)
def test_sampler_bins(ctx, az, el, method, strategy):
    s = check(ctx, *pc.bins_case(az, el, method, strategy))
    assert len(s) > 0 and len(set(s.tolist())) == len(s)


@pytest.mark.parametrize("method,strategy", [(NORMAL, FPS), (MAJOR, RANDOM)])
def test_sampler_more_than_4096_bins(ctx, method, strategy):
    xyz, nrm, cand, last, p = pc.bins_case(65, 64, method, strategy)
    with pytest.raises(_abi.ImlsError) as e:
        dev_sample(ctx, xyz, nrm, cand, last, p)
    assert e.value.status == _abi.IMLS_ERR_UNSUPPORTED
    so, wo = oc.sample_point_cloud(xyz, nrm, cand, last, p)
    sh, wh = ctx.sample_point_cloud(xyz, nrm, cand, last, p)               # the host form has no such bound
    assert len(so) > 0 and np.array_equal(sh, so) and np.array_equal(wh.view(np.uint32), wo.view(np.uint32))


def test_sampler_bin_edges(ctx):
    for name, nrm, (az, el) in pc.edge_normals():
        xyz, nn, cand, last = pc.edge_scene(nrm)
        for method in (MAJOR, NORMAL):
            s = check(ctx, xyz, nn, cand, last, pc.edge_params(az, el, method))
            assert len(s) == 3, name
    # the normals of one histogram together, three points each, every bin sampled down to two
    for bins in sorted({e[2] for e in pc.edge_normals()}):
        sel = [e[1] for e in pc.edge_normals() if e[2] == bins]
        nn = np.repeat(np.array(sel, np.float32), 3, axis=0)
        xyz = np.random.default_rng(len(sel)).uniform(-5, 5, nn.shape).astype(np.float32)
        p = pc.edge_params(*bins, NORMAL)
        p.max_points_per_bin = 2
        assert len(check(ctx, xyz, nn, np.arange(len(nn), dtype=np.int32), None, p)) >= 4


@pytest.mark.parametrize("method", [NORMAL, MAJOR])
@pytest.mark.parametrize("n", pc.FPS_SIZES)
def test_fps_bin_sizes(ctx, n, method):
    """One bin of n points through k_fps: registers up to 8,192 points, HBM above; the first index in
    slot 0, a middle slot and the last, partial slot of the register layout."""
    xyz, nrm = pc.one_bin_cloud(n)
    last = pc.fps_last(xyz) if method == MAJOR else None
    for slot, seed in pc.fps_seeds(n).items():
        s = check(ctx, xyz, nrm, np.arange(n, dtype=np.int32), last, pc.fps_params(method, seed))
        assert len(s) == 64 and s[0] == pc.fps_first_index(seed, n), slot


@pytest.mark.parametrize("kind,n,k", [("lattice", 1200, 64), ("copies", 600, 64), ("duplicates", 9000, 256), ("copies", 9000, 64)])
def test_fps_ties(ctx, kind, n, k):
    xyz, nrm = pc.one_bin_cloud(n, kind)
    for seed in (5, 6):
        s = check(ctx, xyz, nrm, np.arange(n, dtype=np.int32), None, pc.fps_params(NORMAL, seed, k=k))
        assert len(s) == k
        if kind == "copies":                               # the first index, then 0, 1, 2, … skipping it
            first = pc.fps_first_index(seed, n)
            assert list(s) == [first] + [i for i in range(k) if i != first][: k - 1]


@pytest.mark.parametrize("strategy", [FPS, RANDOM])
@pytest.mark.parametrize("r,r_proj", pc.RADII)
def test_major_axis_radii(ctx, r, r_proj, strategy):
    xyz, nrm, cand, last, p = pc.radius_case(r, r_proj, strategy)
    s = check(ctx, xyz, nrm, cand, last, p)
    # all-NaN weights (nothing within the radii): FPS keeps its first index per bin, "random" takes none
    nan = (r, r_proj) in ((0.0, 1.5), (0.05, 1.5), (0.5, 0.05))
    assert (len(s) == 0) == (nan and strategy == RANDOM)


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("kind", ["at", "below"])
def test_major_axis_strict_gate(ctx, kind, shift):
    xyz, nrm, cand, last, p = pc.gate_scene(kind, shift)
    check(ctx, xyz, nrm, cand, last, p)
    sd, wd, _ = dev_sample(ctx, xyz, nrm, cand, last, p)
    floor_bin = pc.bin_ids(nrm[:1], 8, 8)[0]
    assert (wd[floor_bin] == 0) == (kind == "at")


@pytest.mark.parametrize("m", pc.PREV_SIZES)
def test_major_axis_previous_cloud_sizes(ctx, m):
    assert len(check(ctx, *pc.prev_size_case(m))) > 0


@pytest.mark.parametrize("strategy", [FPS, RANDOM])
@pytest.mark.parametrize("method", [NORMAL, MAJOR])
@pytest.mark.parametrize("name", sorted(pc.LIMIT_CASES))
def test_sampler_limits(ctx, name, method, strategy):
    assert len(check(ctx, *pc.limit_case(name, method, strategy))) > 0


# ---- D: the chain ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pc.CHAINS)
def test_chain_off_default(ctx, ctx2, name):
    kw = pc.chain_kwargs(name)
    ctx.sweep_reset()
    dev = producer.ScanRegistration(ctx=ctx, shuffle_seed=4, rand_seed=2, **kw)
    host = producer.ScanRegistration(ctx=ctx2, shuffle_seed=4, rand_seed=2, **kw)
    fp = pc.front_params(16)
    last = None
    for k, raw in enumerate(pc.chain_raws()):
        sp = host.sample_params()
        h = dev.process_raw_device(raw, fp)
        cloud, flat = h.download()
        hcloud, hflat = host.process_raw(raw, fp)
        assert len(cloud) > 1000 and len(flat) > 100
        assert cloud.tobytes() == hcloud.tobytes() and flat.tobytes() == hflat.tobytes()
        assert np.array_equal(h.sampled, host.last_sampled)
        i = h.info
        assert (i["sweep"], i["n_input"], i["n_filtered"], i["n_flat"]) == (k + 1, len(raw), len(hcloud), len(hflat))
        assert i["n_candidates"] == len(host.last_candidates) and i["nan_normals"] == 0 and i["nan_keys"] == 0
        assert (i["pca_failure"], i["plane_invalid"]) == (host.last_pca["pca_failure"], host.last_pca["plane_invalid"])
        _check_transfers(i, raw)
        if name == "index_major_axis":                      # and the oracle's chain directly
            ox, oidx, ors = oc.scan_front_end(raw, fp)
            assert i["n_front"] == len(ox)
            o = oc.ring_pca(ox[:, :3], ors, kw["pca_params"])
            fxyz = ox[:, :3][o["index"]]
            assert np.array_equal(cloud["x"], fxyz[:, 0]) and np.array_equal(cloud["normal_z"], o["normal"][:, 2])
            cand = np.nonzero(o["flags"] & CAND)[0]
            assert np.array_equal(cand, host.last_candidates)
            s, _ = oc.sample_point_cloud(fxyz, o["normal"], cand, last, sp)
            assert np.array_equal(s, h.sampled) and np.array_equal(fxyz[s][:, 1], flat["y"])
            last = fxyz
