"""Producer cases AWAY from the shipped config.json (shared by test_producer_offdefault_cases.py,
which proves on the oracle and numpy alone that each case does what it is named for, and
test_gpu_producer_offdefault.py, which runs them on the device).  No GPU imports: ImlsFrontParams is
filled by hand, as tests/deskew_cases.py does.

The rest of the suite runs the producer's kernels at one parameter set (window 3 / step 1, 8 × 8
bins, r 0.5 / r_proj 1.5, scan_period 0.1, full revolutions).  A parameter dropped or hard-coded on
its way to a kernel, a loop that never took a second trip, a tie that was never decided show only
away from it — and only if the oracle's own result moves with the value, which the premises assert.

  A  front end: scan_period, partial and over-long sweeps (both start_end branches, no halfPassed
     switch), ends without a ring, on-axis points, empty output, block-size edges
  B  ring PCA: (window_size, iter_step), both neighbour modes, every threshold, block-size edges
  C  samplers: bin counts past one block of k_sw_plan, bin edges, k_fps sizes / slots / ties,
     k_major_avg radii, strict gates, chunk counts
  D  the chain under two off-default imls_sweep_params
"""
import functools

import numpy as np

import oracle_ctypes as oc
import producer_methods_np as pm
from planetary_lidar_odometry_amd import _abi, synth
from test_sample_point_cloud import two_planes
from test_scanreg_pca import plane_rings

PI = np.pi


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- A: front end ------------------------------------------------------------------------------

def front_params(ns=16, lo=0.5, hi=100.0, period=0.1, dense=0):
    p = _abi.ImlsFrontParams()
    p.n_scans, p.minimum_range, p.maximum_range, p.scan_period, p.is_dense = ns, lo, hi, period, dense
    return p


def shipped_range(ns):
    """The ranges the existing front-end tests use: VLP-16 geometry for 16 / 32 lines, the launch file's for 64."""
    return (2.0, 150.0) if ns == 64 else (0.5, 100.0)


@functools.lru_cache(maxsize=None)
def _scene():
    return synth.make_scene(3), synth.trajectory(6, 2003)


@functools.lru_cache(maxsize=None)
def full_sweep(model="vlp16", k=0, start_deg=0.0, n_nan=0, n_close=0):
    sc, poses = _scene()
    m = synth.hdl64() if model == "hdl64" else synth.vlp16()
    raw = synth.raw_sweep(sc, m, poses[2 + k], 11 + k, start_deg=start_deg, n_nan=n_nan, n_close=n_close)
    return _ro(raw)[0]


def no_ring_point(ns, az_deg, r=10.0):
    """A point that passes both filters and gets no ring: vertical angle +20° at 16 lines ((20 + 15)/2
    + 0.5 → 18 > 15), +5° at 64 (above upperBound 2°)."""
    el = np.radians(20.0 if ns == 16 else 5.0)
    a = np.radians(az_deg)
    return np.array([r * np.cos(a), r * np.sin(a), r * np.tan(el)], np.float32)


# start_deg of the cut sweeps: the cut takes the named branch of 905-912 only if −atan2 of its first
# and last points do (0.4 revolution) or do not (1.6) straddle the ±π seam; the premises assert it
PARTIAL_START = {"frac04": 300.0, "rev16": 124.0, "rev16_ulp": 120.0, "no_switch": 30.0}
SIZE_OFFSET = {"size": 5064, "size_ulp": 5000}
SCAN_PERIODS = (0.05, 1.0)
FRONT_SIZES = (255, 256, 257)


@functools.lru_cache(maxsize=None)
def front_case(name):
    """(raw (n, 3) float32, ImlsFrontParams) of a section-A case."""
    kind, _, arg = name.partition(":")
    if kind == "period":                                   # period:<ns>:<scan_period>
        ns, period = arg.split(":")
        ns = int(ns)
        raw = full_sweep("hdl64" if ns == 64 else "vlp16", 0, 137.0, 7, 5)
        return raw, front_params(ns, *shipped_range(ns), period=float(period))
    if kind == "frac04":                                   # 0.4 revolution: endOri − startOri < π
        raw = full_sweep("vlp16", 0, PARTIAL_START[kind])
        return raw[: int(0.4 * len(raw))], front_params(16, period=0.05)
    if kind in ("rev16", "rev16_ulp"):                     # 1.6 revolutions: endOri − startOri > 3π
        a, b = full_sweep("vlp16", 0, PARTIAL_START[kind]), full_sweep("vlp16", 1, PARTIAL_START[kind])
        return _ro(np.concatenate([a, b])[: int(0.8 * (len(a) + len(b)))])[0], front_params(16, period=0.05)
    if kind == "no_switch":                                # 0.3 revolution: nothing passes startOri + π
        raw = full_sweep("vlp16", 0, PARTIAL_START[kind])
        return raw[: int(0.3 * len(raw))], front_params(16, period=1.0)
    if kind == "noring_ends":                              # noring_ends:<ns>
        ns = int(arg)
        raw = full_sweep("hdl64" if ns == 64 else "vlp16", 0, 200.0).copy()
        raw[0], raw[-1] = no_ring_point(ns, 100.0), no_ring_point(ns, 55.0)
        return _ro(raw)[0], front_params(ns, *shipped_range(ns))
    if kind == "on_axis":                                  # on_axis:<ns>, minimum_range 0
        ns = int(arg)
        raw = full_sweep("vlp16", 0, 80.0)[:6000]
        axis = np.array([[0, 0, 0], [0, 0, 1], [0, 0, -1]], np.float32)
        raw = np.concatenate([raw[:100], axis[:1], raw[100:3000], axis[1:], raw[3000:], axis[::-1]])
        return _ro(raw.astype(np.float32))[0], front_params(ns, 0.0, 150.0 if ns == 64 else 100.0)
    if kind == "on_axis_first":                            # the origin is the first survivor: startOri = −atan2(0, 0)
        raw = np.concatenate([np.zeros((1, 3), np.float32), full_sweep("vlp16", 0, 80.0)[:3000]])
        return _ro(raw)[0], front_params(32, 0.0, 100.0)
    if kind == "empty":                                    # maximum_range below every return
        return full_sweep("vlp16", 0, 0.0)[:5000], front_params(16, 0.0, 0.3)
    if kind == "dense_nan":                                # dense_nan:<ns>: is_dense with NaN points inside
        ns = int(arg)
        return full_sweep("vlp16", 0, 251.0, 7, 5)[:9000], front_params(ns, *shipped_range(16), dense=1)
    if kind == "dense_nan_first":                          # the first survivor is a NaN point: startOri is NaN
        raw = np.concatenate([np.full((1, 3), np.nan, np.float32), full_sweep("vlp16", 0, 251.0)[:3000]])
        return _ro(raw)[0], front_params(32, dense=1)
    if kind in ("size", "size_ulp"):                       # size:<n>
        off = SIZE_OFFSET[kind]
        return full_sweep("vlp16", 0, 45.0, 7, 5)[off: off + int(arg)], front_params(16, period=0.05)
    if kind == "single":                                   # one survivor among NaN and too-close points
        raw = np.full((9, 3), 0.01, np.float32)
        raw[2] = np.nan
        raw[5] = (3.0, -4.0, 0.3)
        return _ro(raw)[0], front_params(16, period=1.0)
    raise KeyError(name)


# The reference takes startOri / endOri from glibc's atan2f, the device from the correctly rounded
# value; they differ by an ulp on about one point in six.  Where they differ at the first or last
# survivor, every relTime moves by ~1e-8 — inside the tolerance, but above the float resolution of
# ring 0's intensities (< scan_period), so "nearly all rows bit-equal" cannot hold there.  The cases of
# FRONT_CASES are cut where the reference's two end points are correctly rounded (the premises assert
# it through libm); the two *_ulp cases are cuts where they are not.
FRONT_ULP_CASES = ["rev16_ulp", "size_ulp:256"]
FRONT_CASES = ([f"period:{ns}:{sp}" for ns in (16, 32, 64) for sp in SCAN_PERIODS]
               + ["frac04", "rev16", "no_switch", "noring_ends:16", "noring_ends:64", "on_axis:16", "on_axis:32",
                  "on_axis:64", "on_axis_first", "empty", "dense_nan:16", "dense_nan:32", "dense_nan_first"]
               + [f"size:{n}" for n in FRONT_SIZES] + ["single"])


def end_points_correctly_rounded(raw, fp):
    """Whether glibc's atan2f (the reference's std::atan2(float, float)) of the first and of the last
    survivor equals the correctly rounded value (atan2 in double, rounded once)."""
    import ctypes
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.atan2f.restype, libm.atan2f.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    s = front_state_np(raw, fp)[0]
    return [libm.atan2f(float(raw[i, 1]), float(raw[i, 0])) == float(np.float32(np.arctan2(np.float64(raw[i, 1]), np.float64(raw[i, 0]))))
            for i in (s[0], s[-1])]


def front_tolerance(ox_intensity, scan_period):
    """test_front_end_matches_oracle's bound: 2 ulp of the intensity plus the azimuth's ulp through
    relTime, 0.1·2·ulp / (endOri − startOri) < 2e-8 at scan_period 0.1, scaled with scan_period."""
    a = np.abs(ox_intensity).astype(np.float32)
    return 2 * np.spacing(a).astype(np.float64) + 2e-8 * (scan_period / 0.1)


def front_state_np(raw, fp):
    """numpy restatement of 899-912 and the halfPassed switch (1017-1032) on the points that survive
    the two filters: (endOri − startOri before 905-912, branch '>3pi' / '<pi' / 'none', input index of
    the switch point or None).  `ringed`: input indices the oracle kept (only they run 1017-1032)."""
    raw = np.asarray(raw, np.float32)
    ok = np.ones(len(raw), bool) if fp.is_dense else np.isfinite(raw).all(axis=1)
    r2 = (raw[:, 0] * raw[:, 0] + raw[:, 1] * raw[:, 1]) + raw[:, 2] * raw[:, 2]
    lo, hi = np.float32(fp.minimum_range), np.float32(fp.maximum_range)
    ok &= ~((r2 < lo * lo) | (r2 > hi * hi))
    s = np.nonzero(ok)[0]
    start = np.float32(-np.arctan2(raw[s[0], 1], raw[s[0], 0]))
    end = np.float32(np.float64(np.float32(-np.arctan2(raw[s[-1], 1], raw[s[-1], 0]))) + 2 * PI)
    span = np.float64(np.float32(end - start))
    branch = ">3pi" if span > 3 * PI else "<pi" if span < PI else "none"
    return s, start, span, branch


def switch_index_np(raw, start, ringed):
    """Input index of the first ring-valid point whose adjusted azimuth passes startOri + π, or None."""
    p = np.asarray(raw, np.float32)[ringed]
    ori = (-np.arctan2(p[:, 1], p[:, 0])).astype(np.float32).astype(np.float64)
    s = np.float64(start)
    ori = np.where(ori < s - PI / 2, ori + 2 * PI, np.where(ori > s + PI * 3 / 2, ori - 2 * PI, ori)).astype(np.float32)
    hit = np.nonzero((ori - np.float32(start)).astype(np.float64) > PI)[0]
    return int(ringed[hit[0]]) if len(hit) else None


# ---- B: ring PCA -------------------------------------------------------------------------------

WINDOWS = ((0, 1), (1, 1), (2, 1), (3, 2), (3, 4), (3, 7), (2, 3), (4, 1), (5, 1), (6, 1), (8, 3))
UNEQUAL_SIZES = (40, 25, 40, 60, 40)
BAND = 1e-6


def pca_params(**fields):
    p = _abi.default_pca_params()
    for k, v in fields.items():
        setattr(p, k, v)
    return p


@functools.lru_cache(maxsize=None)
def pca_input(name):
    """(xyz, ring sizes) of a section-B input."""
    if name == "vlp":
        st = pm.sweep_stage("vlp16", 0)
        return st["xyz"], st["sizes"]
    kind, _, arg = name.partition(":")
    if kind == "plane":                                    # plane:<per_ring>: 5 equal lines, 2 mm rough
        return _ro(*plane_rings(n_rings=5, per_ring=int(arg), jitter=0.002, seed=5))
    if kind == "unequal":                                  # the first sizes[i] points of line i of plane:60
        xyz, _ = plane_rings(n_rings=5, per_ring=60, jitter=0.002, seed=5)
        return _ro(np.concatenate([xyz[60 * i: 60 * i + s] for i, s in enumerate(UNEQUAL_SIZES)]),
                   np.array(UNEQUAL_SIZES, np.int32))
    if kind == "guarded":                                  # guarded:<size>: one visited line between two guard lines
        return _ro(*plane_rings(n_rings=3, per_ring=int(arg), dx=0.01, jitter=0.002, seed=int(arg)))
    raise KeyError(name)


def expected_index_failures(sizes, w, st):
    """pca_failure in "index" mode with EQUAL line sizes: the three windows clip alike, so a centre j
    fails (count < num) exactly when one of its own window points j + k, k = −w, −w + st, … ≤ w falls
    outside the line: j < w or j + k_max > size − 1 (for st = 1: j > size − 1 − w)."""
    sizes = np.asarray(sizes)
    assert np.all(sizes == sizes[0]) and sizes[0] >= 17
    size = int(sizes[0])
    k_max = -w + st * (2 * w // st)
    j = np.arange(5, size - 5)
    return int(((j < w) | (j + k_max > size - 1)).sum()) * (len(sizes) - 2)


@functools.lru_cache(maxsize=None)
def nn_sq_distances(name="vlp"):
    """The NN-1 squared distance of every visited centre to the previous and the next line, in the
    oracle's float arithmetic ((0 + d0²) + d1²) + d2² (flann::L2_Simple<float>): arrays
    (line i, centre j, side 0 / 1, d², nn index), visited lines only."""
    xyz, sizes = pca_input(name)
    off = np.concatenate([[0], np.cumsum(sizes)])
    rows = []
    for i in range(1, len(sizes) - 1):
        if sizes[i] == 0 or min(sizes[i - 1], sizes[i], sizes[i + 1]) - 11 < 6:
            continue
        c = xyz[off[i] + 5: off[i + 1] - 5]
        for side, a in enumerate((i - 1, i + 1)):
            q = xyz[off[a]: off[a + 1]]
            d = c[:, None, :] - q[None, :, :]
            d2 = (np.float32(0) + d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
            nn = np.argmin(d2, axis=1)
            rows.append(np.stack([np.full(len(c), i), np.arange(5, sizes[i] - 5), np.full(len(c), side),
                                  d2[np.arange(len(c)), nn].astype(np.float64), nn, np.full(len(c), sizes[a])], 1))
    return _ro(np.concatenate(rows))[0]


@functools.lru_cache(maxsize=None)
def knn_thresholds():
    """knn_distance_threshold cases on the VLP-16 stage: the 25 % and 75 % quantiles of the NN squared
    distances, and one row's own squared distance d² (strict <: the row fails) with nextafter(d²)
    (it passes).  The row: its d² is unique, its other side is nearer, and neither its own window
    nor the one around its neighbour is clipped at the shipped window 3 — so it alone changes."""
    t = nn_sq_distances("vlp")
    _, sizes = pca_input("vlp")
    d2 = np.sort(t[:, 3])
    q25, q75 = np.float32(d2[len(d2) // 4]), np.float32(d2[3 * len(d2) // 4])
    vals, counts = np.unique(t[:, 3], return_counts=True)
    unique = set(vals[counts == 1].tolist())
    key = {(int(r[0]), int(r[1]), int(r[2])): r for r in t}
    med = d2[len(d2) // 2]
    for r in t[np.argsort(np.abs(t[:, 3] - med))]:
        i, j, side, v, nn, sa = int(r[0]), int(r[1]), int(r[2]), r[3], int(r[4]), int(r[5])
        other = key[(i, j, 1 - side)]
        if (v in unique and other[3] < v and 3 <= nn <= sa - 4 and 3 <= int(other[4]) <= int(other[5]) - 4
                and 3 <= j <= sizes[i] - 4):
            return dict(q25=float(q25), q75=float(q75), exact=float(np.float32(v)),
                        above=float(np.nextafter(np.float32(v), np.float32(np.inf))), row=(i, j))
    raise AssertionError("no isolated row")


def _pca_table():
    t = {"shipped": ("vlp", {})}
    for w, st in WINDOWS:
        t[f"window:{w}:{st}"] = ("vlp", dict(window_size=w, iter_step=st))
    t["index_vlp"] = ("vlp", dict(neighbor_scan=1))
    for w, st in ((4, 1), (3, 2), (6, 1), (8, 3)):
        t[f"index_plane:{w}:{st}"] = ("plane:40", dict(neighbor_scan=1, window_size=w, iter_step=st))
        t[f"index_unequal:{w}:{st}"] = ("unequal", dict(neighbor_scan=1, window_size=w, iter_step=st))
    t["index_unequal:3:1"] = ("unequal", dict(neighbor_scan=1))
    t["index_plane:3:1"] = ("plane:40", dict(neighbor_scan=1))
    t["kdtree_unequal:4:1"] = ("unequal", dict(window_size=4))
    for k in ("q25", "q75", "exact", "above"):
        t[f"knn:{k}"] = ("vlp", dict(knn_distance_threshold=k))          # resolved by pca_case
    for v in (0.0, 0.005, float("inf")):
        t[f"distance:{v}"] = ("vlp", dict(distance_threshold=v))
    for v in (0.0, 0.5, 1.0, 1.01):
        t[f"valid_points:{v}"] = ("vlp", dict(valid_points_threshold=v))
    for v in (-1.0, 0.0, 0.3, 1.0):
        t[f"planarity:{v}"] = ("vlp", dict(planarity_threshold=v))
    t["drop_invalid"] = ("vlp", dict(use_all_points=0, distance_threshold=0.005))
    for n in (265, 266, 267):
        t[f"guarded:{n}"] = (f"guarded:{n}", dict(window_size=4, iter_step=3))
    return t


PCA_TABLE = _pca_table()
PCA_CASES = list(PCA_TABLE)


def pca_case(name):
    """(xyz, ring sizes, ImlsPcaParams) of a section-B case."""
    inp, fields = PCA_TABLE[name]
    fields = dict(fields)
    if isinstance(fields.get("knn_distance_threshold"), str):
        fields["knn_distance_threshold"] = knn_thresholds()[fields["knn_distance_threshold"]]
    return (*pca_input(inp), pca_params(**fields))


@functools.lru_cache(maxsize=None)
def pca_oracle(name):
    """The oracle's rows of a case, computed once and shared (read-only)."""
    xyz, sizes, p = pca_case(name)
    o = oc.ring_pca(xyz, sizes, p)
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def pca_oracle_all_rows(name):
    """The oracle's rows of a use_all_points = 0 case with use_all_points = 1: the rows the case drops
    are there, with the margin that says whether dropping them may flip."""
    xyz, sizes, p = pca_case(name)
    p.use_all_points = 1
    return oc.ring_pca(xyz, sizes, p)


def pca_bands(o, p):
    """Rows of the oracle where a flag may flip: (plane check: margin < 1e-6, candidate bit:
    |planarity − planarity_threshold| < 1e-6 on the rows that passed the plane check — a row that
    failed it has λ = −1 and never the candidate bit)."""
    valid = (o["flags"] & _abi.IMLS_PCA_PLANE_INVALID) == 0
    with np.errstate(invalid="ignore"):
        return o["margin"] < BAND, valid & (np.abs(o["features"][:, 5] - np.float32(p.planarity_threshold)) < BAND)


# ---- C: samplers -------------------------------------------------------------------------------

BINS = ((1, 1), (1, 8), (7, 5), (17, 16), (64, 64), (1024, 4))
MANY_BINS = ((64, 64), (1024, 4))
RADII = ((0.0, 1.5), (0.05, 1.5), (5.0, 1.5), (0.5, 0.05), (0.5, 0.3), (0.5, 50.0), (2.0, 0.5), (float("inf"), 1.5))
BRUTE_RADII = RADII[:5]
FPS_SIZES = (511, 512, 513, 1025, 8191, 8192, 8193, 20000)
FPS_BLOCK = 512                                   # k_fps: point x lives in slot x // 512 of thread x % 512
PREV_SIZES = (4095, 4096, 4097)
SHIFT = np.array([1000.0, -2000.0, 50.0], np.float32)


def sample_params(method, strategy=None, **fields):
    p = _abi.default_sample_params(method)
    if strategy is not None:
        p.sampling_strategy = strategy
    p.shuffle_seed, p.rand_seed = 11, 7
    for k, v in fields.items():
        setattr(p, k, v)
    return p


@functools.lru_cache(maxsize=None)
def frames():
    """The two VLP-16 producer frames of the sampler tests: ((xyz, normals, candidates), …)."""
    from test_gpu_sample_point_cloud import producer_frames
    out = producer_frames("vlp16")
    for f in out:
        _ro(*f)
    return out


@functools.lru_cache(maxsize=None)
def dense_normals():
    """Frame 1 with EVERY row a candidate and the normals spread over the sphere (each turned by a
    fixed random rotation of up to 60°): enough occupied bins for the 4096-bin histograms to run
    k_sw_plan's and k_sw_boff's loops past their first 256 bins."""
    (x0, _, _), (x1, n1, _) = frames()
    rng = np.random.default_rng(12)
    v = rng.normal(0, 1, n1.shape)
    n = n1.astype(np.float64) + 0.9 * v / np.linalg.norm(v, axis=1, keepdims=True)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return _ro(x1, n.astype(np.float32), np.arange(len(x1), dtype=np.int32), x0)


def bins_case(az, el, method, strategy):
    """(xyz, nrm, cand, last, params).  The small histograms take the producer frame as it is; the
    4096-bin ones take dense_normals() with bins of 2 … 3 points sampled down, so that several
    hundred bins hold a job."""
    if (az, el) in MANY_BINS or (az, el) == (65, 64):
        xyz, nrm, cand, last = dense_normals()
        p = sample_params(method, strategy, azimuth_bins=az, elevation_bins=el, min_points_per_bin=2,
                          max_points_per_bin=3, max_total_points=3000)
    else:
        (x0, _, _), (xyz, nrm, cand) = frames()
        last = x0
        p = sample_params(method, strategy, azimuth_bins=az, elevation_bins=el)
    return xyz, nrm, cand, last, p


def bin_ids(nrm, az, el):
    from test_sample_point_cloud import bin_of
    return bin_of(np.asarray(nrm, np.float32), az, el)


def edge_normals():
    """Hand-built normals on bin edges → list of (name, normal (3,) float32, (az_bins, el_bins))."""
    f = np.float32
    out = [("+x", (1, 0, 0), (8, 8)), ("-x", (-1, 0, 0), (8, 8)), ("-x,-0", (-1, -0.0, 0), (8, 8)),
           ("+z", (0, 0, 1), (8, 8)), ("-z", (0, 0, -1), (8, 8)), ("+z 7x5", (0, 0, 1), (7, 5)), ("-x 7x5", (-1, 0, 0), (7, 5)),
           # azimuth −1e-8 + 2π rounds to float(2π) = 6.2831855 > 2π: the quotient truncates to az_bins → clamped
           ("az→2π", (1, -1e-8, 0), (8, 8)), ("az→2π 7x5", (1, -1e-8, 0), (7, 5))]
    for el in (5, 7):
        for k in range(1, el):
            nz0 = f(-np.cos(k * PI / el))
            for nz in (np.nextafter(nz0, f(-2)), nz0, np.nextafter(nz0, f(2))):
                out.append((f"el {k}/{el} {float(nz)!r}", (float(np.sqrt(1 - np.float64(nz) ** 2)), 0.0, float(nz)), (8, el)))
    return [(n, np.array(v, np.float32), b) for n, v, b in out]


def edge_scene(normal):
    """Three samples carrying `normal`, each with three neighbours in the previous cloud 0.1 m away
    along the normal (cross product 0): major_axis gives its bin — and no other — a weight."""
    n = np.asarray(normal, np.float64)
    xyz = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0]], np.float32)
    last = np.concatenate([xyz + s * n for s in (0.1, 0.2, 0.3)]).astype(np.float32)
    return xyz, np.tile(np.asarray(normal, np.float32), (3, 1)), np.arange(3, dtype=np.int32), last


def edge_params(az, el, method=_abi.IMLS_SAMPLE_MAJOR_AXIS):
    return sample_params(method, _abi.SAMPLE_FPS, azimuth_bins=az, elevation_bins=el, min_points_per_bin=1,
                         max_points_per_bin=100)


@functools.lru_cache(maxsize=None)
def one_bin_cloud(n, kind="random"):
    """n points whose normals are all +z (one bin of a 1 × 1 histogram)."""
    rng = np.random.default_rng(n)
    if kind == "random":
        xyz = rng.uniform(-20, 20, (n, 3))
    elif kind == "lattice":                                 # 20 × 20 × 3 integer lattice: distances tie everywhere
        g = np.stack(np.meshgrid(np.arange(20), np.arange(20), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
        xyz = g[rng.permutation(len(g))].astype(np.float64)
        assert n == len(xyz)
    elif kind == "copies":                                  # n copies of one point: every distance is 0
        xyz = np.tile([[1.5, -2.25, 0.75]], (n, 1))
    elif kind == "duplicates":                              # 300 of the points appear twice
        xyz = rng.uniform(-20, 20, (n, 3))
        src = rng.permutation(n)[:600]
        xyz[src[300:]] = xyz[src[:300]]
    else:
        raise KeyError(kind)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (n, 1))
    return _ro(xyz.astype(np.float32), nrm)


def fps_params(method, rand_seed, k=64):
    """One bin sampled down to k points by FPS: "normal" takes k = max_points_per_bin; major_axis
    takes k = int(weight · max_total_points) with the only bin's weight 1."""
    if method == _abi.IMLS_SAMPLE_NORMAL:
        return sample_params(method, _abi.SAMPLE_FPS, azimuth_bins=1, elevation_bins=1, min_points_per_bin=1,
                             max_points_per_bin=k, rand_seed=rand_seed)
    return sample_params(method, _abi.SAMPLE_FPS, azimuth_bins=1, elevation_bins=1, min_points_per_bin=1,
                         max_points_per_bin=200, max_total_points=k, rand_seed=rand_seed)


def fps_first_index(rand_seed, n):
    """farthestPointSampling's first index: the first rand() after srand(rand_seed), modulo n."""
    return int(oc.rand_sequence(rand_seed, 1)[0]) % n


@functools.lru_cache(maxsize=None)
def fps_seeds(n):
    """rand_seed values whose first index falls in slot 0, in a middle slot (≥ 1, not the last) and in
    the last, partial slot of k_fps' register layout, where n has them: {slot name: seed}."""
    last = (n - 1) // FPS_BLOCK
    want = {"slot0": lambda s: s == 0}
    if last >= 2:
        want["middle"] = lambda s: 1 <= s < last
    if last >= 1:
        want["last"] = lambda s: s == last
    out = {}
    for seed in range(1, 4000):
        s = fps_first_index(seed, n) // FPS_BLOCK
        for k, f in want.items():
            if k not in out and f(s):
                out[k] = seed
        if len(out) == len(want):
            return out
    raise AssertionError((n, out))


def fps_last(xyz):
    """A previous cloud 0.1, 0.2 and 0.3 m above every point: each sample has its three neighbours
    however sparse the bin, so the only bin's weight is 1."""
    xyz = np.asarray(xyz, np.float32)
    return np.concatenate([xyz + np.array([0, 0, dz], np.float32) for dz in (0.1, 0.2, 0.3)]).astype(np.float32)


def radius_case(r, r_proj, strategy=_abi.SAMPLE_FPS):
    """Frame 1 against frame 0 with max_points_per_bin above every bin, so majorAxisSampling's subsets
    are the whole bins and a brute-force restatement needs no shuffle."""
    (x0, _, _), (x1, n1, c1) = frames()
    return x1, n1, c1, x0, sample_params(_abi.IMLS_SAMPLE_MAJOR_AXIS, strategy, r=r, r_proj=r_proj, max_points_per_bin=100000)


def major_weights_np(xyz, nrm, cand, last, p):
    """majorAxisSampling's normalised bin weights (670-723) in float64 by brute force, for subsets
    that are the whole bins (every bin ≤ max_points_per_bin).  NaN where the reference divides 0 by 0."""
    xyz, nrm, last = (np.asarray(a, np.float64) for a in (xyz, nrm, last))
    b = bin_ids(np.asarray(nrm, np.float32)[cand], p.azimuth_bins, p.elevation_bins)
    nb = p.azimuth_bins * p.elevation_bins
    cnt = np.zeros(len(cand), np.int64)
    tot = np.zeros(len(cand))
    l2 = (last * last).sum(1)
    for lo in range(0, len(cand), 512):
        i = np.asarray(cand[lo: lo + 512])
        # prefilter with |x|² + |l|² − 2 x·l (1 % wider than r_proj), then the pairs exactly
        approx = (xyz[i] * xyz[i]).sum(1)[:, None] + l2[None, :] - 2.0 * (xyz[i] @ last.T)
        a, j = np.nonzero(approx < (1.01 * min(p.r_proj, 1e6)) ** 2 + 1e-3)
        d = xyz[i][a] - last[j]
        dist = np.linalg.norm(d, axis=1)
        near = (dist < p.r_proj) & (np.linalg.norm(np.cross(d, nrm[i][a]), axis=1) < p.r)
        np.add.at(cnt, lo + a[near], 1)
        np.add.at(tot, lo + a[near], dist[near])
    w = np.zeros(nb)
    for k in range(nb):
        sel = b == k
        if sel.sum() < p.min_points_per_bin:
            continue
        assert sel.sum() <= p.max_points_per_bin
        v = sel & (cnt >= 3)
        if v.sum() >= 3:
            w[k] = (tot[v] / cnt[v]).sum() / v.sum()
    with np.errstate(invalid="ignore"):
        return w / w.sum()


def gate_scene(kind, shift=False, r_proj=1.5):
    """30 floor samples (normal +z) on a 4 m grid and 30 wall samples (normal +x), all coordinates
    small integers.  Every floor sample has previous-cloud points 0.25 and 0.5 m above it and a third
    one straight above at
      "at":    exactly r_proj — the strict gate (norm < r_proj, 685) leaves it out: 2 neighbours, no weight;
      "below": one ulp nearer — 3 neighbours, the floor bin gets its weight.
    Wall samples have three neighbours 0.25 / 0.5 / 0.75 m along +x.  The grid spacing keeps every
    other point farther than r_proj.  shift: the scene moved by (1000, −2000, 50) m, exact in float."""
    f = np.float32
    gx, gy = np.meshgrid(np.arange(6) * 4.0, np.arange(5) * 4.0, indexing="ij")
    floor = np.stack([gx.ravel(), gy.ravel(), np.zeros(30)], 1).astype(f)
    wall = np.stack([np.full(30, 40.0), np.arange(30) * 4.0, np.full(30, 8.0)], 1).astype(f)
    off = SHIFT if shift else np.zeros(3, f)
    floor, wall = floor + off, wall + off
    top = floor[:, 2] + f(r_proj)
    if kind == "below":
        top = np.nextafter(top, floor[:, 2])
    else:
        assert kind == "at"
    up = lambda dz: floor + np.array([0, 0, dz], f)
    third = floor.copy()
    third[:, 2] = top
    last = np.concatenate([up(0.25), up(0.5), third] + [wall + np.array([dx, 0, 0], f) for dx in (0.25, 0.5, 0.75)])
    xyz = np.concatenate([floor, wall])
    nrm = np.concatenate([np.tile([[0, 0, 1]], (30, 1)), np.tile([[1, 0, 0]], (30, 1))]).astype(f)
    p = sample_params(_abi.IMLS_SAMPLE_MAJOR_AXIS, _abi.SAMPLE_FPS, r_proj=r_proj, max_total_points=40)
    return xyz.astype(f), nrm, np.arange(60, dtype=np.int32), last.astype(f), p


def prev_size_case(m):
    """two_planes against a previous cloud of m points: 64 chunk boxes of 64 points fill k_major_avg's
    first trip over the boxes exactly at 4096."""
    xyz, nrm = two_planes(n_each=50)
    last = np.tile(xyz + np.array([0, 0, 0.1], np.float32), (m // 100 + 1, 1)).astype(np.float32)[:m]
    return xyz, nrm, np.arange(100, dtype=np.int32), last, sample_params(_abi.IMLS_SAMPLE_MAJOR_AXIS)


LIMIT_CASES = {
    "max_total_100": dict(max_total_points=100),
    "max_total_20000": dict(max_total_points=20000),
    "bin_1_513": dict(min_points_per_bin=1, max_points_per_bin=513),
    "bin_1_10000": dict(min_points_per_bin=1, max_points_per_bin=10000),
}


def limit_case(name, method, strategy):
    (x0, _, _), (x1, n1, c1) = frames()
    return x1, n1, c1, x0, sample_params(method, strategy, **LIMIT_CASES[name])


# ---- D: the chain ------------------------------------------------------------------------------

def chain_kwargs(name):
    """ScanRegistration keyword arguments of the two off-default chains."""
    if name == "index_major_axis":
        blocks = {}
        for key, method in (("normal_params", _abi.IMLS_SAMPLE_NORMAL), ("major_axis_params", _abi.IMLS_SAMPLE_MAJOR_AXIS)):
            blocks[key] = sample_params(method, _abi.SAMPLE_FPS, azimuth_bins=17, elevation_bins=16, r_proj=0.8)
        return dict(pca_params=pca_params(window_size=4, iter_step=1, neighbor_scan=1, planarity_threshold=0.1), **blocks)
    if name == "curvature_normal":
        cp = _abi.default_curvature_params()
        cp.window_size = 7
        return dict(pca_params=pca_params(window_size=3, iter_step=2), presample_method="curvature", curvature_params=cp,
                    sample_method="normal",
                    normal_params=sample_params(_abi.IMLS_SAMPLE_NORMAL, _abi.SAMPLE_RANDOM, azimuth_bins=7, elevation_bins=5))
    raise KeyError(name)


CHAINS = ("index_major_axis", "curvature_normal")


@functools.lru_cache(maxsize=None)
def chain_raws():
    """The three raw VLP-16 sweeps of test_gpu_sweep.py's chain tests."""
    sc, poses = _scene()
    return [_ro(synth.raw_sweep(sc, synth.vlp16(), poses[2 + k], 40 + k, start_deg=15.0 * k, n_nan=7, n_close=5))[0]
            for k in range(3)]
