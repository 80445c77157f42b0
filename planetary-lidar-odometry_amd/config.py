"""config.json ↔ imls_params.

Accepts the reference's config.json layout unchanged (the ``laser_odometry`` section that
laser_odometry.cpp reads at 487-518, 570, 606, 640-641 and the dispatcher 183-243) plus one new
key, ``laser_odometry.backend`` ("hip" — the only backend this package ships).  Method names are
the reference's strings: matching "IMLS" / "plane_ICP"; solving "LS" / "RANSAC" / "Ceres" / "ICP" /
"Teaser", plus this package's "Robust" (the M-estimator solve, block ``solve_method.Robust``); RANSAC final "LS" / "Weighted LS" / "DRPM".

producer_from_config() reads the ``scan_registration`` section (scan_registration.cpp:771-799, 935,
1073, 1132-1145, 1451, 1464, 1479) the same way: compute_normal_method "pca" on format
"pointcloud"; presample_method "geometric_features" / "curvature"; sample_method "major_axis" /
"normal" / "three_axis" / "random".
"""
from __future__ import annotations

import json
import pathlib

from . import _abi

DEFAULT_CONFIG = pathlib.Path(__file__).resolve().parent / "config" / "config.json"

MATCHING = {"IMLS": _abi.IMLS_MATCH_IMLS, "plane_ICP": _abi.IMLS_MATCH_PLANE_ICP}
# The top-level solve_method names the reference's dispatcher accepts (laser_odometry.cpp:183-272).
# "Weighted LS" is only a RANSAC final method there: as a top-level name it hits "Invalid
# SOLVE_METHOD!", so it is rejected here too (the C ABI's IMLS_SOLVE_WEIGHTED_LS is an extension
# for callers that want a unit-weight WLS loop, never produced from a config file).
SOLVING = {"LS": _abi.IMLS_SOLVE_LS, "RANSAC": _abi.IMLS_SOLVE_RANSAC, "Robust": _abi.IMLS_SOLVE_ROBUST}
# solve_method.Robust.loss (the robust M-estimator solve, include/imls_gpu.h imls_robust_loss)
ROBUST_LOSS = {"huber": _abi.IMLS_ROBUST_HUBER, "cauchy": _abi.IMLS_ROBUST_CAUCHY,
               "geman_mcclure": _abi.IMLS_ROBUST_GEMAN_MCCLURE}
ROBUST_MAX_ITERATIONS = 32
FINAL = {"LS": _abi.IMLS_FINAL_LS, "Weighted LS": _abi.IMLS_FINAL_WEIGHTED_LS, "DRPM": _abi.IMLS_FINAL_DRPM}
# Third-party solver engines (solver.cpp:25-72, 387-483): outside the GPU path.
UNSUPPORTED_SOLVERS = ("Ceres", "ICP", "Teaser")


class ConfigError(ValueError):
    pass


def load(path: str | pathlib.Path | None = None) -> dict:
    """Parse a config file.  Like common.cpp:8-17 a missing file raises (runtime_error there)."""
    p = pathlib.Path(path) if path else DEFAULT_CONFIG
    if not p.exists():
        raise FileNotFoundError(f"cannot open config file: {p}")
    with open(p) as f:
        return json.load(f)


def params_from_config(cfg: dict, ceres: str | None = None) -> _abi.ImlsParams:
    """Build imls_params from the reference key paths.  Unknown method names raise ConfigError.
    ``ceres="robust"`` (opt-in; by default "Ceres" is refused) maps solve_method "Ceres" to the Robust
    solve with the reference's HuberLoss(0.1) and K = min(Ceres.max_iterations, 32): the same cost,
    linearised at each ICP iteration's pose — not Ceres's own iterates.
    Deliberate change, documented in INTEGRATION.md: the reference prints "Invalid
    MATCHING_METHOD!" / "Invalid SOLVE_METHOD!" and keeps running with every frame's solve failing
    (rPose = I for every frame); this fails once, at configuration time."""
    lo = cfg["laser_odometry"]
    mm = lo["matching_method"]
    sm = lo["solve_method"]
    p = _abi.default_params()
    if mm["method"] not in MATCHING:
        raise ConfigError(f"Invalid MATCHING_METHOD! {mm['method']!r}")
    p.matching_method = MATCHING[mm["method"]]
    p.correspond_number = int(mm["correspond_number"])
    im = mm["IMLS"]
    p.h, p.r = float(im["h"]), float(im["r"])
    tv = im["use_tensor_voting"]
    p.use_tensor_voting, p.tensor_k = int(bool(tv["enabled"])), int(tv["k"])
    p.tensor_sigma, p.tensor_distance_threshold = float(tv["sigma"]), float(tv["distance_threshold"])
    gn = im["get_normals"]
    p.get_normals, p.r_normal, p.search_number_normal = int(bool(gn["enabled"])), float(gn["r_normal"]), int(gn["search_number_normal"])
    pd = im["use_projected_distance"]
    p.use_projected_distance, p.r_proj = int(bool(pd["enabled"])), float(pd["r_proj"])
    nac = im["normal_angle_constraint"]
    p.normal_angle_constraint, p.angle_diff_threshold = int(bool(nac["enabled"])), float(nac["angle_diff_threshold"])
    p.search_number = int(im["IMLS function"]["search_number"])
    pi = mm.get("plane_ICP")
    if pi:
        p.picp_r = float(pi["r"])
        p.picp_use_projected_distance = int(bool(pi["use_projected_distance"]["enabled"]))
        p.picp_r_proj = float(pi["use_projected_distance"]["r_proj"])
        p.picp_normal_angle_constraint = int(bool(pi["normal_angle_constraint"]["enabled"]))
        p.picp_angle_diff_threshold = float(pi["normal_angle_constraint"]["angle_diff_threshold"])
    method = sm["method"]
    if ceres not in (None, "robust"):
        raise ConfigError(f"ceres={ceres!r}: only 'robust' (or None: refuse the name) is known")
    rb = sm.get("Robust", {})
    if method == "Ceres" and ceres == "robust":
        method = "Robust"
        rb = {"loss": "huber", "scale": 0.1,
              "iterations": min(int(sm.get("Ceres", {}).get("max_iterations", 20)), ROBUST_MAX_ITERATIONS)}
    if method in UNSUPPORTED_SOLVERS:
        raise ConfigError(f"solve_method {method!r} is a third-party solver engine outside the GPU path")
    if method not in SOLVING:
        raise ConfigError(f"Invalid SOLVE_METHOD! {method!r}")
    p.solve_method = SOLVING[method]
    p.iterations = int(sm["iterations"])
    p.delta_dist_threshold = float(sm["delta_dist_threshold"])
    p.delta_angle_threshold = float(sm["delta_angle_threshold"])
    p.ls_threshold = float(sm["LS"]["threshold"])
    if "loss" in rb:
        if rb["loss"] not in ROBUST_LOSS:
            raise ConfigError(f"Invalid Robust.loss {rb['loss']!r}: one of {sorted(ROBUST_LOSS)}")
        p.robust_loss = ROBUST_LOSS[rb["loss"]]
    if "scale" in rb:
        p.robust_scale = float(rb["scale"])
    if "iterations" in rb:
        p.robust_iterations = int(rb["iterations"])
    if method == "Robust":
        if not 1 <= p.robust_iterations <= ROBUST_MAX_ITERATIONS:
            raise ConfigError(f"Robust.iterations {p.robust_iterations}: the GPU path takes 1 … {ROBUST_MAX_ITERATIONS}")
        if not (0.0 < p.robust_scale < float("inf")):
            raise ConfigError(f"Robust.scale {p.robust_scale!r} must be finite and > 0")
    rs = sm["RANSAC"]
    p.ransac_max_iterations = int(rs["max_iterations"])
    p.ransac_distance_threshold = float(rs["distance_threshold"])
    p.ransac_min_inliers_percentage = float(rs["min_inliers_percentage"])
    p.ransac_huber_threshold = float(rs["huber_threshold"])
    if rs["final_solve_method"] not in FINAL:
        raise ConfigError(f"Invalid FINAL_SOLVE_METHOD in RANSAC! {rs['final_solve_method']!r}")
    p.ransac_final_method = FINAL[rs["final_solve_method"]]
    p.ransac_ls_threshold = float(rs["LS_threshold"])
    p.drpm_threshold = float(rs["DRPM_threshold"])
    p.drpm_stdev_points = float(rs["DRPM_stdev_points"])
    p.drpm_stdev_normals = float(rs["DRPM_stdev_normals"])
    p.transform_normal = int(bool(lo.get("transform_normal", False)))
    p.max_queue_size = int(lo.get("max_queue_size", 1))
    backend = lo.get("backend", "hip")
    if backend != "hip":
        raise ConfigError(f"laser_odometry.backend {backend!r}: only 'hip' is shipped")
    return p


# scan_registration: the producer configurations the reference marks as verified run on the GPU; the
# others it lists (its own results table marks them as not working) are refused by name.
NORMAL_FORMATS = ("pointcloud",)
NORMAL_METHODS = ("pca",)
UNSUPPORTED_NORMAL_FORMATS = ("range_image",)
UNSUPPORTED_NORMAL_METHODS = ("cross_product", "FALS", "SRI")
PRESAMPLE = ("geometric_features", "curvature")
UNSUPPORTED_PRESAMPLE = ("tensor_voting",)
SAMPLE = ("major_axis", "normal", "three_axis", "random")
NEIGHBOR_SCAN = {"kdtree": 0, "index": 1}
SAMPLING_STRATEGY = {"FPS": _abi.SAMPLE_FPS, "random": _abi.SAMPLE_RANDOM}


def _sample_block(block: dict, method: int) -> _abi.ImlsSampleParams:
    sp = _abi.default_sample_params(method)
    if "r" in block:
        sp.r = float(block["r"])
    if "r_proj" in block:
        sp.r_proj = float(block["r_proj"])
    if "max_total_points" in block:
        sp.max_total_points = int(block["max_total_points"])
    for key in ("azimuth_bins", "elevation_bins", "min_points_per_bin", "max_points_per_bin"):
        if key in block:
            setattr(sp, key, int(block[key]))
    if "sampling_strategy" in block:
        if block["sampling_strategy"] not in SAMPLING_STRATEGY:
            raise ConfigError(f"Invalid sampling_strategy {block['sampling_strategy']!r}")
        sp.sampling_strategy = SAMPLING_STRATEGY[block["sampling_strategy"]]
    return sp


def producer_from_config(cfg: dict, ctx=None, **kwargs):
    """Build the GPU producer (producer.ScanRegistration) from the reference's scan_registration key
    paths.  A key the file leaves out keeps its shipped value (a file without the section selects
    the shipped pca → geometric_features → major_axis chain).  Methods outside the GPU path raise
    ConfigError naming the method (the reference prints "Invalid …_METHOD!" and publishes empty
    clouds; this fails once, at configuration time).  The context is created at the producer's
    first use unless `ctx` is given, so a configuration can be validated without a GPU."""
    from .producer import ScanRegistration

    sr = cfg.get("scan_registration", {})
    cn = sr.get("compute_normal_method", {})
    fmt, method = cn.get("format", "pointcloud"), cn.get("method", "pca")
    if fmt in UNSUPPORTED_NORMAL_FORMATS:
        raise ConfigError(f"compute_normal_method.format {fmt!r} (FALS / SRI range images) is outside the GPU path")
    if fmt not in NORMAL_FORMATS:
        raise ConfigError(f"Invalid compute_normal_method.format {fmt!r}")
    if method in UNSUPPORTED_NORMAL_METHODS:
        raise ConfigError(f"compute_normal_method {method!r} is outside the GPU path (the reference marks it not working)")
    if method not in NORMAL_METHODS:
        raise ConfigError(f"Invalid COMPUTE_NORMAL_METHOD! {method!r}")
    pca = _abi.default_pca_params()
    pb = cn.get("pca", {})
    if "window_size" in pb:
        pca.window_size = int(pb["window_size"])
    if "iter_step" in pb:
        pca.iter_step = int(pb["iter_step"])
    if "knn_distance_threshold" in pb:
        pca.knn_distance_threshold = float(pb["knn_distance_threshold"])
    if "neighbor_scan" in pb:
        if pb["neighbor_scan"] not in NEIGHBOR_SCAN:
            raise ConfigError(f"Invalid pca.neighbor_scan {pb['neighbor_scan']!r}")
        pca.neighbor_scan = NEIGHBOR_SCAN[pb["neighbor_scan"]]
    pc = pb.get("plane_constraint", {})
    if "distance_threshold" in pc:
        pca.distance_threshold = float(pc["distance_threshold"])
    if "valid_points_threshold" in pc:
        pca.valid_points_threshold = float(pc["valid_points_threshold"])
    if "use_all_points" in sr.get("model", {}):
        pca.use_all_points = int(bool(sr["model"]["use_all_points"]))
    ps = sr.get("presample_method", {})
    presample = ps.get("method", "geometric_features")
    if presample in UNSUPPORTED_PRESAMPLE:
        raise ConfigError(f"presample_method {presample!r} is outside the GPU path (the reference marks it not working)")
    if presample not in PRESAMPLE:
        raise ConfigError(f"Invalid PRESAMPLE_METHOD! {presample!r}")
    if "planarity_threshold" in ps.get("geometric_features", {}):
        pca.planarity_threshold = float(ps["geometric_features"]["planarity_threshold"])
    curv = _abi.default_curvature_params()
    cb = ps.get("curvature", {})
    if "curvature_threshold" in cb:
        curv.curvature_threshold = float(cb["curvature_threshold"])
    if "window_size" in cb:
        curv.window_size = int(cb["window_size"])
    sm = sr.get("sample_method", {})
    sample = sm.get("method", "major_axis")
    if sample not in SAMPLE:
        raise ConfigError(f"Invalid SAMPLE_METHOD! {sample!r}")
    points_per_list = int(sm.get("three_axis", {}).get("points_per_list", 200))
    if not 1 <= points_per_list <= _abi.THREE_AXIS_MAX_POINTS_PER_LIST:
        raise ConfigError(f"three_axis.points_per_list {points_per_list}: the GPU path takes 1 … "
                          f"{_abi.THREE_AXIS_MAX_POINTS_PER_LIST}")
    return ScanRegistration(ctx=ctx, pca_params=pca, sample_method=sample, presample_method=presample,
                            curvature_params=curv, points_per_list=points_per_list,
                            max_points=int(sm.get("random", {}).get("max_points", 2000)),
                            normal_params=_sample_block(sm.get("normal", {}), _abi.IMLS_SAMPLE_NORMAL),
                            major_axis_params=_sample_block(sm.get("major_axis", {}), _abi.IMLS_SAMPLE_MAJOR_AXIS),
                            **kwargs)


def bench_params(iterations: int = 20) -> _abi.ImlsParams:
    """shipped IMLS parameters, LS (t = 0.02), fixed iteration count
    (delta thresholds −1 so the convergence test never fires)."""
    p = params_from_config(load())
    p.solve_method = _abi.IMLS_SOLVE_LS
    p.iterations = iterations
    p.delta_dist_threshold = -1.0
    p.delta_angle_threshold = -1.0
    return p
