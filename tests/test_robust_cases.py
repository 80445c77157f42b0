"""CPU: the robust M-estimator solve's ABI and configuration, and the premises of the device cases
(tests/test_gpu_robust.py) proved on the numpy restatement alone (tests/robust_np.py)."""
import ctypes as C
import pathlib
import re
import subprocess

import numpy as np
import pytest

import oracle_ctypes as oc
import pose_info_np as pin
import robust_cases as rc
import robust_np as rnp
from planetary_lidar_odometry_amd import _abi, config, sequences

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "imls_gpu.h").read_text()


# ---- ABI and configuration -------------------------------------------------------------------------
def test_header_declares_the_method_the_losses_and_the_fields():
    assert re.search(r"IMLS_SOLVE_ROBUST\s*=\s*4\b", HEADER)
    for name, val in (("HUBER", 0), ("CAUCHY", 1), ("GEMAN_MCCLURE", 2)):
        assert re.search(rf"IMLS_ROBUST_{name}\s*=\s*{val}\b", HEADER)
    body = HEADER[HEADER.index("typedef struct imls_params"):HEADER.index("} imls_params;")]
    tail = body[body.index("_reserved[4]"):]           # at the struct's end, in the union with the reserved words
    assert re.search(r"int32_t\s+robust_loss;", tail) and re.search(r"int32_t\s+robust_iterations;", tail)
    assert re.search(r"double\s+robust_scale;", tail)
    assert re.search(r"#define\s+IMLS_GPU_ABI_VERSION\s+1\b", HEADER)


def test_abi_mirror():
    assert _abi.IMLS_SOLVE_ROBUST == 4
    assert (_abi.IMLS_ROBUST_HUBER, _abi.IMLS_ROBUST_CAUCHY, _abi.IMLS_ROBUST_GEMAN_MCCLURE) == (0, 1, 2)
    tail = _abi.ImlsParams._reserved.offset               # the fields live in the struct's reserved tail
    assert tail + 16 == C.sizeof(_abi.ImlsParams)
    assert (_abi.ImlsParams.robust_loss.offset, _abi.ImlsParams.robust_iterations.offset,
            _abi.ImlsParams.robust_scale.offset) == (tail, tail + 4, tail + 8)
    p = _abi.default_params()
    assert (p.robust_loss, p.robust_scale, p.robust_iterations) == (_abi.IMLS_ROBUST_HUBER, 0.1, 5)
    assert p.solve_method == _abi.IMLS_SOLVE_RANSAC          # the shipped method stays RANSAC


def test_c_defaults_match_the_mirror():
    """as_dict skips the tail union, so the robust defaults of imls_default_params are compared here,
    with the whole struct byte for byte."""
    p = _abi.ImlsParams()
    _abi.load_library().imls_default_params(C.byref(p))
    assert (p.robust_loss, p.robust_iterations, p.robust_scale) == (_abi.IMLS_ROBUST_HUBER, 5, 0.1)
    assert bytes(p) == bytes(_abi.default_params())


def test_config_robust_block():
    cfg = config.load()
    assert bytes(config.params_from_config(cfg)) == bytes(_abi.default_params())
    sm = cfg["laser_odometry"]["solve_method"]
    sm["Robust"] = {}                                         # a block may leave keys out: the defaults hold
    p = config.params_from_config(cfg)
    assert (p.robust_loss, p.robust_scale, p.robust_iterations) == (_abi.IMLS_ROBUST_HUBER, 0.1, 5)
    sm["method"] = "Robust"
    for name, val in config.ROBUST_LOSS.items():
        sm["Robust"] = {"loss": name, "scale": 0.25, "iterations": 7}
        p = config.params_from_config(cfg)
        assert (p.solve_method, p.robust_loss, p.robust_scale, p.robust_iterations) == (4, val, 0.25, 7)
    for bad in ("Huber", "tukey", "", "l2"):
        sm["Robust"] = {"loss": bad, "scale": 0.1, "iterations": 5}
        with pytest.raises(config.ConfigError):
            config.params_from_config(cfg)
    for block in ({"loss": "huber", "scale": 0.1, "iterations": 0}, {"loss": "huber", "scale": 0.1, "iterations": 33},
                  {"loss": "huber", "scale": 0.0, "iterations": 5}, {"loss": "huber", "scale": float("nan"), "iterations": 5}):
        sm["Robust"] = block
        with pytest.raises(config.ConfigError):
            config.params_from_config(cfg)


def test_ceres_maps_to_robust_only_on_request():
    cfg = config.load()
    sm = cfg["laser_odometry"]["solve_method"]
    sm["method"] = "Ceres"
    with pytest.raises(config.ConfigError):
        config.params_from_config(cfg)
    for max_it, want in ((20, 20), (4, 4), (50, 32)):
        sm["Ceres"] = {"max_iterations": max_it}
        sm["Robust"] = {"loss": "cauchy", "scale": 0.7, "iterations": 3}      # not what Ceres maps to
        p = config.params_from_config(cfg, ceres="robust")
        assert (p.solve_method, p.robust_loss, p.robust_scale, p.robust_iterations) == \
            (_abi.IMLS_SOLVE_ROBUST, _abi.IMLS_ROBUST_HUBER, 0.1, want)
    with pytest.raises(config.ConfigError):
        config.params_from_config(cfg, ceres="yes")
    sm["method"] = "ICP"
    with pytest.raises(config.ConfigError):
        config.params_from_config(cfg, ceres="robust")


def test_halo_block_accepts_robust():
    class Odo:
        params = rc.robust_params()

        def map_push(self, cloud):
            pass

        def register(self, flat):
            return np.eye(4)

    out = sequences.run_halo_block(Odo(), [(None, None)] * 3, range(0, 1), range(1, 3))
    assert out.shape == (2, 4, 4)


def test_adapter_header_compiles(tmp_path):
    src = tmp_path / "robust_adapter.cpp"
    src.write_text(
        '#include <array>\n#include "imls_icp_hip.hpp"\n'
        "typedef std::vector<std::array<double, 3>> Cloud;\n"
        "bool f(Cloud& s, Cloud& r, Cloud& n, double (&D)[16]) {\n"
        '    return imls_hip::SolveMotionEstimationProblemRobust(s, r, n, D, "t", IMLS_ROBUST_CAUCHY, 0.1, 5);\n'
        "}\nint main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{ROOT / 'include'}", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- premises of the device cases ------------------------------------------------------------------
def _shares(a, b, loss, c, K, u=None):
    xs, _ = rnp.iterates(a, b, config.ROBUST_LOSS[loss], c, K, u)
    return [float((np.abs(pin.dot_seq(a, x) - b) > c).mean()) for x in xs[:-1]]


@pytest.mark.parametrize("loss", rc.LOSSES)
@pytest.mark.parametrize("c", rc.SCALES)
def test_outlier_set_runs_both_branches_at_every_iteration(loss, c):
    for n in (255, 4096, 4097):
        a, b = pin.rows_ab(*rc.outlier_set(n))
        for share in _shares(a, b, loss, c, 32):
            assert rc.BRANCH_SHARE <= share <= 1 - rc.BRANCH_SHARE, (n, share)
    a, b = pin.rows_ab(*rc.outlier_set())
    share0 = _shares(a, b, loss, c, 1)[0]
    assert abs(share0 - {0.1: 0.635, 0.5: 0.276}[c]) < 0.005, share0


def test_golden_rows_run_both_branches():
    """The golden pairs' recorded rows x1/y1/n1.  At k = 0 (the residual −b under the pose the ICP loop
    has reached) both branches of ψ run: 30.6 % of the vlp16 rows lie above c = 0.1 and 4.4 % of the
    planetary rows above c = 0.02 (0.4 % at c = 0.1, which is why that pair runs at 0.02).  The
    planetary rows keep ≥ 2 % on each side at every inner iteration.  The vlp16 rows do not: under x¹
    every residual is below 0.1 (measured: shares 0.306, 0, 0, 0, 0 for all three losses), so on that
    pair the c/|r| branch runs in the first inner iteration only; outlier_set() is the case that
    exercises both branches at every k (the test above)."""
    g = rc.golden("vlp16_pair")
    a, b = pin.rows_ab(g["x1"], g["y1"], g["n1"])
    for loss in rc.LOSSES:
        shares = _shares(a, b, loss, 0.1, 5)
        print("vlp16_pair", loss, shares)
        assert abs(shares[0] - 0.306) < 0.005
    g = rc.golden("planetary_pair")
    a, b = pin.rows_ab(g["x1"], g["y1"], g["n1"])
    assert abs((np.abs(b) > 0.1).mean() - 0.004) < 0.002
    for loss in rc.LOSSES:
        shares = _shares(a, b, loss, 0.02, 5)
        print("planetary_pair", loss, shares)
        assert abs(shares[0] - 0.044) < 0.005
        assert all(rc.BRANCH_SHARE <= v <= 1 - rc.BRANCH_SHARE for v in shares), shares


@pytest.mark.parametrize("loss", rc.LOSSES)
def test_robust_x_is_nearer_the_truth_than_ls(loss):
    a, b = pin.rows_ab(*rc.outlier_set())
    err_ls = np.abs(pin.solve_x(a, b) - rc.TRUE_X).max()
    xs, _ = rnp.iterates(a, b, config.ROBUST_LOSS[loss], 0.1, 5)
    err = np.abs(xs[-1] - rc.TRUE_X).max()
    print(f"{loss}: LS {err_ls:.2e} robust {err:.2e}")
    assert err < err_ls / 3
    steps = [np.abs(xs[k + 1] - xs[k]).max() for k in range(5)]
    assert all(steps[k + 1] < steps[k] / 3 for k in range(1, 4)), steps    # the inner steps shrink


@pytest.mark.parametrize("loss", rc.LOSSES)
def test_one_iteration_is_weighted_ls_under_psi_of_minus_b(loss):
    s, d, n = rc.outlier_set(257)
    a, b = pin.rows_ab(s, d, n)
    u = rc.caller_weights(257)
    w = u * rnp.psi(config.ROBUST_LOSS[loss], 0.1, -b)
    xs, ws = rnp.iterates(a, b, config.ROBUST_LOSS[loss], 0.1, 1, u)
    assert np.array_equal(ws[0], w) and np.array_equal(xs[1], pin.solve_x(a, b, w))
    # QR on √w-scaled rows and the normal equations agree far inside the device tolerance
    H = (a * w[:, None]).T @ a
    assert np.abs(np.linalg.solve(H, (a * w[:, None]).T @ b) - xs[1]).max() < 1e-12


def test_psi_values():
    r = np.array([0.0, 0.05, -0.1, 0.2, -0.4])
    assert np.allclose(rnp.psi(0, 0.1, r), [1, 1, 1, 0.5, 0.25], rtol=0, atol=1e-16)
    assert np.allclose(rnp.psi(1, 0.1, r), 1 / (1 + (r / 0.1) ** 2), rtol=1e-15)
    assert np.allclose(rnp.psi(2, 0.1, r), (0.01 / (0.01 + r * r)) ** 2, rtol=1e-15)


def test_below_scale_rows_are_unit_weight_ls():
    s, d, n = rc.below_scale_set()
    a, b = pin.rows_ab(s, d, n)
    xs, ws = rnp.iterates(a, b, _abi.IMLS_ROBUST_HUBER, 0.5, 5)
    assert all((w == 1.0).all() for w in ws)
    assert max(np.abs(pin.dot_seq(a, x) - b).max() for x in xs) < 0.25


def test_corridor_is_rank_five():
    from test_gpu_ls_conditioning import corridor, targets
    s, nrm = corridor(4000, 0.0, 6)
    a, b = pin.rows_ab(s, targets(s, nrm, 6), nrm)
    assert not a[:, 3].any()                                   # no row sees t_x
    xs, _ = rnp.iterates(a, b, _abi.IMLS_ROBUST_HUBER, 0.1, 5)
    assert all(x[3] == 0.0 for x in xs) and np.abs(xs[-1]).max() > 0.01


@pytest.mark.parametrize("n", rc.PROJECT_SIZES)
def test_planes_scene_keeps_every_row(n):
    p = rc.robust_params()
    src, tgt = rc.planes_source(n), rc.planes_map()
    x, y, nr, idx, rej = oc.project(np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T), np.eye(4), p)
    assert len(idx) == n and not rej.any()
    if n >= 64:
        a, b = pin.rows_ab(x, y, nr)
        for share in _shares(a, b, "huber", 0.1, 5):
            assert rc.BRANCH_SHARE <= share <= 1 - rc.BRANCH_SHARE, share


@pytest.mark.parametrize("name", list(rc.FRAMES))
def test_frames_cover_their_row_ranges(name):
    build, c, (lo, hi) = rc.FRAMES[name]
    src, tgt = build()
    p = rc.robust_params(scale=c, iters=rc.FRAME_ITERS)
    r = rnp.register_from(np.ascontiguousarray(rc.rows6(src).T), np.ascontiguousarray(rc.rows6(tgt).T), p)
    assert r["iters"] == rc.FRAME_ITERS or r["status"] == _abi.IMLS_FRAME_CONVERGED
    assert all(lo <= t["n_valid"] < hi for t in r["trace"]), [t["n_valid"] for t in r["trace"]]
