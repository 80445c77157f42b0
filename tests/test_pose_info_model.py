"""CPU tests of the pose-info report's definition (tests/pose_info_np.py, the numpy restatement of
include/imls_gpu.h `struct imls_pose_info`): that the reported covariance means something, that the
DRPM probabilities and the RANSAC inliers restated there are the oracle's, the degenerate geometry,
the covariance chain of the driver, the premises of the device cases, and the ABI mirror."""
import ctypes as C
import pathlib
import re
import subprocess

import numpy as np
import pytest

import oracle_ctypes as oc
import pose_info_cases as cases
import pose_info_np as pin
from planetary_lidar_odometry_amd import _abi, imls_icp
from ransac_cases import outlier_set, shipped_params

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "imls_gpu.h"


# ---- the covariance means something ----------------------------------------------------------------
def _monte_carlo(t, seed=5, rows=500, sigma=0.01, trials=400):
    """Per diagonal: sample variance of the estimate over the trials / mean reported variance."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-15, 15, (rows, 3))
    n = rng.normal(0, 1, (rows, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    x_true = np.array([0.01, -0.02, 0.015, 0.2, -0.1, 0.05])
    a, _ = pin.rows_ab(s, s, n)
    b0 = a @ x_true
    xs, var = [], []
    for _ in range(trials):
        d = s + n * (b0 + rng.normal(0, sigma, rows))[:, None]      # b = n·(d − s) = b0 + noise
        r = pin.restate_ls(s, d, n, t)
        xs.append(r["x"])
        var.append(np.diag(r["covariance"]))
    return np.var(np.array(xs), axis=0, ddof=1) / np.mean(var, axis=0)


def test_covariance_matches_the_sample_variance_untrimmed():
    """500 well-spread rows, Gaussian noise σ = 0.01 on b, 400 trials: the estimator of a variance
    ratio has a relative spread of √(2/399) = 0.071, so [0.75, 1.3] is about ±3.5 σ."""
    ratio = _monte_carlo(0.0)
    print("ratio", ratio)
    assert ratio.min() >= 0.75 and ratio.max() <= 1.3, ratio


def test_covariance_is_optimistic_under_trimming():
    """The documented bias: at ls_threshold 0.02 the reported variance is below the sample variance."""
    ratio = _monte_carlo(0.02)
    print("ratio", ratio)
    assert ratio.min() >= 0.9 and ratio.max() <= 1.6, ratio


# ---- the restated solvers are the oracle's ----------------------------------------------------------
def test_drpm_probabilities_pinned_to_the_oracle_on_the_degenerate_plane():
    s, d, n = cases.plane_rows()
    p = shipped_params(final="DRPM")
    w = np.ones(len(s))
    r = pin.drpm(s, d, n, w, p.drpm_threshold, p.drpm_stdev_points, p.drpm_stdev_normals)
    assert r["degenerate"] and r["prob"].min() < p.drpm_threshold
    ok, D = oc.solve(_abi.IMLS_SOLVE_DRPM, s, d, n, p, weights=w)
    assert ok
    x = r["U"].T @ (np.where(np.abs(r["ev"]) > 1e-10, r["prob"] / r["ev"], 0.0) * (r["U"] @ r["g"]))
    err = np.abs(oc.delta_from_x(x) - D).max()
    print("|Δ(x) − oracle|", err, "p", r["prob"])
    assert err <= 1e-12


@pytest.mark.parametrize("final", ["LS", "WLS", "DRPM"])
def test_restated_ransac_is_the_oracles(final):
    """The numpy hypothesis loop picks the oracle's inliers: Δ of the restated final solve equals
    oc.solve's (1e-9: the final solves differ only in how their sums associate)."""
    s, d, n = outlier_set(4000, 0.02, 7)
    p = shipped_params(final=final)
    r = pin.restate_ransac(s, d, n, p)
    ok, D = oc.solve(_abi.IMLS_SOLVE_RANSAC, s, d, n, p)
    err = np.abs(oc.delta_from_x(r["x"]) - D).max()
    print(final, "inliers", len(r["inliers"]), "|Δ − oracle|", err)
    assert ok and err <= 1e-9


@pytest.mark.parametrize("N", [65, 1031])
@pytest.mark.parametrize("t", cases.THRESHOLDS)
def test_restated_ls_is_the_oracles(N, t):
    s, d, n = cases.solve_rows(N)
    p = shipped_params()
    p.ls_threshold = t
    ok, D = oc.solve(_abi.IMLS_SOLVE_LS, s, d, n, p)
    r = pin.restate_ls(s, d, n, t)
    assert ok and np.abs(oc.delta_from_x(r["x"]) - D).max() <= 1e-12
    lo, hi = pin.trim_ranks(N, t)
    assert r["n_rows"] == hi - lo + 1


# ---- degenerate geometry ----------------------------------------------------------------------------
def test_flat_plane_has_rank_three_and_a_zero_covariance_on_its_null_space():
    s, d, n = cases.flat_rows()
    r = pin.restate_wls(s, d, n)
    assert r["rank"] == 3 and r["flags"] & _abi.IMLS_INFO_RANK_DEFICIENT and not r["flags"] & _abi.IMLS_INFO_NO_DOF
    null = r["eigenvectors"][:3]
    # span{ωz, tx, ty} exactly: the rows' columns 2, 3, 4 are exactly zero
    assert np.all(null[:, [0, 1, 5]] == 0)
    assert np.linalg.matrix_rank(null[:, [2, 3, 4]]) == 3
    for k in (2, 3, 4):
        assert np.all(r["covariance"][k] == 0) and np.all(r["covariance"][:, k] == 0)
    assert np.all(np.diag(r["covariance"])[[0, 1, 5]] > 0)


def test_sign_rule_and_tie():
    U = np.eye(6)
    U[0] = [-0.5, 0.5, 0, 0, 0, np.sqrt(0.5)]
    U[1] = [0.5, -0.5, 0, 0, 0, -np.sqrt(0.5)]
    U[2] = [-np.sqrt(0.5), np.sqrt(0.5), 0, 0, 0, 0]       # a tie: the first component decides
    P = pin.pin_sign(U)
    assert P[0, 5] > 0 and P[1, 5] > 0 and P[2, 0] > 0 and P[2, 1] < 0


# ---- adjoint / propagate_covariance -----------------------------------------------------------------
def _random_pose(rng, rot=0.4, tr=5.0):
    return pin.exp_pose(np.concatenate([rng.normal(0, rot, 3), rng.normal(0, tr, 3)]))


def test_adjoint_and_propagation_against_finite_differences():
    rng = np.random.default_rng(17)
    h = 1e-5
    prev = np.eye(4)
    for _ in range(5):                    # a chain nowPose = prevPose·rPose
        rel = _random_pose(rng, 0.1, 1.0)
        now = prev @ rel
        now_inv = np.linalg.inv(now)

        def f(xp, xr):
            return pin.log_pose(pin.exp_pose(xp) @ prev @ pin.exp_pose(xr) @ rel @ now_inv)

        Jp, Jr = np.zeros((6, 6)), np.zeros((6, 6))
        for k in range(6):
            e = np.zeros(6)
            e[k] = h
            Jp[:, k] = (f(e, np.zeros(6)) - f(-e, np.zeros(6))) / (2 * h)
            Jr[:, k] = (f(np.zeros(6), e) - f(np.zeros(6), -e)) / (2 * h)
        A = imls_icp.adjoint(prev)
        assert np.abs(Jp - np.eye(6)).max() <= 1e-6
        assert np.abs(Jr - A).max() <= 1e-6 * max(1.0, np.abs(A).max())
        Sp, Sr = (lambda m: m @ m.T)(rng.normal(0, 1e-3, (6, 6))), (lambda m: m @ m.T)(rng.normal(0, 1e-3, (6, 6)))
        want = Jp @ Sp @ Jp.T + Jr @ Sr @ Jr.T
        got = imls_icp.propagate_covariance(Sp, prev, Sr)
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
        prev = now


def test_covariance_to_ros_reorders_to_translation_first():
    S = np.arange(36, dtype=np.float64).reshape(6, 6)
    S = S + S.T
    ros = imls_icp.covariance_to_ros(S).reshape(6, 6)
    assert np.array_equal(ros[:3, :3], S[3:, 3:]) and np.array_equal(ros[3:, 3:], S[:3, :3])
    assert np.array_equal(ros[:3, 3:], S[3:, :3]) and np.array_equal(ros, ros.T)


# ---- premises of the device cases -------------------------------------------------------------------
@pytest.mark.parametrize("N", cases.SIZES)
@pytest.mark.parametrize("t", cases.THRESHOLDS)
def test_trim_boundaries_are_well_separated(N, t):
    """The device's Cholesky x₀ and the restatement's QR x₀ differ by ~1e-13 relative: with a gap of at
    least 1e-9 × median |r₁| on both sides of both boundary ranks they order the boundary rows alike."""
    r = pin.restate_ls(*cases.solve_rows(N), t)
    print(N, t, "gap / median", r["gap"], "gap / row scale", r["gap_scale"])
    assert r["gap"] >= 1e-9
    if N == 6:
        # six rows, six unknowns: the first solve fits them exactly, every |r₁| is rounding noise and
        # the gap above is noise over noise.  Untrimmed (t = 0, 0.02) nothing depends on the order; at
        # t = 0.25 the kept rows are not determined, and the device test finds them among the subsets
        assert r["gap_scale"] < 1e-9 and (r["trimmed"] == (t == 0.25))
    else:
        assert r["gap_scale"] >= 1e-9 or not r["trimmed"]


def test_sentinel_premise():
    lo, hi = pin.trim_ranks(1031, cases.SENTINEL_T)
    kept = {}
    for side in ("in", "out"):
        s, d, n = cases.sentinel_rows(side)
        r = pin.restate_ls(s, d, n, cases.SENTINEL_T)
        a, b = pin.rows_ab(s, d, n)
        r1 = np.abs(pin.dot_seq(a, r["x0"]) - b)
        rank = int((np.lexsort((np.arange(len(b)), r1)) == cases.SENTINEL_ROW).nonzero()[0][0])
        assert rank == (hi if side == "in" else hi + 1), (side, rank, hi)
        assert r["gap"] >= 1e-9 and r["n_rows"] == hi - lo + 1
        assert (cases.SENTINEL_ROW in r["members"]) == (side == "in")
        kept[side] = r
    # the two reports differ by far more than the device bound 2·n·ε·Σ|term|
    diff = np.abs(kept["in"]["hessian"] - kept["out"]["hessian"])
    bound = 2 * kept["in"]["n_rows"] * pin.EPS * kept["in"]["abs_hessian"]
    assert (diff > 1e3 * bound).any()


@pytest.mark.parametrize("N", [4000, 16385])
def test_known_clean_rows_are_not_ransacs_inliers(N):
    """Why the device's RANSAC cases (outlier_set(N, 0.02, 7), shipped parameters) take their inliers
    from the restated hypothesis loop: under the shipped 0.8 m threshold corrupted rows land inside the
    band by chance, so the inliers are not the set's clean rows."""
    s, d, n = outlier_set(N, 0.02, 7)
    p = shipped_params(final="WLS")
    inl, w, draws = pin.ransac_inliers(s, d, n, p)
    a = 0.02
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    clean = np.abs(d - (s @ R.T + np.array([0.3, -0.1, 0.05]))).max(1) < 1e-9
    print("N", N, "inliers", len(inl), "clean", int(clean.sum()), "draws", draws)
    assert abs(w.sum() - 1) < 1e-12
    assert len(inl) != int(clean.sum())


# ---- ABI --------------------------------------------------------------------------------------------
def test_pose_info_layout_matches_c(tmp_path):
    fields = [f for f, _ in _abi.ImlsPoseInfo._fields_]
    prog = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
            'printf("%zu\\n", sizeof(struct imls_pose_info));', 'printf("%zu\\n", sizeof(imls_iter_trace));',
            'printf("%zu\\n", sizeof(imls_params));']
    prog += [f'printf("%zu\\n", offsetof(struct imls_pose_info, {f}));' for f in fields]
    prog += ["return 0;}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == C.sizeof(_abi.ImlsPoseInfo)
    assert vals[1] == C.sizeof(_abi.ImlsIterTrace) and vals[2] == C.sizeof(_abi.ImlsParams)
    for f, off in zip(fields, vals[3:]):
        assert getattr(_abi.ImlsPoseInfo, f).offset == off, f


def test_pose_info_symbols_and_constants():
    lib = _abi.load_library()
    assert lib.imls_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (imls_\w+)", out))
    for name in ("imls_capture_pose_info", "imls_pose_info"):
        assert name in exported and name in _abi.ABI_SYMBOLS and hasattr(lib, name)
    text = HEADER.read_text()
    for name in ("VALID", "RANK_DEFICIENT", "NO_DOF", "DRPM_RAN", "DRPM_DEGENERATE"):
        m = re.search(rf"IMLS_INFO_{name}\s*=\s*(\d+)", text)
        assert m and int(m.group(1)) == getattr(_abi, f"IMLS_INFO_{name}"), name
    m = re.search(r"#define IMLS_INFO_RANK_RELTOL\s+(\S+)", text)
    assert m and float(m.group(1)) == _abi.IMLS_INFO_RANK_RELTOL


def test_cpp_adapter_pose_info_compiles(tmp_path):
    src = tmp_path / "adapter.cpp"
    src.write_text(f'''
#include "{ROOT / "include" / "imls_icp_hip.hpp"}"
using namespace imls_hip;
int main() {{
  IMLSICPMatcherHip m;
  m.capturePoseInfo(true);
  double P[16]; m.registerFrame(P);
  const struct imls_pose_info info = m.poseInfo();   // the covariance slot of IMLSICPMatcher::Match
  return info.flags & IMLS_INFO_VALID ? 0 : 1; }}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{ROOT / 'include'}", str(src)],
                   check=True)
