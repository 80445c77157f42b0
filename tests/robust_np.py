"""numpy restatement of the robust M-estimator solve (IMLS_SOLVE_ROBUST, include/imls_gpu.h), for
tests/test_robust_cases.py (CPU) and tests/test_gpu_robust.py (device).  No GPU imports.

With (a_i, b_i) the point-to-plane rows (solver.cpp:95-103, pose_info_np.rows_ab), u_i the caller's
weight (else 1) and x⁰ = 0, for k = 0 … K−1:
    r_i = a_i·xᵏ − b_i,   w_i = u_i·ψ(r_i; c),   xᵏ⁺¹ = argmin Σ w_i (a_i·x − b_i)²
each step solved by the oracle's column-pivoted Householder QR on the √w-scaled rows (the project's
parity contract: QR in the oracle, normal equations on the device); Δ = oc.delta_from_x(x^K).
ψ: Huber 1 for |r| ≤ c, else c/|r|; Cauchy 1/(1 + r²/c²); Geman-McClure (c²/(c² + r²))².
"""
import math

import numpy as np

import oracle_ctypes as oc
import pose_info_np as pin
from planetary_lidar_odometry_amd import _abi

LOSSES = {"huber": _abi.IMLS_ROBUST_HUBER, "cauchy": _abi.IMLS_ROBUST_CAUCHY,
          "geman_mcclure": _abi.IMLS_ROBUST_GEMAN_MCCLURE}


def psi(loss, c, r):
    r = np.asarray(r, dtype=np.float64)
    if loss == _abi.IMLS_ROBUST_HUBER:
        ar = np.abs(r)
        return np.where(ar <= c, 1.0, c / np.where(ar > 0, ar, 1.0))
    c2, r2 = c * c, r * r
    if loss == _abi.IMLS_ROBUST_CAUCHY:
        return 1.0 / (1.0 + r2 / c2)
    if loss == _abi.IMLS_ROBUST_GEMAN_MCCLURE:
        t = c2 / (c2 + r2)
        return t * t
    raise ValueError(loss)


def iterates(a, b, loss, c, K, u=None):
    """[x⁰ = 0, x¹, …, x^K] and the weights [w⁰ … w^{K−1}] each step solved under."""
    u = np.ones(len(b)) if u is None else np.asarray(u, dtype=np.float64)
    xs, ws = [np.zeros(6)], []
    for _ in range(K):
        r = pin.dot_seq(a, xs[-1]) - b
        w = u * psi(loss, c, r)
        ws.append(w)
        xs.append(pin.solve_x(a, b, w))
    return xs, ws


def solve_rows(s, d, n, p, weights=None):
    """(ok, Δ) of the stand-alone robust solve under p's robust_* fields; no row → (False, I)."""
    a, b = pin.rows_ab(s, d, n)
    if len(b) == 0:
        return False, np.eye(4)
    xs, _ = iterates(a, b, p.robust_loss, p.robust_scale, p.robust_iterations, weights)
    return True, oc.delta_from_x(xs[-1])


def restate_info(s, d, n, p, weights=None):
    """The pose-info report of a robust solve: every row, the weights of the last 6×6 system."""
    a, b = pin.rows_ab(s, d, n)
    xs, ws = iterates(a, b, p.robust_loss, p.robust_scale, p.robust_iterations, weights)
    out = pin.report(a, b, ws[-1], xs[-1])
    out.update(members=np.arange(len(b)), weights=ws[-1], x_prev=xs[-2])
    return out


def register_from(src6, tgt6, p, init=None):
    """The ICP loop of laser_odometry.cpp:478-660 (model_restatement.register_from) with the robust
    solve in place of the oracle's: oc.project, the too-few gate, Δ, rPose = Δ·rPose, the convergence
    test."""
    pose = np.eye(4) if init is None else np.array(init, dtype=np.float64).reshape(4, 4)
    status, iters, trace = _abi.IMLS_FRAME_MAX_ITERS, 0, []
    for it in range(p.iterations):
        iters = it
        x, y, n, idx, _rej = oc.project(src6, tgt6, pose, p)
        if len(idx) < p.correspond_number:
            status = _abi.IMLS_FRAME_TOO_FEW
            break
        ok, D = solve_rows(x, y, n, p)
        if not ok:
            status = _abi.IMLS_FRAME_SOLVE_FAILED
            break
        pose = oc.chain_pose(D, pose)
        trace.append(dict(n_valid=len(idx), pose=pose.copy(), delta=D.copy()))
        dd = math.sqrt(D[0, 3] ** 2 + D[1, 3] ** 2 + D[2, 3] ** 2)
        ct = min(1.0, max(((D[0, 0] + D[1, 1] + D[2, 2]) - 1.0) / 2.0, -1.0))
        iters = it + 1
        if dd < p.delta_dist_threshold and math.acos(ct) < p.delta_angle_threshold:
            status = _abi.IMLS_FRAME_CONVERGED
            break
    return dict(pose=pose, iters=iters, status=status, trace=trace)
