// drpm.hip — SolveMotionEstimationProblemDRPM (solver.cpp:486-603, degeneracy.h:14-131) on device:
// H = Σ w a aᵀ and g = Σ w a b (pass 1 of the LS chain), a cyclic Jacobi eigendecomposition
// (SelfAdjointEigenSolver order: ascending), the per-point noise mean / variance along the
// eigenvectors, normal-CDF probabilities with SNR factor 10, and x = U·diag(p/λ)·Uᵀ g when
// min p < threshold, else the weighted solve.  One launch sequence (launch_drpm) for RANSAC's final
// solve and for the stand-alone method; launch_drpm_batch runs it for every frame of a batch (grid
// y = frame, the same bodies).
#include <algorithm>

#include "drpm_common.h"

namespace imlsgpu {
namespace {

// The wave's totals of the 42 DRPM terms by recursive halving (internal.h wave_sum28's scheme): terms
// 0..31 in one pass (31 + 1 fp64 exchanges), 32..41 padded to 16 in another (15 + 2) — 49 exchanges
// where 42 butterfly wave_sums issued 252 (round 6).  Lane 2k returns total k in r0 (k < 32) and
// total 32 + k in r1 (k < 10).  A fixed association shared by every DRPM launch (alone and batched).
template <int H, int N>
__device__ __forceinline__ void halve_n(double (&a)[N], int lane) {
    const bool up = (lane & (2 * H)) != 0;
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const double send = up ? a[i] : a[H + i];
        const double keep = up ? a[H + i] : a[i];
        a[i] = keep + xor_f64(send, 2 * H);
    }
    if constexpr (H > 1) halve_n<H / 2, N>(a, lane);
}
__device__ __forceinline__ void wave_sum42(const double (&v)[kDrpmSlab], double& r0, double& r1) {
    const int lane = threadIdx.x & 63;
    double a[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) a[k] = v[k];
    halve_n<16, 32>(a, lane);
    r0 = a[0] + xor_f64(a[0], 1);
    double b[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) b[k] = k < kDrpmSlab - 32 ? v[32 + k] : 0.0;
    halve_n<8, 16>(b, lane);
    r1 = b[0] + xor_f64(b[0], 1);
    r1 = r1 + xor_f64(r1, 32);
}
// lane 2k of wave wv writes its totals to red[wv][·] (the block's per-wave rows)
__device__ __forceinline__ void wave_sum42_store(const double (&v)[kDrpmSlab], double* __restrict__ row) {
    double r0, r1;
    wave_sum42(v, r0, r1);
    const int lane = threadIdx.x & 63;
    if (!(lane & 1)) {
        row[lane >> 1] = r0;
        if ((lane >> 1) < kDrpmSlab - 32) row[32 + (lane >> 1)] = r1;
    }
}

// reduce the weighted normal equations (pass-1 slabs), eigendecompose H
__device__ __forceinline__ void drpm_eig_body(const double* __restrict__ partial, int blocks, const SolveState& st,
                                              const DrpmDev& Dv) {
    if (*st.done) return;
    __shared__ double red[(256 / 64) * kNormEq];
    __shared__ double acc[kNormEq];
    double loc[kNormEq];
#pragma unroll
    for (int k = 0; k < kNormEq; ++k) loc[k] = 0.0;
    for (int b = threadIdx.x; b < blocks; b += 256)
#pragma unroll
        for (int k = 0; k < kNormEq; ++k) loc[k] += partial[(size_t)b * kNormEq + k];
    block_sum28<256>(loc, red, acc);
    if (threadIdx.x >= 64) return;
    drpm_eig_tail(acc, Dv);
}

// the 42 noise terms of row i (zero when i ≥ N or the row is absent), degeneracy.h:14-72
__device__ __forceinline__ void drpm_noise_terms(const Rows& rows, int i, int N, const DrpmDev& Dv, double sp, double sn,
                                                 double (&acc)[kDrpmSlab]) {
#pragma unroll
    for (int k = 0; k < kDrpmSlab; ++k) acc[k] = 0.0;
    double a[6], b, wt;
    if (i < N && rows.get(i, a, b, wt)) {
        const size_t i3 = 3 * (size_t)i;
        const double s[3] = {rows.ds[i3], rows.ds[i3 + 1], rows.ds[i3 + 2]};
        const double n[3] = {rows.dn[i3], rows.dn[i3 + 1], rows.dn[i3 + 2]};
        // skew(v) = [0 −z y; z 0 −x; −y x 0] (degeneracy.h:7-12)
        const double nx[9] = {0, -n[2], n[1], n[2], 0, -n[0], -n[1], n[0], 0};
        const double px[9] = {0, -s[2], s[1], s[2], 0, -s[0], -s[1], s[0], 0};
        double B[36];
#pragma unroll
        for (int q = 0; q < 36; ++q) B[q] = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                B[r * 6 + c] = -nx[r * 3 + c];
                double pn = 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) pn += px[r * 3 + k] * nx[k * 3 + c];
                B[r * 6 + 3 + c] = pn;
                B[(3 + r) * 6 + 3 + c] = nx[r * 3 + c];
            }
        const double sp2 = sp * sp, sn2 = sn * sn;
        const double Nd[6] = {sp2, sp2, sp2, sn2, sn2, sn2};
        double C[36];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                double v = 0;
#pragma unroll
                for (int k = 0; k < 6; ++k) v += B[r * 6 + k] * Nd[k] * B[c * 6 + k];
                C[r * 6 + c] = v * wt;
            }
#pragma unroll
        for (int q = 0; q < 36; ++q) acc[q] = C[q];
        const double sw = sqrt(wt);
        double v6[6];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            double pn = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) pn += px[r * 3 + k] * n[k];
            v6[r] = sw * pn;
            v6[3 + r] = sw * n[r];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            double aa = 0, bb = 0;
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                double cu = 0;
#pragma unroll
                for (int c = 0; c < 6; ++c) cu += C[r * 6 + c] * Dv.U[k * 6 + c];
                aa += Dv.U[k * 6 + r] * cu;
                bb += Dv.U[k * 6 + r] * v6[r];
            }
            acc[36 + k] = 2 * aa * aa + 4 * aa * bb * bb;
        }
    }
}

// per-point noise mean (36) and variance along the eigenvectors (6), degeneracy.h:14-72
__device__ __forceinline__ void drpm_noise_body(const Rows& rows, int N, const SolveState& st, const DrpmDev& Dv, double sp,
                                                double sn) {
    if (*st.done) return;
    __shared__ double red[(kBlock / 64) * kDrpmSlab];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    double acc[kDrpmSlab];
    drpm_noise_terms(rows, i, N, Dv, sp, sn, acc);
    const int wv = threadIdx.x >> 6;
    wave_sum42_store(acc, red + wv * kDrpmSlab);
    __syncthreads();
    if (threadIdx.x < kDrpmSlab) {
        double s = 0.0;
        for (int w = 0; w < kBlock / 64; ++w) s += red[w * kDrpmSlab + threadIdx.x];
        Dv.slabs[(size_t)blockIdx.x * kDrpmSlab + threadIdx.x] = s;
    }
}

__device__ __forceinline__ double normal_cdf(double mean, double sd, double x) {
    return 0.5 * erfc(-(x - mean) / (sd * sqrt(2.0)));   // Boost.Math cdf(normal(mean, sd), x)
}

// The DRPM decision and solve from the reduced noise terms tot[42] (solver.cpp:540-603), by wave 0
// (every other thread returns): lane k < 6 evaluates prob[k] — the thread-0 loop's expressions for
// that k, so the same bits — the minimum over k in order, then either the SNR-weighted
// eigen-solution (thread 0) or the plain normal-equation solve by the whole wave (solve6_u: solve6's
// operations with a wave-uniform pivot, bit for bit), Δ and the pose update by thread 0.  Round 6:
// one thread ran all six probabilities and solve6's predicated pivot swaps (k_drpm_final 27 µs per
// call on a lone 1600-row frame, profiles/r06_calib).
__device__ __forceinline__ void drpm_solve_wave0(const SolveState& st, const DrpmDev& Dv, imls_iter_trace* tr,
                                                 const KParams& kp, double threshold, const int* __restrict__ count_all,
                                                 const int* __restrict__ count_in, int update_pose, const double* tot) {
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    const double snr = 10.0;   // solver.cpp:547
    double pk = 0.0;
    if (lane < 6) {
        const int k = lane;
        double meas = 0, exp_noise = 0;
        for (int r = 0; r < 6; ++r) {
            double hu = 0, mu = 0;
            for (int c = 0; c < 6; ++c) { hu += Dv.H[r * 6 + c] * Dv.U[k * 6 + c]; mu += tot[r * 6 + c] * Dv.U[k * 6 + c]; }
            meas += Dv.U[k * 6 + r] * hu;
            exp_noise += Dv.U[k * 6 + r] * mu;
        }
        const double sd = sqrt(tot[36 + k]);
        const double tp = meas / (1.0 + snr);
        const bool bad = isnan(exp_noise) || isnan(sd) || isnan(tp);
        pk = bad ? 0.0 : normal_cdf(exp_noise, sd, tp);
    }
    double prob[6], pmin = INFINITY;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        prob[k] = readlane_f64(pk, k);
        pmin = fmin(pmin, prob[k]);
    }
    double x[6];
    if (pmin < threshold) {
        if (lane) return;
        double ut[6];
        for (int k = 0; k < 6; ++k) {
            const double dps = fabs(Dv.ev[k]) > 1e-10 ? prob[k] / Dv.ev[k] : 0.0;
            double acc = 0;
            for (int r = 0; r < 6; ++r) acc += Dv.U[k * 6 + r] * Dv.g[r];
            ut[k] = dps * acc;
        }
        for (int r = 0; r < 6; ++r) {
            double acc = 0;
            for (int k = 0; k < 6; ++k) acc += Dv.U[k * 6 + r] * ut[k];
            x[r] = acc;
        }
    } else {
        double ne[kNormEq];
        int k = 0;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) ne[k++] = Dv.H[r * 6 + c];
        for (int r = 0; r < 6; ++r) ne[21 + r] = Dv.g[r];
        ne[27] = 0;
        solve6_u(ne, x);
        if (lane) return;
    }
    double D[16];
    delta_from_x(x, D);
    finish_iteration(st, tr, D, (double)*count_all, (double)*count_in, update_pose, kp);
    if (st.info) {
        for (int k = 0; k < 6; ++k) st.info->prob[k] = prob[k];
        st.info->degenerate = pmin < threshold ? 1 : 0;
        info_export(st.info, kInfoDrpm, x, st, update_pose);
    }
}

__device__ __forceinline__ void drpm_final_body(int blocks, const SolveState& st, const DrpmDev& Dv, imls_iter_trace* tr,
                                                const KParams& kp, double threshold, const int* __restrict__ count_all,
                                                const int* __restrict__ count_in, int update_pose) {
    if (*st.done) return;
    __shared__ double red[(256 / 64) * kDrpmSlab];
    __shared__ double tot[kDrpmSlab];
    double loc[kDrpmSlab];
#pragma unroll
    for (int k = 0; k < kDrpmSlab; ++k) loc[k] = 0.0;
    for (int b = threadIdx.x; b < blocks; b += 256)
#pragma unroll
        for (int k = 0; k < kDrpmSlab; ++k) loc[k] += Dv.slabs[(size_t)b * kDrpmSlab + k];
    const int wv = threadIdx.x >> 6;
    wave_sum42_store(loc, red + wv * kDrpmSlab);
    __syncthreads();
    if (threadIdx.x < kDrpmSlab) {
        double s = 0.0;
        for (int w = 0; w < 256 / 64; ++w) s += red[w * kDrpmSlab + threadIdx.x];
        tot[threadIdx.x] = s;
    }
    __syncthreads();
    drpm_solve_wave0(st, Dv, tr, kp, threshold, count_all, count_in, update_pose, tot);
}

__global__ __launch_bounds__(256) void k_drpm_eig(const double* __restrict__ partial, int blocks, SolveState st, DrpmDev Dv) {
    drpm_eig_body(partial, blocks, st, Dv);
}
__global__ __launch_bounds__(kBlock) void k_drpm_noise(Rows rows, int N, SolveState st, DrpmDev Dv, double sp, double sn) {
    drpm_noise_body(rows, N, st, Dv, sp, sn);
}
__global__ __launch_bounds__(256) void k_drpm_final(int blocks, SolveState st, DrpmDev Dv, imls_iter_trace* tr, KParams kp,
                                                    double threshold, const int* __restrict__ count_all,
                                                    const int* __restrict__ count_in, int update_pose, RansacDev R,
                                                    imls_iter_trace* rtr) {
    drpm_final_body(blocks, st, Dv, tr, kp, threshold, count_all, count_in, update_pose);
    ransac_trace_t0(R, count_all, rtr);
}

// batched: frame = tab[blockIdx.y], its RANSAC scratch A.rf, its pose update always on
__global__ __launch_bounds__(256) void k_drpm_eig_b(const PairDev* __restrict__ tab) {
    const PairDev A = device_view(tab + blockIdx.y);
    drpm_eig_body(A.st.partial1, solve_blocks(A.rf.cap), A.st, A.rf.Dv);
}
__global__ __launch_bounds__(kBlock) void k_drpm_noise_b(const PairDev* __restrict__ tab, double sp, double sn) {
    const PairDev A = device_view(tab + blockIdx.y);
    if ((int)blockIdx.x >= solve_blocks(A.rf.cap)) return;
    drpm_noise_body(frame_rows(A, 1, 1), A.rf.cap, A.st, A.rf.Dv, sp, sn);
}
__global__ __launch_bounds__(256) void k_drpm_final_b(const PairDev* __restrict__ tab, KParams kp, double threshold, int it) {
    const PairDev A = device_view(tab + blockIdx.y);
    drpm_final_body(solve_blocks(A.rf.cap), A.st, A.rf.Dv, A.trace + it, kp, threshold, A.rf.cnt_all, A.rf.cnt_in, 1);
    ransac_trace_t0(A.rf.R, A.rf.cnt_all, A.trace + it);
}

// stand-alone DRPM with no rows fails like the oracle's solve_drpm (N == 0 → false)
__global__ void k_drpm_guard(const int* __restrict__ c, SolveState st) {
    if (threadIdx.x == 0 && *c == 0) { *st.status = IMLS_FRAME_SOLVE_FAILED; *st.done = 1; }
}

__global__ void k_set_count(int* __restrict__ c, int v) {
    if (threadIdx.x == 0) *c = v;
}

}  // namespace

void launch_set_count(hipStream_t s, int* count, int v) { k_set_count<<<1, 64, 0, s>>>(count, v); }

void launch_drpm(hipStream_t s, const Rows& rows, int cap, const SolveState& st, const DrpmDev& Dv, imls_iter_trace* tr,
                 const KParams& kp, const RansacParams& rp, const int* cnt_all, const int* cnt_in, int update_pose,
                 const RansacDev& R, imls_iter_trace* rtr, bool head_done) {
    const int b1 = solve_blocks(cap);
    if (!head_done) {
        launch_rows_pass1(s, rows, cap, st.partial1, b1);
        k_drpm_eig<<<1, 256, 0, s>>>(st.partial1, b1, st, Dv);
    }
    k_drpm_noise<<<b1, kBlock, 0, s>>>(rows, cap, st, Dv, rp.drpm_stdev_points, rp.drpm_stdev_normals);
    k_drpm_final<<<1, 256, 0, s>>>(b1, st, Dv, tr, kp, rp.drpm_threshold, cnt_all, cnt_in, update_pose, R, rtr);
}

void launch_drpm_batch(hipStream_t s, const PairDev* tab, const int* cap_host, int npairs, int maxc, const KParams& kp,
                       const RansacParams& rp, int it) {
    const dim3 g1(1, npairs);
    launch_rows_pass1_batch(s, tab, cap_host, npairs, 1);
    k_drpm_eig_b<<<g1, 256, 0, s>>>(tab);
    k_drpm_noise_b<<<dim3(solve_blocks(maxc), npairs), kBlock, 0, s>>>(tab, rp.drpm_stdev_points, rp.drpm_stdev_normals);
    k_drpm_final_b<<<g1, 256, 0, s>>>(tab, kp, rp.drpm_threshold, it);   // + RANSAC's trace record
}

// stand-alone SolveMotionEstimationProblemDRPM (solver.cpp:499-603) on host fp64 rows + weights
void launch_drpm_alone(hipStream_t s, const SolveLaunch& L) {
    const int cap = std::max(L.N, 1);
    char* p = (char*)L.scratch;
    int* cnt = carve<int>(p, 1);
    const DrpmDev Dv = drpm_carve(p, solve_blocks(cap));
    launch_set_count(s, cnt, L.N);
    k_drpm_guard<<<1, 64, 0, s>>>(cnt, L.st);
    const size_t c = (size_t)L.N;
    const Rows rows{nullptr, nullptr, nullptr, L.rows_d, L.rows_d + 3 * c, L.rows_d + 6 * c, L.weights, 1, cnt, nullptr};
    launch_drpm(s, rows, cap, L.st, Dv, L.tr, L.kp, L.ransac, cnt, cnt, L.update_pose, RansacDev{}, nullptr, false);
}

}  // namespace imlsgpu
