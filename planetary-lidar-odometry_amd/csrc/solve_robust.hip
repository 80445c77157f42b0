// solve_robust.hip — the robust M-estimator solve (IMLS_SOLVE_ROBUST, include/imls_gpu.h): the
// point-to-plane rows of the LS solve (solver.cpp:89-107), re-weighted K times by their residual
// under ψ ∈ {Huber, Cauchy, Geman-McClure}.  With x⁰ = 0, for k = 0 … K−1:
//     r = a·xᵏ − b,  w = u·ψ(r; c),  H = Σ w a aᵀ,  g = Σ w a b,  xᵏ⁺¹ = solve6_u(H, g)
// (LS's column-pivoted solve and rank rule; with fewer than 6 valid rows the rank is capped at their count)
// then Δ = delta_from_x(x^K) and finish_iteration, as LS.  The cost is the reference's Ceres problem
// (HuberLoss(0.1), solver.cpp:25-72) linearised at the ICP iteration's pose.
//
// Two forms, chosen by the rows alone (so a frame takes the same one alone and in a batch):
//   float rows of ≤ kSmallRows   k_robust_small: one block; each thread keeps its ≤ kSmallPer rows in
//                                registers across the K passes; per pass the weights, block_sum28,
//                                solve6_u in wave 0, x through LDS.  One launch per solve.
//   larger frames, fp64 rows     K × (k_robust_pass: one row per thread, one slab of 28 sums per
//                                block into partial1; k_robust_step: one block reduces the slabs in
//                                order and solves, writes xᵏ⁺¹ to st.x0 where the next pass reads it;
//                                the last one does Δ and the pose update).  2K launches.
// Grid shapes and the order of every sum depend on N only.  Every kernel returns at once when the
// frame's `done` flag is set; ordinary vector stores, no floating-point atomics.
#include "solve.h"
#include "solve_common.h"

namespace imlsgpu {
namespace {

// one row's weighted terms added to the 28 running sums: w·a·aᵀ (21), w·a·b (6), the row count
__device__ __forceinline__ void robust_add(double (&loc)[kNormEq], const double (&a)[6], double b, double w) {
    double wa[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) wa[p] = w * a[p];
    int q = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int c = p; c < 6; ++c) loc[q++] += wa[p] * a[c];
#pragma unroll
    for (int p = 0; p < 6; ++p) loc[21 + p] += wa[p] * b;
    loc[27] += 1.0;
}
// r = a·x − b in the solvers' order of operations (resid_hist_core)
__device__ __forceinline__ double robust_resid(const double (&a)[6], double b, const double* x) {
    double v = a[0] * x[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) v = v + a[k] * x[k];
    return v - b;
}

// H is a sum of one dyad per row of weight > 0: its rank cannot exceed their count (what QR on the
// √w-scaled rows has by construction).  Float rows have u = 1 and ψ > 0: every valid row counts.
__device__ __forceinline__ int robust_max_rank(double npos) { return npos < 6.0 ? (int)npos : 6; }

// The gates of LS on the valid-row count (block-uniform): true when the frame stops here.
__device__ __forceinline__ bool robust_gate(const SolveState& st, imls_iter_trace* tr, const KParams& kp, double nvalid,
                                            int update_pose) {
    if (update_pose && nvalid < (double)kp.correspond_number) {   // laser_odometry.cpp:570-576
        if (threadIdx.x == 0) {
            *st.status = IMLS_FRAME_TOO_FEW;
            *st.done = 1;
            if (tr) tr->n_valid = (unsigned long long)nvalid;
        }
        return true;
    }
    if (nvalid == 0.0) {                  // no valid row: the solve fails, as LS
        if (threadIdx.x == 0) { *st.status = IMLS_FRAME_SOLVE_FAILED; *st.done = 1; }
        return true;
    }
    return false;
}
// thread 0, after the last step: Δ, pose update, trace, convergence, the pose-info export
__device__ __forceinline__ void robust_finish(const SolveState& st, imls_iter_trace* tr, const KParams& kp, const double* xprev,
                                              const double x[6], double nvalid, int update_pose) {
    double D[16];
    delta_from_x(x, D);
    finish_iteration(st, tr, D, nvalid, nvalid, update_pose, kp);
    if (st.info) {
        for (int k = 0; k < 6; ++k) st.info->x0[k] = xprev[k];
        info_export(st.info, kInfoRobust, x, st, update_pose);
    }
}

// ---------------------------------------------------------------------------------------------
// small float frames: one block (the analogue of k_solve_small, solve.hip, whose row loads these are)
constexpr int kSmallBlock = 512;
constexpr int kSmallPer = kSmallRows / kSmallBlock;
static_assert(kSmallRows % kSmallBlock == 0 && kSmallPer % 2 == 0, "rows per thread, in two groups");

__device__ __forceinline__ void row_a(const float4& s4, const float4& n4, double a[6]) {
    const double s[3] = {s4.x, s4.y, s4.z}, n[3] = {n4.x, n4.y, n4.z};
    a[0] = n[2] * s[1] - n[1] * s[2];
    a[1] = n[0] * s[2] - n[2] * s[0];
    a[2] = n[1] * s[0] - n[0] * s[1];
    a[3] = n[0]; a[4] = n[1]; a[5] = n[2];
}
__device__ __forceinline__ double row_b(const float4& s4, const float4& d4, const float4& n4) {
    const double s[3] = {s4.x, s4.y, s4.z}, d[3] = {d4.x, d4.y, d4.z}, n[3] = {n4.x, n4.y, n4.z};
    double b = n[0] * (d[0] - s[0]);
    b = b + n[1] * (d[1] - s[1]);
    b = b + n[2] * (d[2] - s[2]);
    return b;
}

__device__ __forceinline__ void robust_small_body(const Rows& rows, int N, const SolveState& st, imls_iter_trace* tr,
                                                  const KParams& kp, int update_pose) {
    const int stopped = *st.done;         // read with the rows, not ahead of them (k_solve_small)
    __shared__ double red[(kSmallBlock / 64) * kNormEq];
    __shared__ double acc[kNormEq];
    __shared__ double xs[2][6];           // xᵏ (the pass reads it) and xᵏ⁺¹, alternating
    const int t = threadIdx.x;
    // this thread's rows t + k·512: s (w = valid flag), n and b stay in registers for every pass; loaded
    // in two groups from a clamped index, the second ordered behind the first (see solve_small_body)
    float4 rs[kSmallPer], rn[kSmallPer];
    double rb[kSmallPer];
    const int rmax = N > 0 ? N - 1 : 0;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    constexpr int kGrp = kSmallPer / 2;
    int tg = t;
    auto load_group = [&](int k0) {
        float4 c[kGrp], d[kGrp], n[kGrp];
#pragma unroll
        for (int u = 0; u < kGrp; ++u) {
            const int rr = min(tg + (k0 + u) * kSmallBlock, rmax);
            c[u] = rows.cs[rr];
            d[u] = rows.cd[rr];
            n[u] = rows.cn[rr];
        }
#pragma unroll
        for (int u = 0; u < kGrp; ++u) {
            const int k = k0 + u;
            const int r = t + k * kSmallBlock;
            rs[k] = r < N ? c[u] : z4;
            const bool v = r < N && rs[k].w != 0.f;
            rn[k] = v ? n[u] : z4;
            rb[k] = row_b(rs[k], v ? d[u] : z4, rn[k]);
        }
    };
    load_group(0);
    if (N > kGrp * kSmallBlock) {
        asm volatile("" : "+v"(tg) : "v"(rb[0]), "v"(rb[kGrp - 1]));
        load_group(kGrp);
    } else {
#pragma unroll
        for (int k = kGrp; k < kSmallPer; ++k) { rs[k] = z4; rn[k] = z4; rb[k] = 0.0; }
    }
    if (stopped) return;                  // block-uniform, before any LDS write or barrier
    if (t < 6) xs[0][t] = 0.0;
    __syncthreads();
    const int K = kp.robust_iters, loss = kp.robust_loss;
    const double c = kp.robust_scale;
    double nvalid = 0.0;
    for (int it = 0; it < K; ++it) {
        const double* x = xs[it & 1];
        double loc[kNormEq];
#pragma unroll
        for (int k = 0; k < kNormEq; ++k) loc[k] = 0.0;
#pragma unroll
        for (int k = 0; k < kSmallPer; ++k) {
            if (t + k * kSmallBlock < N && rs[k].w != 0.f) {
                double a[6];
                row_a(rs[k], rn[k], a);
                robust_add(loc, a, rb[k], robust_psi(loss, c, robust_resid(a, rb[k], x)));
            }
        }
        block_sum28<kSmallBlock>(loc, red, acc);
        nvalid = acc[27];
        if (it == 0 && robust_gate(st, tr, kp, nvalid, update_pose)) return;
        if (t < 64) {                     // wave 0: the 6×6 solve by its 64 lanes
            double xn[6];
            solve6_u(acc, xn, robust_max_rank(nvalid));
            if (t == 0)
                for (int k = 0; k < 6; ++k) xs[(it + 1) & 1][k] = xn[k];
        }
        __syncthreads();
    }
    if (t != 0) return;
    double x[6];
    for (int k = 0; k < 6; ++k) x[k] = xs[K & 1][k];
    robust_finish(st, tr, kp, xs[(K - 1) & 1], x, nvalid, update_pose);
}

// ---------------------------------------------------------------------------------------------
// the grid chain: pass `it` (one slab per block) and step `it` (one block)
__device__ __forceinline__ void robust_pass_body(const Rows& rows, int N, const SolveState& st, const KParams& kp, int it) {
    if (*st.done) return;
    __shared__ double red[(kBlock / 64) * kNormEq];
    __shared__ double out[kNormEq];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    double x[6] = {0, 0, 0, 0, 0, 0};
    if (it > 0)
        for (int k = 0; k < 6; ++k) x[k] = st.x0[k];
    double loc[kNormEq];
#pragma unroll
    for (int k = 0; k < kNormEq; ++k) loc[k] = 0.0;
    double a[6], b, wt;
    bool pos = false;
    if (i < N && rows.get(i, a, b, wt)) {
        const double w = wt * robust_psi(kp.robust_loss, kp.robust_scale, robust_resid(a, b, x));
        robust_add(loc, a, b, w);
        pos = w > 0.0;
    }
    // the block's rows of weight > 0 (caller weights may be 0), one word per block in partial2: the rank cap
    __shared__ int wpos[kBlock / 64];
    const int npos = __popcll(__ballot(pos));
    if ((threadIdx.x & 63) == 0) wpos[threadIdx.x >> 6] = npos;
    block_sum28<kBlock>(loc, red, out);
    if (threadIdx.x < kNormEq) st.partial1[(size_t)blockIdx.x * kNormEq + threadIdx.x] = out[threadIdx.x];
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kBlock / 64; ++w) s += wpos[w];
        st.partial2[blockIdx.x] = (double)s;
    }
}

constexpr int kStepBlock = 256;
__device__ __forceinline__ void robust_step_body(int blocks, const SolveState& st, imls_iter_trace* tr, const KParams& kp, int it,
                                                 int update_pose) {
    if (*st.done) return;
    __shared__ double red[(kStepBlock / 64) * kNormEq];
    __shared__ double acc[kNormEq];
    const int t = threadIdx.x;
    double loc[kNormEq];
#pragma unroll
    for (int k = 0; k < kNormEq; ++k) loc[k] = 0.0;
    double cnt = 0.0;                     // rows of weight > 0 (small integers: exact in any order)
    for (int b = t; b < blocks; b += kStepBlock) {
#pragma unroll
        for (int k = 0; k < kNormEq; ++k) loc[k] += st.partial1[(size_t)b * kNormEq + k];
        cnt += st.partial2[b];
    }
    __shared__ double wcnt[kStepBlock / 64];
    cnt = wave_sum(cnt);
    if ((t & 63) == 0) wcnt[t >> 6] = cnt;
    block_sum28<kStepBlock>(loc, red, acc);
    const double nvalid = acc[27];
    if (it == 0 && robust_gate(st, tr, kp, nvalid, update_pose)) return;
    if (t >= 64) return;
    double npos = 0.0;
    for (int w = 0; w < kStepBlock / 64; ++w) npos += wcnt[w];
    double x[6];
    solve6_u(acc, x, robust_max_rank(npos));   // wave 0
    if (t != 0) return;
    if (it + 1 < kp.robust_iters) {
        for (int k = 0; k < 6; ++k) st.x0[k] = x[k];
        return;
    }
    double xprev[6] = {0, 0, 0, 0, 0, 0};
    if (it > 0)
        for (int k = 0; k < 6; ++k) xprev[k] = st.x0[k];
    robust_finish(st, tr, kp, xprev, x, nvalid, update_pose);
}

// ---------------------------------------------------------------------------------------------
// Kernels: one frame (arguments by value) and batched (frame = tab[blockIdx.y]); the same bodies.
__global__ __launch_bounds__(kSmallBlock) void k_robust_small(Rows rows, int N, SolveState st, imls_iter_trace* tr, KParams kp,
                                                             int update_pose) {
    robust_small_body(rows, N, st, tr, kp, update_pose);
}
__global__ __launch_bounds__(kBlock) void k_robust_pass(Rows rows, int N, SolveState st, KParams kp, int it) {
    robust_pass_body(rows, N, st, kp, it);
}
__global__ __launch_bounds__(kStepBlock) void k_robust_step(int blocks, SolveState st, imls_iter_trace* tr, KParams kp, int it,
                                                            int update_pose) {
    robust_step_body(blocks, st, tr, kp, it, update_pose);
}
__global__ __launch_bounds__(kSmallBlock) void k_robust_small_b(const PairDev* __restrict__ tab, KParams kp, int iter) {
    const PairDev A = device_view(tab + blockIdx.y);
    if (A.N > kSmallRows) return;
    robust_small_body(frame_rows(A, 0, 0), A.N, A.st, A.trace + iter, kp, 1);
}
__global__ __launch_bounds__(kBlock) void k_robust_pass_b(const PairDev* __restrict__ tab, KParams kp, int it) {
    const PairDev A = device_view(tab + blockIdx.y);
    if (A.N <= kSmallRows || (int)blockIdx.x >= solve_blocks(A.N)) return;
    robust_pass_body(frame_rows(A, 0, 0), A.N, A.st, kp, it);
}
__global__ __launch_bounds__(kStepBlock) void k_robust_step_b(const PairDev* __restrict__ tab, KParams kp, int it, int iter) {
    const PairDev A = device_view(tab + blockIdx.y);
    if (A.N <= kSmallRows) return;
    robust_step_body(solve_blocks(A.N), A.st, A.trace + iter, kp, it, 1);
}

}  // namespace

void launch_solve_robust(hipStream_t s, const SolveLaunch& L) {
    const int N = L.N;
    const size_t c = (size_t)N;
    Rows rows{L.cs, L.cd, L.cn, nullptr, nullptr, nullptr, L.weights, L.rows_are_double, L.count, nullptr};
    if (L.rows_are_double) {
        rows.ds = L.rows_d;
        rows.dd = L.rows_d + 3 * c;
        rows.dn = L.rows_d + 6 * c;
    } else if (N <= kSmallRows) {
        k_robust_small<<<1, kSmallBlock, 0, s>>>(rows, N, L.st, L.tr, L.kp, L.update_pose);
        return;
    }
    const int nb = std::max(solve_blocks(N), 1);
    for (int it = 0; it < L.kp.robust_iters; ++it) {
        k_robust_pass<<<nb, kBlock, 0, s>>>(rows, N, L.st, L.kp, it);
        k_robust_step<<<1, kStepBlock, 0, s>>>(nb, L.st, L.tr, L.kp, it, L.update_pose);
    }
}

void launch_solve_robust_batch(hipStream_t s, const PairDev* tab, const int* n_host, int npairs, const KParams& kp, int it) {
    if (npairs <= 0) return;
    int maxN = 0;
    bool any_small = false, any_large = false;
    for (int k = 0; k < npairs; ++k) {
        maxN = std::max(maxN, n_host[k]);
        (n_host[k] <= kSmallRows ? any_small : any_large) = true;
    }
    if (any_small) k_robust_small_b<<<dim3(1, npairs), kSmallBlock, 0, s>>>(tab, kp, it);
    if (!any_large) return;
    for (int k = 0; k < kp.robust_iters; ++k) {
        k_robust_pass_b<<<dim3(solve_blocks(maxN), npairs), kBlock, 0, s>>>(tab, kp, k);
        k_robust_step_b<<<dim3(1, npairs), kStepBlock, 0, s>>>(tab, kp, k, it);
    }
}

}  // namespace imlsgpu
