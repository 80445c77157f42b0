// pose_info.hip — the covariance / degeneracy report of the last solve (imls_capture_pose_info;
// include/imls_gpu.h defines every field).  Two launches behind a solve sequence:
//
//   k_info_rows   one lane per row, read through Rows (the projection's float rows and the fp64 rows of
//                 the host API / the RANSAC inliers share the code).  Membership in the solve's final
//                 system comes from the solve's own export (internal.h InfoExport): every valid row, or —
//                 a trimmed LS — the rows of the closed interval [(key_lo, row_lo), (key_hi, row_hi)]
//                 of the total order (|r₁| bits, row); or — a robust solve — every valid row with the
//                 weights of its last 6×6 system, u·ψ(a·x0 − b) under the exported x0 = x^{K−1}
//                 (robust_psi and the residual expression of solve_robust.hip).  The key is recomputed with the expression the
//                 solver uses (resid_hist_core / solve_small_body; -ffp-contract=off: the same bits).
//                 Per kept row, in fp64: 21 terms of w·a·aᵀ, 6 of w·a·b, w·b², w, 1 and w·(a·x − b)²
//                 (x is exported before the pass starts, so the residual needs no launch of its own).
//                 Reduced wave → block → slab in a fixed order (wave_sum28's halving, then the block's
//                 four waves in order); no floating-point atomics, so a frame's report has the same
//                 bits alone and in a batch.
//   k_info_final  one block: the slabs summed in order (thread t takes slabs t, t + 256, …), H
//                 mirrored, the DRPM head's Jacobi (sym_eig6_wave, solve_common.h: the same
//                 operations and stop rule), the sign rule, rank, σ², the pseudo-inverse covariance.
#include "solve.h"
#include "solve_common.h"

namespace imlsgpu {
namespace {

constexpr int kTermBtb = 27, kTermW = 28, kTermRows = 29, kTermRss = 30;
static_assert(kInfoTerms == 32 && kTermRss < kInfoTerms, "wave_sum28 reduces 32 values per lane");

__device__ __forceinline__ bool info_pair_le(unsigned long long ka, unsigned ra, unsigned long long kb, unsigned rb) {
    return ka < kb || (ka == kb && ra <= rb);
}

// Block sum of kInfoTerms values per thread: lane 2k of each wave holds value k's wave total
// (wave_sum28 reduces all 32 slots), the waves are added in order.  out: [kInfoTerms], global or LDS.
template <int NT>
__device__ __forceinline__ void info_block_sum(double (&v)[kInfoTerms], double* red, double* out) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double s = wave_sum28(v);
    if (!(lane & 1)) red[wv * kInfoTerms + (lane >> 1)] = s;
    __syncthreads();
    if (threadIdx.x < kInfoTerms) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) t += red[w * kInfoTerms + threadIdx.x];
        out[threadIdx.x] = t;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kBlock) void k_info_rows(Rows rows, int N, const InfoExport* __restrict__ ex,
                                                       double* __restrict__ slabs, int robust_loss, double robust_scale) {
    __shared__ double red[(kBlock / 64) * kInfoTerms];
    const int kind = ex->kind;
    if (kind == kInfoNone) return;        // no solve succeeded: k_info_final reports zeros
    const int i = blockIdx.x * kBlock + threadIdx.x;
    double v[kInfoTerms];
#pragma unroll
    for (int k = 0; k < kInfoTerms; ++k) v[k] = 0.0;
    double a[6], b, wt;
    if (i < N && rows.get(i, a, b, wt)) {
        bool in = true;
        if (kind == kInfoTrim) {
            wt = 1.0;                     // the trimmed second solve is unweighted (solver.cpp:124-136)
            double r1 = a[0] * ex->x0[0];
            for (int k = 1; k < 6; ++k) r1 = r1 + a[k] * ex->x0[k];
            const unsigned long long kb = (unsigned long long)__double_as_longlong(fabs(r1 - b));
            in = info_pair_le(ex->key_lo, ex->row_lo, kb, (unsigned)i) && info_pair_le(kb, (unsigned)i, ex->key_hi, ex->row_hi);
        }
        if (kind == kInfoRobust) {
            double r0 = a[0] * ex->x0[0];
            for (int k = 1; k < 6; ++k) r0 = r0 + a[k] * ex->x0[k];
            wt = wt * robust_psi(robust_loss, robust_scale, r0 - b);
        }
        if (in) {
            double wa[6];
#pragma unroll
            for (int r = 0; r < 6; ++r) wa[r] = wt * a[r];
            int q = 0;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = r; c < 6; ++c) v[q++] = wa[r] * a[c];
#pragma unroll
            for (int r = 0; r < 6; ++r) v[21 + r] = wa[r] * b;
            v[kTermBtb] = (wt * b) * b;
            v[kTermW] = wt;
            v[kTermRows] = 1.0;
            double ax = a[0] * ex->x[0];
            for (int k = 1; k < 6; ++k) ax = ax + a[k] * ex->x[k];
            const double res = ax - b;
            v[kTermRss] = (wt * res) * res;
        }
    }
    info_block_sum<kBlock>(v, red, slabs + (size_t)blockIdx.x * kInfoTerms);
}

struct InfoFinalArgs {
    const InfoExport* ex;
    const int *status, *iters;
    int in_loop, solve_method, final_method;
    const double* slabs;
    int blocks;
    struct imls_pose_info* out;
};

__global__ __launch_bounds__(256) void k_info_final(InfoFinalArgs A) {
    __shared__ double red[(256 / 64) * kInfoTerms];
    __shared__ double tot[kInfoTerms];
    __shared__ double ev[6], U[36], H[36], cov[36];
    __shared__ double sigma2;
    __shared__ int meta[2];               // rank, flags
    const int t = threadIdx.x;
    double* o = reinterpret_cast<double*>(A.out);
    constexpr int kWords = (int)(sizeof(struct imls_pose_info) / 8);
    static_assert(sizeof(struct imls_pose_info) % 8 == 0, "report is copied as 8-byte words");
    const int kind = A.ex->kind;
    const int status = *A.status;
    bool valid = kind != kInfoNone;
    if (A.in_loop)      // the rows on the device are those of the frame's last iteration, and it succeeded
        valid = valid && (status == IMLS_FRAME_MAX_ITERS || status == IMLS_FRAME_CONVERGED) && A.ex->iteration == *A.iters - 1;
    else
        valid = valid && status != IMLS_FRAME_SOLVE_FAILED && status != IMLS_FRAME_TOO_FEW;
    if (!valid) {       // block-uniform
        for (int k = t; k < kWords; k += 256) o[k] = 0.0;
        return;
    }
    double loc[kInfoTerms];
#pragma unroll
    for (int k = 0; k < kInfoTerms; ++k) loc[k] = 0.0;
    for (int b = t; b < A.blocks; b += 256)
#pragma unroll
        for (int k = 0; k < kInfoTerms; ++k) loc[k] += A.slabs[(size_t)b * kInfoTerms + k];
    info_block_sum<256>(loc, red, tot);
    if (t < 36) {
        const int r = t / 6, c = t % 6, lo = r < c ? r : c, hi = r < c ? c : r;
        H[t] = tot[lo * 6 - lo * (lo - 1) / 2 + (hi - lo)];   // upper-triangle slot of (lo, hi)
    }
    __syncthreads();
    if (t < 64) {       // wave 0: lane k < 6 holds row k
        double row[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) row[c] = t < 6 ? H[t * 6 + c] : 0.0;
        sym_eig6_wave(row, ev, U);
    }
    __syncthreads();
    if (t < 6) {        // sign: the largest-magnitude component positive, the first one on a tie
        int best = 0;
        double m = fabs(U[t * 6]);
        for (int r = 1; r < 6; ++r)
            if (fabs(U[t * 6 + r]) > m) { m = fabs(U[t * 6 + r]); best = r; }
        if (U[t * 6 + best] < 0)
            for (int r = 0; r < 6; ++r) U[t * 6 + r] = -U[t * 6 + r];
    }
    __syncthreads();
    if (t == 0) {
        int rank = 0;
        for (int k = 0; k < 6; ++k) rank += ev[k] > IMLS_INFO_RANK_RELTOL * ev[5] ? 1 : 0;
        const double n = tot[kTermRows];
        unsigned flags = IMLS_INFO_VALID;
        if (rank < 6) flags |= IMLS_INFO_RANK_DEFICIENT;
        double s2 = 0.0;
        if (n <= (double)rank) flags |= IMLS_INFO_NO_DOF;
        else s2 = tot[kTermRss] / (n - (double)rank);
        if (kind == kInfoDrpm) {
            flags |= IMLS_INFO_DRPM_RAN;
            if (A.ex->degenerate) flags |= IMLS_INFO_DRPM_DEGENERATE;
        }
        sigma2 = s2;
        meta[0] = rank;
        meta[1] = (int)flags;
    }
    __syncthreads();
    if (t < 36) {
        const int r = t / 6, c = t % 6;
        double s = 0.0;
        if (!(meta[1] & IMLS_INFO_NO_DOF))
            for (int k = 0; k < 6; ++k)
                if (ev[k] > IMLS_INFO_RANK_RELTOL * ev[5]) s += U[k * 6 + r] * U[k * 6 + c] / ev[k];
        cov[t] = sigma2 * s;
    }
    __syncthreads();
    struct imls_pose_info* out = A.out;
    if (t < 36) {
        out->hessian[t] = H[t];
        out->eigenvectors[t] = U[t];
        out->covariance[t] = cov[t];
    }
    if (t < 6) {
        out->gradient[t] = tot[21 + t];
        out->x[t] = A.ex->x[t];
        out->eigenvalues[t] = ev[t];
        out->drpm_probability[t] = kind == kInfoDrpm ? A.ex->prob[t] : 0.0;
    }
    if (t == 0) {
        out->btb = tot[kTermBtb];
        out->rss = tot[kTermRss];
        out->weight_sum = tot[kTermW];
        out->n_rows = (unsigned long long)tot[kTermRows];
        out->sigma2 = sigma2;
        out->rank = meta[0];
        out->iteration = A.ex->iteration;
        out->status = status;
        out->solve_method = A.solve_method;
        out->final_method = A.final_method;
        out->flags = (unsigned)meta[1];
        out->_reserved[0] = 0;
        out->_reserved[1] = 0;
    }
}

}  // namespace

void launch_pose_info(hipStream_t s, const InfoLaunch& L) {
    const size_t c = (size_t)std::max(L.N, 0);
    Rows rows{L.cs, L.cd, L.cn, nullptr, nullptr, nullptr, L.weights, L.rows_d ? 1 : 0, L.count, L.wsum};
    if (L.rows_d) {
        rows.ds = L.rows_d;
        rows.dd = L.rows_d + 3 * c;
        rows.dn = L.rows_d + 6 * c;
    }
    const int nb = info_blocks(L.N);
    k_info_rows<<<nb, kBlock, 0, s>>>(rows, L.N, L.ex, L.slabs, L.robust_loss, L.robust_scale);
    k_info_final<<<1, 256, 0, s>>>(InfoFinalArgs{L.ex, L.status, L.iters, L.in_loop, L.solve_method, L.final_method,
                                                  L.slabs, nb, L.out});
}

}  // namespace imlsgpu
