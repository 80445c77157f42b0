// drpm_common.h — what the DRPM solve (drpm.hip) shares with the RANSAC unit (ransac.hip): its scratch
// piece, its launch sequence, and the two bodies that k_drpm_head_small and RANSAC's trace kernels run.
#pragma once
#include "solve.h"
#include "solve_common.h"

namespace imlsgpu {

constexpr int kDrpmSlab = 42;         // 36 noise-mean terms + 6 variance terms per block

// the DRPM piece of a scratch layout for `blocks` row blocks (ransac_frame, the stand-alone DRPM)
inline DrpmDev drpm_carve(char*& p, int blocks) {
    DrpmDev Dv;
    Dv.H = carve<double>(p, 36);
    Dv.g = carve<double>(p, 6);
    Dv.U = carve<double>(p, 36);
    Dv.ev = carve<double>(p, 6);
    Dv.slabs = carve<double>(p, (size_t)(blocks + 1) * kDrpmSlab);
    return Dv;
}

#pragma GCC visibility push(hidden)
// The DRPM solve on `rows` (cap of them at most, weights w / Σw): pass 1 of the weighted normal
// equations → k_drpm_eig → k_drpm_noise → k_drpm_final.  head_done: k_drpm_head_small has run pass 1
// and the eigendecomposition already.  R / rtr: RANSAC's own trace record, written by the final
// kernel after the solve's when the RANSAC solve was active (rtr null: the stand-alone DRPM).
void launch_drpm(hipStream_t s, const Rows& rows, int cap, const SolveState& st, const DrpmDev& Dv, imls_iter_trace* tr,
                 const KParams& kp, const RansacParams& rp, const int* cnt_all, const int* cnt_in, int update_pose,
                 const RansacDev& R, imls_iter_trace* rtr, bool head_done);
// every frame of tab on its RANSAC inlier rows (grid y = frame), ICP iteration `it`; maxc: the largest cap
void launch_drpm_batch(hipStream_t s, const PairDev* tab, const int* cap_host, int npairs, int maxc, const KParams& kp,
                       const RansacParams& rp, int it);
void launch_set_count(hipStream_t s, int* count, int v);   // *count = v on the stream (fp64 rows that arrive compact)
#pragma GCC visibility pop

namespace {

// H (row-major, from the upper-triangle terms) and g of the reduced normal equations acc[kNormEq];
// the eigendecomposition by wave 0 (the caller's threads ≥ 64 have left), lane k holding row k
// (sym_eig6_wave: the oracle's Jacobi, operation for operation).  Returns the sweeps run.
__device__ __forceinline__ int drpm_eig_tail(const double* acc, const DrpmDev& Dv) {
    const int lane = threadIdx.x, k = lane < 6 ? lane : 0;
    double row[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const int r0 = k < c ? k : c, c0 = k < c ? c : k;
        row[c] = acc[6 * r0 - r0 * (r0 - 1) / 2 + (c0 - r0)];
    }
    if (lane < 6) {
#pragma unroll
        for (int c = 0; c < 6; ++c) Dv.H[lane * 6 + c] = row[c];
        Dv.g[lane] = acc[21 + lane];
    }
    return sym_eig6_wave(row, Dv.ev, Dv.U);
}

// trace of a RANSAC iteration as the oracle records it (n_valid = correspondences, n_kept = 0), when
// the RANSAC solve was active; after the final solve's own record (rtr null: none, R unread)
__device__ __forceinline__ void ransac_trace_t0(const RansacDev& R, const int* __restrict__ count_all, imls_iter_trace* rtr) {
    if (threadIdx.x == 0 && rtr && *R.active) {
        rtr->n_valid = (unsigned long long)*count_all;
        rtr->n_kept = 0;
    }
}

}  // namespace
}  // namespace imlsgpu
