// solve.h — the Solving step as its callers see it: one dispatcher per launch shape
// (solve_dispatch.hip) over the LS / weighted-LS chain (solve.hip), the robust M-estimator
// (solve_robust.hip), RANSAC (ransac.hip, compact_rows.hip) and DRPM (drpm.hip); the pose-info
// pass over the last solve's rows (pose_info.hip).
#pragma once
#include "internal.h"

namespace imlsgpu {

constexpr int kHypMax = 8192;          // RANSAC hypotheses per chunk (ransac_chunks)
constexpr int kMaxRansacBatch = 1024;  // frames per batched RANSAC launch
struct RansacParams {
    int max_iterations;
    double distance_threshold, min_inliers_percentage, huber_threshold;
    int final_method;                  // imls_final_method
    double ls_threshold, drpm_threshold, drpm_stdev_points, drpm_stdev_normals;
};
struct SolveLaunch {
    int N;                             // rows (float rows: source count; fp64 rows: row count)
    int blocks1;                       // pass-1 slabs already in st.partial1 (float rows from k_finish)
    KParams kp;
    const float4 *cs, *cd, *cn;
    const double* rows_d;              // fp64 rows [s 3N | d 3N | n 3N] (host API) or null
    const double* weights;
    SolveState st;
    imls_iter_trace* tr;
    int update_pose, rows_are_double;
    const int* count;
    void* scratch;                     // ransac_bytes(N) device bytes (RANSAC and DRPM only)
    int* rng;                          // [34] glibc rand() state, device (RANSAC only)
    RansacParams ransac;
};

// solve_dispatch.hip — the solve sequence of L.kp.solve_method for one frame, and of kp.solve_method
// for all frames of tab (ICP iteration `it`; n_host: the frames' N; nonzero: launch_ransac_batch's).
void launch_solve(hipStream_t s, const SolveLaunch& L);
#pragma GCC visibility push(hidden)
int launch_solve_frames(hipStream_t s, const PairDev* tab, const int* n_host, int npairs, const KParams& kp,
                        const RansacParams& rp, int it);
#pragma GCC visibility pop

// solve.hip — LS / weighted LS
void launch_solve_chain(hipStream_t s, int N, int blocks1, const KParams& kp, const float4* cs,
                        const float4* cd, const float4* cn, const double* rows_d, const double* weights,
                        SolveState& st, imls_iter_trace* tr, int update_pose, int rows_are_double,
                        const int* count = nullptr, const double* wsum = nullptr);
// Batched LS / weighted-LS solve + pose update for all frames of tab (float rows from the batched
// projection): k_solve_small over the frames with N ≤ kSmallRows, the grid chain over the others.
// src 0: float rows of the batched projection; src 1: every frame's RANSAC inlier rows (fp64, the
// grid chain always; n_host = the frames' RANSAC caps), pass 1 included.
void launch_solve_batch(hipStream_t s, const PairDev* tab, const int* n_host, int npairs, const KParams& kp, int it,
                        int src = 0);
// pass 1 over every frame's RANSAC inlier rows (weighted: w / Σw)
void launch_rows_pass1_batch(hipStream_t s, const PairDev* tab, const int* cap_host, int npairs, int weighted);

// solve_robust.hip — the robust M-estimator solve (IMLS_SOLVE_ROBUST): K re-weighted 6×6 solves of
// the point-to-plane rows under ψ ∈ {Huber, Cauchy, Geman-McClure}, then Δ and the pose update.
// Float rows of ≤ kSmallRows: one block; larger frames and fp64 rows: K × (grid pass, one-block solve).
void launch_solve_robust(hipStream_t s, const SolveLaunch& L);
// every frame of tab (float rows of the batched projection), one launch per step for the whole batch
void launch_solve_robust_batch(hipStream_t s, const PairDev* tab, const int* n_host, int npairs, const KParams& kp, int it);

// ransac.hip — RANSAC with its final LS / weighted LS / DRPM, one frame; and for all frames of tab:
// one launch per step for the whole batch, every frame at its own count / rand() stream / done flag
// (nonzero, nothing enqueued: more than kMaxRansacBatch frames)
#pragma GCC visibility push(hidden)
void launch_ransac(hipStream_t s, const SolveLaunch& L);
#pragma GCC visibility pop
int launch_ransac_batch(hipStream_t s, const PairDev* tab, const int* n_host, int npairs, const KParams& kp,
                        const RansacParams& rp, int it);
size_t ransac_bytes(int cap);
RansacFrame ransac_frame(void* scratch, int cap, int* rng);   // the carve of ransac_bytes(cap)
int ransac_init_tables(int device);    // the rand() jump table on `device` (current), once per device
void ransac_seed_host(uint32_t seed, int st[34]);

// drpm.hip — the stand-alone DRPM solve on host fp64 rows + weights
#pragma GCC visibility push(hidden)
void launch_drpm_alone(hipStream_t s, const SolveLaunch& L);
#pragma GCC visibility pop

// pose_info.hip — the covariance / degeneracy report of the last solve (imls_capture_pose_info)
struct InfoLaunch {
    const float4 *cs, *cd, *cn;        // float rows of the projection, or
    const double* rows_d;              // fp64 rows [s 3n | d 3n | n 3n] (weights, count, wsum as Rows takes them)
    const double* weights;
    const int* count;
    const double* wsum;
    int N;                             // rows to visit
    const InfoExport* ex;
    const int *status, *iters;         // the frame's (SolveState)
    int in_loop;                       // a registration (its iteration must be the frame's last)
    int solve_method, final_method;
    int robust_loss;                   // ψ of a robust solve's weights (kInfoRobust)
    double robust_scale;
    double* slabs;                     // [info_blocks(N) × kInfoTerms]
    struct imls_pose_info* out;               // device
};
constexpr int kInfoTerms = 32;         // 21 H + 6 g + btb + Σw + rows + rss (+ 1 unused)
inline int info_blocks(int N) { return (std::max(N, 1) + kBlock - 1) / kBlock; }
void launch_pose_info(hipStream_t s, const InfoLaunch& L);

}  // namespace imlsgpu
