// compact_rows.h — the order-keeping row compaction of the RANSAC solve (compact_rows.hip): valid
// correspondences, or the inliers of a Δ with their weights, into fp64 row arrays of stride `cap`.
// What a compaction reads (Source), writes (CompactOut) and runs on the kept count (CompactPost), the
// two host calls, and the one-block body that k_drpm_head_small (ransac.hip) runs inside its block.
#pragma once
#include "solve_common.h"

namespace imlsgpu {

constexpr int kCompactOne = 16384;    // caps up to this: the whole compaction in one 1024-thread block

struct CompactOut {
    double* rows;       // [10·cap]: s[3·cap] | d[3·cap] | n[3·cap] (xyz per row) | w[cap] — the Rows layout
    int* count;         // [1]
    double* wsum;       // [1] Σw of the kept rows (inlier pass) — may be null
    int cap;
    static __host__ __device__ CompactOut valid(const RansacFrame& F) { return CompactOut{F.all, F.cnt_all, nullptr, F.cap}; }
    static __host__ __device__ CompactOut inliers(const RansacFrame& F) { return CompactOut{F.inl, F.cnt_in, F.wsum, F.cap}; }
};

// Predicate + payload: valid correspondences of the projection (float rows), or inliers of Δ.
struct Source {
    const float4 *cs, *cd, *cn;       // float rows (valid flag cs.w), or null
    const double* rows;               // fp64 rows (Rows layout, stride cap) with count, or null
    const int* count;
    int cap;
    const double* T;                  // inlier pass: Δ (row-major 4×4)
    double dist_thr, h2;
    static __host__ __device__ Source valid(const float4* cs, const float4* cd, const float4* cn) {
        Source s{};
        s.cs = cs; s.cd = cd; s.cn = cn;
        return s;
    }
    // the frame's valid rows within dist_thr of the plane under its best Δ, Huber knee h2
    static __host__ __device__ Source inliers(const RansacFrame& F, double dist_thr, double h2) {
        Source s{};
        s.rows = F.all; s.count = F.cnt_all; s.cap = F.cap; s.T = F.R.bestT;
        s.dist_thr = dist_thr; s.h2 = h2;
        return s;
    }
    __device__ __forceinline__ bool get(int i, double s[3], double d[3], double n[3], double& w) const {
        if (cs) {
            const float4 s4 = cs[i];
            if (s4.w == 0.f) return false;
            const float4 d4 = cd[i], n4 = cn[i];
            s[0] = s4.x; s[1] = s4.y; s[2] = s4.z;
            d[0] = d4.x; d[1] = d4.y; d[2] = d4.z;
            n[0] = n4.x; n[1] = n4.y; n[2] = n4.z;
            w = 1.0;
            return true;
        }
        if (i >= *count) return false;
        const size_t c3 = 3 * (size_t)cap;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s[k] = rows[3 * (size_t)i + k];
            d[k] = rows[c3 + 3 * (size_t)i + k];
            n[k] = rows[2 * c3 + 3 * (size_t)i + k];
        }
        if (!T) { w = 1.0; return true; }
        // solver.cpp:301-314 / 334-356: point-to-plane distance of Δ·s
        double tp[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) tp[r] = ((T[r * 4] * s[0] + T[r * 4 + 1] * s[1]) + T[r * 4 + 2] * s[2]) + T[r * 4 + 3];
        const double dist = fabs(((tp[0] - d[0]) * n[0] + (tp[1] - d[1]) * n[1]) + (tp[2] - d[2]) * n[2]);
        if (!(dist < dist_thr)) return false;
        const double ar = exp(-fabs(dist));
        w = sqrt(ar) < h2 ? ar : 2 * h2 * sqrt(ar) - h2 * h2;
        return true;
    }
};

// What runs after a compaction, by thread 0 with the kept count (one launch fewer each): the RANSAC
// begin (the TOO_FEW gate, laser_odometry.cpp:570-576, and the selection reset) after the valid-row
// compaction; the empty-inlier check after the inlier one.
struct CompactPost {
    int kind;                         // 0 none, 1 RANSAC begin, 2 inlier check
    int correspond_number, update_pose;
    SolveState st;
    imls_iter_trace* tr;
    RansacDev R;
};

#pragma GCC visibility push(hidden)
// One compaction of a lone frame with its post step folded in: one block for F.cap ≤ kCompactOne,
// else count → scan → scatter over F's block arrays.
void launch_compact(hipStream_t s, const Source& src, int n, const CompactOut& out, const CompactPost& P, const RansacFrame& F);
// One compaction per frame of tab (grid y = frame), ICP iteration `it`.  mode 0: the frame's valid
// float rows → all, then the count gate and selection reset; mode 1: the inliers of its best Δ,
// weighted → inl (+ Σw), then the empty-set check.  maxc: the largest cap of the batch.
void launch_compact_batch(hipStream_t s, const PairDev* tab, int npairs, int maxc, int mode, double dist_thr, double h2,
                          int correspond_number, int it);
#pragma GCC visibility pop

namespace {

__device__ __forceinline__ void compact_post(const CompactPost& P, int n) {
    if (P.kind == 1) {
        const RansacDev& R = P.R;
        *R.active = 1;
        if (P.update_pose && n < P.correspond_number) {
            *P.st.status = IMLS_FRAME_TOO_FEW;
            *P.st.done = 1;
            if (P.tr) P.tr->n_valid = (unsigned long long)n;
            return;
        }
        *R.best = 0;
        *R.evaluated = 0;
        *R.rdone = n < 3 ? 1 : 0;   // FPS needs three distinct points
#pragma unroll
        for (int k = 0; k < 16; ++k) R.bestT[k] = (k % 5 == 0) ? 1.0 : 0.0;
    } else if (P.kind == 2 && n == 0) {   // nothing to solve on (the oracle's N == 0 → false): a failed solve
        *P.st.status = IMLS_FRAME_SOLVE_FAILED;
        *P.st.done = 1;
    }
}
// a finished frame skips the compaction; its RANSAC solve is then inactive (no trace record)
__device__ __forceinline__ bool compact_skip(const CompactPost& P) {
    if (!*P.st.done) return false;
    if (P.kind == 1 && threadIdx.x == 0) *P.R.active = 0;
    return true;
}

// kept row → slot o of the output
__device__ __forceinline__ void store_row(const CompactOut& out, int o, const double s[3], const double d[3],
                                          const double n[3], double w) {
    const size_t c3 = 3 * (size_t)out.cap, o3 = 3 * (size_t)o;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out.rows[o3 + k] = s[k];
        out.rows[c3 + o3 + k] = d[k];
        out.rows[2 * c3 + o3 + k] = n[k];
    }
    out.rows[3 * c3 + (size_t)o] = w;
}

// The whole compaction in one 1024-thread block (count + scan + scatter, for caps ≤ kCompactOne):
// tiles of 1024 rows in order; Σw accumulated exactly as the three-kernel path does it (per-wave
// sums, 4 waves per 256-row block in order, then the block sums in block order) — same bits.
__device__ __forceinline__ void compact_one_body(const Source& src, int n, const CompactOut& out, const CompactPost& P) {
    __shared__ int wc[16];
    __shared__ double ws[16];
    __shared__ int sbase;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t == 0) sbase = 0;
    double wacc = 0.0;                                     // thread 0
    for (int tile = 0; tile < n; tile += 1024) {
        const int i = tile + t;
        double s[3], d[3], nn[3], w = 0.0;
        const bool keep = i < n && src.get(i, s, d, nn, w);
        const unsigned long long m = __ballot(keep);
        const double wvs = wave_sum(keep ? w : 0.0);
        if (lane == 0) { wc[wv] = __popcll(m); ws[wv] = wvs; }
        __syncthreads();
        int off = sbase;
        for (int k = 0; k < wv; ++k) off += wc[k];
        off += __popcll(m & ((1ull << lane) - 1ull));
        if (keep) store_row(out, off, s, d, nn, w);
        __syncthreads();
        if (t == 0) {
            int tot = 0;
            for (int b = 0; b < 4; ++b) {
                if (tile + 256 * b >= n) break;            // blocks past n do not exist in the 3-kernel path
                double sw = 0.0;
                for (int k = 0; k < 4; ++k) { sw += ws[4 * b + k]; tot += wc[4 * b + k]; }
                wacc += sw;
            }
            sbase += tot;
        }
        __syncthreads();
    }
    if (t == 0) {
        *out.count = sbase;
        if (out.wsum) *out.wsum = wacc;
        compact_post(P, sbase);
    }
}

}  // namespace
}  // namespace imlsgpu
