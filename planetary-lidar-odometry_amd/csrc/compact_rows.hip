// compact_rows.hip — order-keeping compaction (count → scan → scatter, or all three in one block)
// of correspondence rows into the fp64 row arrays the RANSAC solve works on (compact_rows.h), for a
// lone frame and for every frame of a batch (grid y = frame, the same bodies).
#include "compact_rows.h"

namespace imlsgpu {
namespace {

__device__ __forceinline__ void compact_count_body(const Source& src, int n, int* __restrict__ blkcnt,
                                                   double* __restrict__ blkw) {
    __shared__ int wc[kBlock / 64];
    __shared__ double ws[kBlock / 64];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    double s[3], d[3], nn[3], w = 0.0;
    const bool keep = i < n && src.get(i, s, d, nn, w);
    const unsigned long long m = __ballot(keep);
    const double wv = wave_sum(keep ? w : 0.0);
    if ((threadIdx.x & 63) == 0) { wc[threadIdx.x >> 6] = __popcll(m); ws[threadIdx.x >> 6] = wv; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        double sw = 0.0;
        for (int k = 0; k < kBlock / 64; ++k) { c += wc[k]; sw += ws[k]; }
        blkcnt[blockIdx.x] = c;
        blkw[blockIdx.x] = sw;
    }
}

// One block: exclusive scan of the block counts (in place), total count and Σw in fixed order.
__device__ __forceinline__ void compact_scan_body(int* __restrict__ blkcnt, const double* __restrict__ blkw, int nb,
                                                  const CompactOut& out, const CompactPost& P) {
    __shared__ int sc[1024];
    __shared__ double sw[1024];
    int carry = 0;
    double wcarry = 0.0;
    for (int base = 0; base < nb; base += 1024) {
        const int b = base + threadIdx.x;
        const int v = b < nb ? blkcnt[b] : 0;
        sc[threadIdx.x] = v;
        sw[threadIdx.x] = b < nb ? blkw[b] : 0.0;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int t = threadIdx.x >= off ? sc[threadIdx.x - off] : 0;
            __syncthreads();
            sc[threadIdx.x] += t;
            __syncthreads();
        }
        if (b < nb) blkcnt[b] = carry + sc[threadIdx.x] - v;
        if (threadIdx.x == 0) {
            double acc = 0.0;
            for (int k = 0; k < 1024 && base + k < nb; ++k) acc += sw[k];
            sw[0] = acc;   // reuse after the scan: chunk sum
        }
        __syncthreads();
        carry += sc[1023];
        wcarry += sw[0];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *out.count = carry;
        if (out.wsum) *out.wsum = wcarry;
        compact_post(P, carry);
    }
}

__device__ __forceinline__ void compact_scatter_body(const Source& src, int n, const int* __restrict__ blkoff,
                                                     const CompactOut& out) {
    __shared__ int wc[kBlock / 64];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double s[3], d[3], nn[3], w = 0.0;
    const bool keep = i < n && src.get(i, s, d, nn, w);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wc[wv] = __popcll(m);
    __syncthreads();
    int off = blkoff[blockIdx.x];
    for (int k = 0; k < wv; ++k) off += wc[k];
    off += __popcll(m & ((1ull << lane) - 1ull));
    if (keep) store_row(out, off, s, d, nn, w);
}

__global__ __launch_bounds__(kBlock) void k_compact_count(Source src, int n, int* __restrict__ blkcnt,
                                                          double* __restrict__ blkw, const int* __restrict__ done) {
    if (done && *done) return;
    compact_count_body(src, n, blkcnt, blkw);
}
__global__ __launch_bounds__(1024) void k_compact_scan(int* __restrict__ blkcnt, const double* __restrict__ blkw, int nb,
                                                       CompactOut out, CompactPost P) {
    if (compact_skip(P)) return;
    compact_scan_body(blkcnt, blkw, nb, out, P);
}
__global__ __launch_bounds__(1024) void k_compact_one(Source src, int n, CompactOut out, CompactPost P) {
    if (compact_skip(P)) return;
    compact_one_body(src, n, out, P);
}
__global__ __launch_bounds__(kBlock) void k_compact_scatter(Source src, int n, const int* __restrict__ blkoff, CompactOut out,
                                                            const int* __restrict__ done) {
    if (done && *done) return;
    compact_scatter_body(src, n, blkoff, out);
}

// The two compactions of a batched frame (launch_compact_batch's modes); returns the rows to visit.
__device__ __forceinline__ int frame_compact(const PairDev& A, int mode, double dist_thr, double h2, Source& src,
                                             CompactOut& out) {
    if (mode == 0) {
        src = Source::valid(A.cs, A.cd, A.cn);
        out = CompactOut::valid(A.rf);
        return A.N;
    }
    src = Source::inliers(A.rf, dist_thr, h2);
    out = CompactOut::inliers(A.rf);
    return A.rf.cap;
}
__device__ __forceinline__ CompactPost frame_post(const PairDev& A, int mode, int correspond_number, int it) {
    return CompactPost{mode == 0 ? 1 : 2, correspond_number, 1, A.st, A.trace + it, A.rf.R};
}
__global__ __launch_bounds__(kBlock) void k_compact_count_b(const PairDev* __restrict__ tab, int mode, double dist_thr,
                                                            double h2) {
    const PairDev A = device_view(tab + blockIdx.y);
    Source src;
    CompactOut out;
    const int n = frame_compact(A, mode, dist_thr, h2, src, out);
    if ((int)blockIdx.x >= (n + kBlock - 1) / kBlock || *A.st.done) return;
    compact_count_body(src, n, A.rf.blkcnt, A.rf.blkw);
}
__global__ __launch_bounds__(1024) void k_compact_scan_b(const PairDev* __restrict__ tab, int mode, int correspond_number,
                                                         int it) {
    const PairDev A = device_view(tab + blockIdx.y);
    const CompactPost P = frame_post(A, mode, correspond_number, it);
    if (compact_skip(P)) return;
    Source src;
    CompactOut out;
    const int n = frame_compact(A, mode, 0.0, 0.0, src, out);
    compact_scan_body(A.rf.blkcnt, A.rf.blkw, (n + kBlock - 1) / kBlock, out, P);
}
__global__ __launch_bounds__(1024) void k_compact_one_b(const PairDev* __restrict__ tab, int mode, double dist_thr, double h2,
                                                        int correspond_number, int it) {
    const PairDev A = device_view(tab + blockIdx.y);
    const CompactPost P = frame_post(A, mode, correspond_number, it);
    if (compact_skip(P)) return;
    Source src;
    CompactOut out;
    const int n = frame_compact(A, mode, dist_thr, h2, src, out);
    compact_one_body(src, n, out, P);
}
__global__ __launch_bounds__(kBlock) void k_compact_scatter_b(const PairDev* __restrict__ tab, int mode, double dist_thr,
                                                              double h2) {
    const PairDev A = device_view(tab + blockIdx.y);
    Source src;
    CompactOut out;
    const int n = frame_compact(A, mode, dist_thr, h2, src, out);
    if ((int)blockIdx.x >= (n + kBlock - 1) / kBlock || *A.st.done) return;
    compact_scatter_body(src, n, A.rf.blkcnt, out);
}

}  // namespace

void launch_compact(hipStream_t s, const Source& src, int n, const CompactOut& out, const CompactPost& P, const RansacFrame& F) {
    if (F.cap <= kCompactOne) {
        k_compact_one<<<1, 1024, 0, s>>>(src, n, out, P);
        return;
    }
    const int nb = solve_blocks(F.cap);
    k_compact_count<<<nb, kBlock, 0, s>>>(src, n, F.blkcnt, F.blkw, P.st.done);
    k_compact_scan<<<1, 1024, 0, s>>>(F.blkcnt, F.blkw, nb, out, P);
    k_compact_scatter<<<nb, kBlock, 0, s>>>(src, n, F.blkcnt, out, P.st.done);
}

void launch_compact_batch(hipStream_t s, const PairDev* tab, int npairs, int maxc, int mode, double dist_thr, double h2,
                          int correspond_number, int it) {
    const dim3 gc(solve_blocks(maxc), npairs), g1(1, npairs);
    if (maxc <= kCompactOne) {
        k_compact_one_b<<<g1, 1024, 0, s>>>(tab, mode, dist_thr, h2, correspond_number, it);
        return;
    }
    k_compact_count_b<<<gc, kBlock, 0, s>>>(tab, mode, dist_thr, h2);
    k_compact_scan_b<<<g1, 1024, 0, s>>>(tab, mode, correspond_number, it);
    k_compact_scatter_b<<<gc, kBlock, 0, s>>>(tab, mode, dist_thr, h2);
}

}  // namespace imlsgpu
