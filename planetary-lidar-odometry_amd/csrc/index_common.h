// index_common.h — what the index units (filter.hip, index.hip, fifo_index.hip) share: one device
// body per build step, so the lone, batched and FIFO builders compute the same floats from one
// source text, and one host helper per piece of bookkeeping (tree shape, scratch layouts, the
// subtree round plan, the radix sort, the launch check).
#pragma once
#include "index.h"

namespace imlsgpu {

// ---- host bookkeeping ---------------------------------------------------------------------------

inline bool ensure(DevBuf& b, size_t bytes, std::string& err) {
    // a replaced buffer is retired behind the work that may still read it (internal.h devbuf_grow)
    if (devbuf_grow(b, bytes, bytes + bytes / 4 + 4096)) return true;
    err = "hipMalloc failed (" + std::to_string(bytes + bytes / 4 + 4096) + " bytes)";
    return false;
}

inline unsigned grid_for(size_t n, int b = kBlock) { return (unsigned)((n + b - 1) / b); }

// after a launch sequence: `what` names it in the context's error text
inline int launched(const char* what, std::string& err) {
    if (hipGetLastError() == hipSuccess) return IMLS_OK;
    err = what;
    return IMLS_ERR_DEVICE;
}

// Tree shape of M points in buckets of B: L leaves hold points, padded to P = 2^levels.
struct TreeShape { int L, P, levels; };
inline int tree_shape(int M, int B, TreeShape& t, std::string& err) {
    t.L = (M + B - 1) / B;
    t.P = 1;
    t.levels = 0;
    while (t.P < t.L) { t.P <<= 1; ++t.levels; }
    if (t.levels > kStackDepth - 1) { err = "tree too deep for the traversal stack"; return IMLS_ERR_CAPACITY; }
    return IMLS_OK;
}

// Scratch of one tree build: the P leaf boxes and the two buffers the subtree rounds alternate between.
struct TreeScratch { float *leafbox, *rootsA, *rootsB; };
inline size_t tree_root_floats(int P) { return ((size_t)P / kBlock + 1) * 6; }
inline size_t tree_scratch_bytes(int P) { return carve_bytes<float>((size_t)P * 6) + 2 * carve_bytes<float>(tree_root_floats(P)); }
inline TreeScratch tree_scratch(char*& p, int P) {
    TreeScratch t;
    t.leafbox = carve<float>(p, (size_t)P * 6);
    t.rootsA = carve<float>(p, tree_root_floats(P));
    t.rootsB = carve<float>(p, tree_root_floats(P));
    return t;
}

// The bottom-up reduction of P leaf boxes as rounds of k_subtree blocks: a block takes
// min(count, 256) consecutive boxes of depth D, so a round ends 8 levels higher (levels ≤ 23: three
// rounds at most).  The lone builders launch from the plan; the batched build copies it into its
// job table.
constexpr int kSubRounds = 4;
static_assert(kBlock == 256 && 8 * kSubRounds >= kStackDepth - 1, "the deepest tree tree_shape accepts must reduce within kSubRounds rounds");
struct SubRound {
    const float* in;                    // count boxes of depth D
    float* out;                         // one root box per block
    int count, D;
};
inline int subtree_width(int count) { return std::min(count, kBlock); }
inline int subtree_blocks(int count) { return count / subtree_width(count); }
// fills r[0 .. rounds) and returns rounds (the rest stays as given); −1: more than kSubRounds
inline int subtree_plan(const TreeScratch& t, int P, int levels, SubRound (&r)[kSubRounds]) {
    const float* in = t.leafbox;
    float* outs[2] = {t.rootsA, t.rootsB};
    int count = P, D = levels, n = 0;
    for (; count > 1; ++n) {
        if (n == kSubRounds) return -1;
        r[n] = SubRound{in, outs[n & 1], count, D};
        int lg = 0;
        while ((1 << lg) < subtree_width(count)) ++lg;
        in = outs[n & 1];
        count = subtree_blocks(count);
        D -= lg;
    }
    return n;
}

// The sort orders the full 48-bit Morton codes.  Sorting their top 32 bits only (two radix passes
// fewer, the lone frame's index build ~15 µs shorter) coarsens the order inside 1/1625-extent cells:
// config B's leaves and packets lose coherence, 423.7 → 397.5 pairs/s (round 4, profiles/r04_final3)
constexpr int kMortonSortLo = 0;

// Double-buffered radix sort of (64-bit key, 32-bit value) pairs on bits [kMortonSortLo, end_bit)
// (round 6: the plain form ended in two copy-back launches of keys and values): fill k0 / v0, run();
// afterwards k0 / v0 name whichever buffers hold the sorted pairs.
struct PairSort {
    unsigned long long *k0 = nullptr, *k1 = nullptr;
    unsigned *v0 = nullptr, *v1 = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    int n = 0, end_bit = 48;

    PairSort(int n_, int end_bit_, hipStream_t s = 0);   // sizes tmp_bytes (index.hip: hipcub is instantiated there alone)
    // own_v1: the caller's storage for the second value buffer (not carved)
    size_t bytes(bool own_v1 = false) const {
        return 2 * carve_bytes<unsigned long long>(n) + (own_v1 ? 1 : 2) * carve_bytes<unsigned>(n) + carve_bytes<char>(tmp_bytes);
    }
    void carve_from(char*& p, unsigned* own_v1 = nullptr) {
        k0 = carve<unsigned long long>(p, n);
        k1 = carve<unsigned long long>(p, n);
        v0 = carve<unsigned>(p, n);
        v1 = own_v1 ? own_v1 : carve<unsigned>(p, n);
        tmp = carve<char>(p, tmp_bytes);
    }
    void run(hipStream_t s);
};

// index.hip's launchers that fifo_index.hip shares (the kernels live in index.hip)
// ≤ `parts` blocks of k_bbox_partial over n points: six floats per block to `part`; returns the blocks
int bbox_partials(hipStream_t s, const float4* pts, int n, int parts, float* part);
// the internal levels from P leaf boxes (k_subtree rounds, 256 boxes per block per round)
void subtree_rounds(hipStream_t s, const TreeScratch& t, int P, int levels, float4* nodes);

// ---- device bodies ------------------------------------------------------------------------------

struct Box { float lo[3], hi[3]; };

__device__ __forceinline__ Box box_empty() { return Box{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}}; }
__device__ __forceinline__ void box_add(Box& b, const float4& p) {
    b.lo[0] = fminf(b.lo[0], p.x); b.lo[1] = fminf(b.lo[1], p.y); b.lo[2] = fminf(b.lo[2], p.z);
    b.hi[0] = fmaxf(b.hi[0], p.x); b.hi[1] = fmaxf(b.hi[1], p.y); b.hi[2] = fmaxf(b.hi[2], p.z);
}
__device__ __forceinline__ Box box_union(const Box& a, const Box& b) {
    Box r;
    for (int d = 0; d < 3; ++d) { r.lo[d] = fminf(a.lo[d], b.lo[d]); r.hi[d] = fmaxf(a.hi[d], b.hi[d]); }
    return r;
}

// The block's box from every thread's own, T threads: afterwards red[0..2][0] = min, red[3..5][0] =
// max, visible to the whole block (min / max are exact in any order).
template <int T>
__device__ __forceinline__ void block_box(const Box& mine, float (&red)[6][T]) {
    const int t = threadIdx.x;
    for (int d = 0; d < 3; ++d) { red[d][t] = mine.lo[d]; red[3 + d][t] = mine.hi[d]; }
    __syncthreads();
    for (int s = T / 2; s > 0; s >>= 1) {
        if (t < s)
            for (int d = 0; d < 3; ++d) {
                red[d][t] = fminf(red[d][t], red[d][t + s]);
                red[3 + d][t] = fmaxf(red[3 + d][t], red[3 + d][t + s]);
            }
        __syncthreads();
    }
}
// … from nparts block partials of six floats (k_bbox_partial's output)
template <int T>
__device__ __forceinline__ void block_box_of_parts(const float* __restrict__ part, int nparts, float (&red)[6][T]) {
    Box r = box_empty();
    for (int b = threadIdx.x; b < nparts; b += T)
        for (int d = 0; d < 3; ++d) {
            r.lo[d] = fminf(r.lo[d], part[b * 6 + d]);
            r.hi[d] = fmaxf(r.hi[d], part[b * 6 + 3 + d]);
        }
    block_box<T>(r, red);
}

// The Morton quantisation of a box (morton48's qp): origin = its min, one scale for all axes, the
// largest extent (at least 1e-6) on 16 bits.
__device__ __forceinline__ void box_quantisation(float lx, float ly, float lz, float hx, float hy, float hz, float* qp) {
    const float ext = fmaxf(fmaxf(fmaxf(hx - lx, hy - ly), hz - lz), 1e-6f);
    qp[0] = lx; qp[1] = ly; qp[2] = lz;
    qp[3] = 65535.f / ext;
}

// leaf box of bucket b = mpt[b·B, min((b+1)·B, M)); a bucket past the points is empty (inverted box,
// never visited)
__device__ __forceinline__ void leaf_box_body(const float4* __restrict__ mpt, int M, int B, int b, float* __restrict__ leafbox) {
    Box bx = box_empty();
    const int s = b * B, e = min(s + B, M);
    for (int k = s; k < e; ++k) box_add(bx, mpt[k]);
    for (int d = 0; d < 3; ++d) { leafbox[b * 6 + d] = bx.lo[d]; leafbox[b * 6 + 3 + d] = bx.hi[d]; }
}

// One block reduces width = 2^s (≤ 256) consecutive boxes of depth D into their subtree: writes the
// internal-node records of depths D−1 … D−s and the subtree root box to roots[blockIdx.x].
__device__ __forceinline__ void subtree_body(const float* __restrict__ in, int width, int D, float4* __restrict__ nodes,
                                             float* __restrict__ roots) {
    __shared__ Box sb[kBlock];
    const int t = threadIdx.x;
    const int base = blockIdx.x * width;
    if (t < width) {
        const float* q = in + (size_t)(base + t) * 6;
        for (int d = 0; d < 3; ++d) { sb[t].lo[d] = q[d]; sb[t].hi[d] = q[3 + d]; }
    }
    __syncthreads();
    int n = width, depth = D;
    while (n > 1) {
        n >>= 1;
        --depth;
        Box u;
        const bool act = t < n;
        if (act) {
            const Box l = sb[2 * t], r = sb[2 * t + 1];
            const int id = (1 << depth) + (base >> (D - depth)) + t;
            float4* rec = nodes + 3 * (size_t)id;
            rec[0] = make_float4(l.lo[0], l.lo[1], l.lo[2], l.hi[0]);
            rec[1] = make_float4(l.hi[1], l.hi[2], r.lo[0], r.lo[1]);
            rec[2] = make_float4(r.lo[2], r.hi[0], r.hi[1], r.hi[2]);
            u = box_union(l, r);
        }
        __syncthreads();
        if (act) sb[t] = u;
        __syncthreads();
    }
    if (t == 0)
        for (int d = 0; d < 3; ++d) { roots[blockIdx.x * 6 + d] = sb[0].lo[d]; roots[blockIdx.x * 6 + 3 + d] = sb[0].hi[d]; }
}

}  // namespace imlsgpu
