// fifo_index.hip — incremental index of the map FIFO (accumulateTargetCloud, laser_odometry.cpp:116-136: the last
// max_queue_size filtered scans, oldest first; setTargetPointCloud rebuilds libnabo's tree over
// their concatenation every frame, imls_icp.cpp:80-103).  With a quantisation frame fixed for the
// FIFO, a scan's Morton keys never change: each scan is sorted ONCE (a run, fifo_run_build), and a
// registration only merges — the previous merged order minus the evicted scans (a stable
// compaction), merged with the new runs (merge path, older entries first on equal keys).  That is
// exactly the stable sort of the concatenation by key, i.e. the order the full build gives under
// the same quantisation; the records then get their concatenated filtered index (the libnabo tie
// order, mpt[].w), ipos, the leaf keys and the tree (fifo_index).
#include "index_common.h"

namespace imlsgpu {
namespace {

constexpr int kMergeTile = 2048;            // outputs per merge block (12 B each in LDS)

// keys under the fixed quantisation fq; points outside its cube (clamped: still exact, the tree's
// boxes come from the points) are counted, so the host can re-frame the FIFO at its next build
__global__ void k_morton_fq(const float4* __restrict__ pt, int n, const float* __restrict__ fq,
                            unsigned long long* __restrict__ key, unsigned* __restrict__ val, unsigned* __restrict__ clamp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool out = false;
    if (i < n) {
        const float4 p = pt[i];
        key[i] = morton48(p.x, p.y, p.z, fq);
        val[i] = (unsigned)i;
        const float sc = fq[3], qmax = 65535.f;
        const float u = (p.x - fq[0]) * sc, v = (p.y - fq[1]) * sc, w = (p.z - fq[2]) * sc;
        out = !(u >= 0.f && u <= qmax && v >= 0.f && v <= qmax && w >= 0.f && w <= qmax);
    }
    const unsigned long long m = __ballot(out);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(clamp, (unsigned)__popcll(m));
}

// a run's Morton-ordered records: rpt = (xyz, bits(local filtered index)), rnr, and its sorted keys
// (from wherever the double-buffered sort left them: no copy-back launches)
__global__ void k_run_gather(const float4* __restrict__ pt, const float4* __restrict__ nr, const unsigned* __restrict__ perm,
                             const unsigned long long* __restrict__ skey, int n, float4* __restrict__ rpt,
                             float4* __restrict__ rnr, unsigned long long* __restrict__ rkey) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const unsigned j = perm[k];
    const float4 p = pt[j];
    rpt[k] = make_float4(p.x, p.y, p.z, __uint_as_float(j));
    rnr[k] = nr[j];
    rkey[k] = skey[k];
}

// the FIFO quantisation frame: a cube of side 2 × the runs' largest bbox extent, its origin half an
// extent below their bbox on every axis (later scans of a moving sensor stay inside; the host
// re-frames if one does not).  Side and offset are powers of two times the full build's cell
// (origin = bbox min, side = extent): the grid lines are the full build's, one level up, so the
// Morton order — and the tree — is the full build's up to the top-level block order and the last
// bit (on config B's map the query-ball overlaps of leaves / nodes are 8.03 / 74.1 per query vs the
// full build's 7.80 / 73.5; a 1.5× cube centred on the bbox gave 8.85 / 86.4:
// tools/fifo_frame_probe.py)
__global__ void k_fifo_frame(const float* __restrict__ part, int nparts, float* __restrict__ fq) {
    __shared__ float red[6][kBlock];
    block_box_of_parts<kBlock>(part, nparts, red);
    if (threadIdx.x == 0) {
        float ext = 1e-6f;
        for (int d = 0; d < 3; ++d) ext = fmaxf(ext, red[3 + d][0] - red[d][0]);
        const float side = 2.0f * ext;
        for (int d = 0; d < 3; ++d) fq[d] = red[d][0] - 0.5f * ext;
        fq[3] = 65535.f / side;
    }
}

// stable compaction of the merged order: entries whose run id (val >> 27) is live.  Two launches
// (round 6: count + scan + scatter and the scan's init were four): tiles of kKeepTile entries, 16 per
// thread in order; the scatter block sums the earlier tiles' counts itself (≤ a few hundred words)
// instead of a device-wide scan launch
__device__ __forceinline__ bool live_entry(unsigned v, unsigned live) { return (live >> (v >> 27)) & 1u; }
constexpr int kKeepPer = 16;
constexpr int kKeepTile = kBlock * kKeepPer;   // entries per block: kKeepPer rounds of kBlock, coalesced
__global__ __launch_bounds__(kBlock) void k_keep_count(const unsigned* __restrict__ val, int n, unsigned live, int* __restrict__ blk) {
    __shared__ int wc[kBlock / 64];
    const int base = blockIdx.x * kKeepTile + threadIdx.x;
    int c = 0;
#pragma unroll
    for (int k = 0; k < kKeepPer; ++k) {
        const int i = base + k * kBlock;
        c += (i < n && live_entry(val[i], live)) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int k = 0; k < kBlock / 64; ++k) t += wc[k];
        blk[blockIdx.x] = t;
    }
}
__global__ __launch_bounds__(kBlock) void k_keep_scatter(const unsigned long long* __restrict__ key, const unsigned* __restrict__ val,
                                                         int n, unsigned live, const int* __restrict__ blk,
                                                         unsigned long long* __restrict__ okey, unsigned* __restrict__ oval) {
    __shared__ int wsum[kKeepPer][kBlock / 64];
    __shared__ int s_off;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // this tile's output offset: Σ of the earlier tiles' counts
    int pre = 0;
    for (int b = tid; b < (int)blockIdx.x; b += kBlock) pre += blk[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pre += __shfl_xor(pre, o, 64);
    if (lane == 0) wsum[0][wv] = pre;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int k = 0; k < kBlock / 64; ++k) t += wsum[0][k];
        s_off = t;
    }
    __syncthreads();
    // every round's wave counts first (one barrier), then each entry's rank in tile order
    const int base = blockIdx.x * kKeepTile + tid;
    unsigned long long m[kKeepPer];
#pragma unroll
    for (int k = 0; k < kKeepPer; ++k) {
        const int i = base + k * kBlock;
        m[k] = __ballot(i < n && live_entry(val[i], live));
        if (lane == 0) wsum[k][wv] = __popcll(m[k]);
    }
    __syncthreads();
    int run = s_off;
#pragma unroll
    for (int k = 0; k < kKeepPer; ++k) {
        int before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) {
            before += w < wv ? wsum[k][w] : 0;
            tot += wsum[k][w];
        }
        if ((m[k] >> lane) & 1ull) {
            const int i = base + k * kBlock;
            const int o = run + before + __popcll(m[k] & ((1ull << lane) - 1ull));
            okey[o] = key[i];
            oval[o] = val[i];
        }
        run += tot;
    }
}

// merge path: the entries of A among the first d outputs of merge(A, B), A first on equal keys
// (A: the older entries)
__device__ __forceinline__ int merge_split_at(const unsigned long long* __restrict__ a, int na,
                                              const unsigned long long* __restrict__ b, int nb, long long d) {
    int lo = (int)std::max(0ll, d - nb), hi = (int)std::min<long long>(d, na);
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= b[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// one output tile of kMergeTile: its two splits by binary search on the diagonals (threads 0 / 1;
// round 6: a separate split launch before), both input segments in LDS; then each thread finds its own
// diagonal split of the tile (one binary search in LDS) and merges its kMergePer consecutive outputs
// sequentially (round 6: one binary search per output before), A first on equal keys.  B's values
// are (bid << 27) | index (a run's entries in its sorted order)
constexpr int kMergePer = kMergeTile / kBlock;
__global__ __launch_bounds__(kBlock) void k_merge_tile(const unsigned long long* __restrict__ a, const unsigned* __restrict__ av,
                                                       int na, const unsigned long long* __restrict__ b, unsigned bid, int nb,
                                                       unsigned long long* __restrict__ okey, unsigned* __restrict__ oval) {
    __shared__ unsigned long long sk[kMergeTile];
    __shared__ unsigned sv[kMergeTile];
    __shared__ int ssplit[2];
    const int t = blockIdx.x;
    const long long d0 = (long long)t * kMergeTile, d1 = std::min(d0 + kMergeTile, (long long)na + nb);
    if (threadIdx.x < 2) ssplit[threadIdx.x] = merge_split_at(a, na, b, nb, threadIdx.x ? d1 : d0);
    __syncthreads();
    const int i0 = ssplit[0], i1 = ssplit[1];
    const int j0 = (int)(d0 - i0), j1 = (int)(d1 - i1);
    const int la = i1 - i0, lb = j1 - j0;
    for (int k = threadIdx.x; k < la; k += kBlock) { sk[k] = a[i0 + k]; sv[k] = av[i0 + k]; }
    for (int k = threadIdx.x; k < lb; k += kBlock) { sk[la + k] = b[j0 + k]; sv[la + k] = (bid << 27) | (unsigned)(j0 + k); }
    __syncthreads();
    // this thread's outputs [q, q + kMergePer) of the tile: x of A's entries before output q
    const int q = threadIdx.x * kMergePer, n = la + lb;
    if (q >= n) return;
    int lo = max(0, q - lb), hi = min(q, la);
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sk[mid] <= sk[la + q - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    int x = lo, y = q - lo;
    const int qe = min(q + kMergePer, n);
    for (int r = q; r < qe; ++r) {
        const bool takeA = y >= lb || (x < la && sk[x] <= sk[la + y]);
        const int src = takeA ? x : la + y;
        okey[d0 + r] = sk[src];
        oval[d0 + r] = sv[src];
        x += takeA ? 1 : 0;
        y += takeA ? 0 : 1;
    }
}

// the index records from the merged order: mpt (xyz, bits(concatenated filtered index)), mnr, ipos,
// every B-th key (the leaves' first keys, for the seed search) — and, fused in (round 6: four launches
// fewer — k_leaf_boxes, and three small copies), each leaf's box (a segmented min / max over the B
// lanes of its points: the same values as k_leaf_boxes' serial loop, min / max being exact), the
// padded leaves' empty boxes, the quantisation after the leaf keys (TreeView::qparams) and this
// build's clamp count into the host's coherent word.  The run table comes by value.
__global__ __launch_bounds__(kBlock) void k_fifo_gather(const unsigned long long* __restrict__ mkey,
                                                        const unsigned* __restrict__ mval, int M, FifoRunTable runs, int B,
                                                        int L, int P, const float* __restrict__ fq,
                                                        const unsigned* __restrict__ clamp, unsigned* __restrict__ h_clamp,
                                                        float4* __restrict__ mpt, float4* __restrict__ mnr,
                                                        unsigned* __restrict__ ipos, unsigned long long* __restrict__ lkeys,
                                                        float* __restrict__ leafbox) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (k < M) {
        const unsigned v = mval[k];
        const FifoRun r = runs.r[v >> 27];
        const unsigned pos = v & ((1u << 27) - 1u);
        const float4 p = r.rpt[pos];
        const unsigned w = r.off + __float_as_uint(p.w);
        mpt[k] = make_float4(p.x, p.y, p.z, __uint_as_float(w));
        mnr[k] = r.rnr[pos];
        ipos[w] = (unsigned)k;
        if (k % B == 0) lkeys[k / B] = mkey[k];
        lo[0] = hi[0] = p.x; lo[1] = hi[1] = p.y; lo[2] = hi[2] = p.z;
    }
    // leaf k / B = lanes [k − k % B, … + B) of this wave (B divides 64)
    for (int o = 1; o < B; o <<= 1) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = fminf(lo[d], __shfl_xor(lo[d], o, 64));
            hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], o, 64));
        }
    }
    if (k < M && k % B == 0) {
        float* q = leafbox + (size_t)(k / B) * 6;
        q[0] = lo[0]; q[1] = lo[1]; q[2] = lo[2]; q[3] = hi[0]; q[4] = hi[1]; q[5] = hi[2];
    }
    if (k < P - L) {                           // padded leaves L … P−1: empty boxes
        float* q = leafbox + (size_t)(L + k) * 6;
        q[0] = q[1] = q[2] = INFINITY;
        q[3] = q[4] = q[5] = -INFINITY;
    }
    if (k < 4) reinterpret_cast<float*>(lkeys + L)[k] = fq[k];
    if (k == 0) *h_clamp = *clamp;
}

}  // namespace

constexpr int kFrameParts = 64;             // bbox partial blocks per run

size_t fifo_scratch_bytes(int max_run, int nruns, int M) {
    const int nb = (int)grid_for((size_t)std::max(M, 1));
    const size_t run = PairSort(std::max(max_run, 1), 48).bytes() + 1024;
    const size_t frame = (size_t)std::max(nruns, 1) * kFrameParts * 24 + 1024;
    const size_t keep = 2 * carve_bytes<int>(nb) + 1024;
    const size_t merge = ((size_t)M / kMergeTile + 2) * 4 + 256;
    return std::max(std::max(run, frame), std::max(keep, merge));
}

int fifo_frame(hipStream_t s, const std::vector<std::pair<const float4*, int>>& runs, float* fq, DevBuf& scratch,
               std::string& err) {
    if (!ensure(scratch, runs.size() * kFrameParts * 24 + 1024, err)) return IMLS_ERR_DEVICE;
    float* part = (float*)scratch.p;
    int np = 0;
    for (const auto& r : runs)
        if (r.second > 0) np += bbox_partials(s, r.first, r.second, kFrameParts, part + (size_t)np * 6);
    if (np == 0) return IMLS_OK;
    k_fifo_frame<<<1, kBlock, 0, s>>>(part, np, fq);
    return launched("FIFO frame launch failed", err);
}

int fifo_run_build(hipStream_t s, const float4* fpt, const float4* fnr, int n, const float* fq, unsigned* clamp,
                   DevBuf& run, DevBuf& scratch, std::string& err) {
    if (n <= 0) return IMLS_OK;
    if (n >= (1 << 27)) { err = "scan too large for the FIFO index"; return IMLS_ERR_CAPACITY; }
    PairSort sort(n, 48, s);
    if (!ensure(scratch, sort.bytes(), err) || !ensure(run, fifo_run_bytes(n), err)) return IMLS_ERR_DEVICE;
    char* p = (char*)scratch.p;
    sort.carve_from(p);
    k_morton_fq<<<grid_for(n), kBlock, 0, s>>>(fpt, n, fq, sort.k0, sort.v0, clamp);
    sort.run(s);
    // k_run_gather takes the keys from wherever the sort left them
    k_run_gather<<<grid_for(n), kBlock, 0, s>>>(fpt, fnr, sort.v0, sort.k0, n, fifo_run_pts(run.p, n),
                                                fifo_run_nrm(run.p, n), fifo_run_keys(run.p, n));
    return launched("FIFO run build launch failed", err);
}

int fifo_keep(hipStream_t s, const unsigned long long* key, const unsigned* val, int n, unsigned live,
              unsigned long long* okey, unsigned* oval, DevBuf& scratch, std::string& err) {
    if (n <= 0) return IMLS_OK;
    const int nb = (n + kKeepTile - 1) / kKeepTile;
    if (!ensure(scratch, carve_bytes<int>(nb) + 1024, err)) return IMLS_ERR_DEVICE;
    int* blk = (int*)scratch.p;
    k_keep_count<<<nb, kBlock, 0, s>>>(val, n, live, blk);
    k_keep_scatter<<<nb, kBlock, 0, s>>>(key, val, n, live, blk, okey, oval);
    return launched("FIFO compaction launch failed", err);
}

int fifo_merge(hipStream_t s, const unsigned long long* a, const unsigned* av, int na, const unsigned long long* b,
               unsigned bid, int nb, unsigned long long* okey, unsigned* oval, std::string& err) {
    const int tiles = (int)(((long long)na + nb + kMergeTile - 1) / kMergeTile);
    if (tiles == 0) return IMLS_OK;
    k_merge_tile<<<tiles, kBlock, 0, s>>>(a, av, na, b, bid, nb, okey, oval);
    return launched("FIFO merge launch failed", err);
}

int fifo_index(hipStream_t s, const unsigned long long* mkey, const unsigned* mval, int M, const FifoRunTable& runs,
               const float* fq, const unsigned* clamp, unsigned* h_clamp, int B, DevBuf& lkeys, DevBuf& mpt, DevBuf& nodes,
               DevBuf& treescratch, int* P_out, int* levels_out, std::string& err) {
    if (M <= 0) { *P_out = 0; *levels_out = 0; return IMLS_OK; }
    TreeShape t;
    if (int rc = tree_shape(M, B, t, err)) return rc;
    if (!ensure(treescratch, tree_scratch_bytes(t.P), err) || !ensure(mpt, (size_t)M * 36 + 64, err) ||
        !ensure(nodes, (size_t)(t.P + 1) * 48, err) || !ensure(lkeys, (size_t)t.L * 8 + 16, err))
        return IMLS_ERR_DEVICE;
    char* p = (char*)treescratch.p;
    const TreeScratch ts = tree_scratch(p, t.P);
    float4* mp = (float4*)mpt.p;
    k_fifo_gather<<<grid_for(M), kBlock, 0, s>>>(mkey, mval, M, runs, B, t.L, t.P, fq, clamp, h_clamp, mp, mp + M,
                                                 (unsigned*)(mp + 2 * (size_t)M), (unsigned long long*)lkeys.p, ts.leafbox);
    subtree_rounds(s, ts, t.P, t.levels, (float4*)nodes.p);
    if (int rc = launched("FIFO index launch failed", err)) return rc;
    *P_out = t.P;
    *levels_out = t.levels;
    return IMLS_OK;
}

}  // namespace imlsgpu
