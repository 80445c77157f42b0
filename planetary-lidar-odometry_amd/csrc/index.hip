// index.hip — per-frame spatial index of the target map (replaces the libnabo kd-tree built by
// IMLSICPMatcher::setTargetPointCloud, imls_icp.cpp:80-103) and the source's query order.
//
// Build = filtered points (filter.hip) → bbox → 48-bit Morton keys → radix sort (key, filtered
//       index) → Morton-ordered float4 points → B-point buckets as the leaves of an implicit
//       complete binary tree of AABBs.  Lone (one frame), small (one launch) and batched (many
//       frames, one launch sequence); the steps' bodies are index_common.h's.
// All kernels are HBM-streaming: coalesced float loads, float4 stores.
#include <hipcub/hipcub.hpp>

#include "index_common.h"

namespace imlsgpu {

// PairSort (index_common.h): the one place hipcub's radix sort is instantiated
PairSort::PairSort(int n_, int end_bit_, hipStream_t s) : n(n_), end_bit(end_bit_) {
    hipcub::DoubleBuffer<unsigned long long> kq(nullptr, nullptr);
    hipcub::DoubleBuffer<unsigned> vq(nullptr, nullptr);
    hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, kq, vq, std::max(n, 1), kMortonSortLo, end_bit, s);
}
void PairSort::run(hipStream_t s) {
    hipcub::DoubleBuffer<unsigned long long> kb(k0, k1);
    hipcub::DoubleBuffer<unsigned> vb(v0, v1);
    hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, kb, vb, n, kMortonSortLo, end_bit, s);
    k0 = kb.Current();
    v0 = vb.Current();
}

namespace {

__global__ void k_bbox_partial(const float4* __restrict__ pt, int M, float* __restrict__ part) {
    __shared__ float red[6][kBlock];
    Box bx = box_empty();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x) box_add(bx, pt[i]);
    block_box<kBlock>(bx, red);
    if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = red[threadIdx.x][0];
}

// the points' bbox from the block partials → their quantisation
__global__ void k_bbox_final(const float* __restrict__ part, int nparts, float* __restrict__ qp) {
    __shared__ float red[6][kBlock];
    block_box_of_parts<kBlock>(part, nparts, red);
    if (threadIdx.x == 0) box_quantisation(red[0][0], red[1][0], red[2][0], red[3][0], red[4][0], red[5][0], qp);
}

__global__ void k_morton(const float4* __restrict__ pt, int M, const float* __restrict__ qp,
                         unsigned long long* __restrict__ key, unsigned* __restrict__ val) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    float4 p = pt[i];
    key[i] = morton48(p.x, p.y, p.z, qp);
    val[i] = (unsigned)i;
}

__global__ void k_leaf_keys(const unsigned long long* __restrict__ sorted, int M, int B, unsigned long long* __restrict__ lk) {
    int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l * B < M) lk[l] = sorted[(size_t)l * B];
}

// Morton-ordered copies: mpt (xyz + original index), mnr (normals), and ipos (original → Morton)
__global__ void k_gather(const float4* __restrict__ pt, const float4* __restrict__ nr, const unsigned* __restrict__ perm,
                         int M, float4* __restrict__ mpt, float4* __restrict__ mnr, unsigned* __restrict__ ipos) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= M) return;
    unsigned j = perm[k];
    float4 p = pt[j];
    mpt[k] = make_float4(p.x, p.y, p.z, __uint_as_float(j));
    mnr[k] = nr[j];
    ipos[j] = (unsigned)k;
}

// leaf boxes: one thread per bucket b < P; buckets ≥ L are empty
__global__ void k_leaf_boxes(const float4* __restrict__ mpt, int M, int B, int P, float* __restrict__ leafbox) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P) return;
    leaf_box_body(mpt, M, B, b, leafbox);
}

__global__ void k_subtree(const float* __restrict__ in, int count, int D, float4* __restrict__ nodes, float* __restrict__ roots) {
    subtree_body(in, min(count, kBlock), D, nodes, roots);
}

// Permutation (sorted → input index) of n float4 points by 48-bit Morton code over their bbox.
// With lkeys: also the first key of each B-point leaf and the quantisation (seed search).
// *perm_out = the buffer holding the permutation — perm's own storage when the caller needs it there
// (no perm_out: one device copy if the sort left it in scratch), else possibly scratch.
// qp_fixed: a quantisation given by the caller (device, [4]) instead of the points' own bbox — the
// kNN queries are keyed in the target's frame (query_order).
int morton_perm(hipStream_t s, const float4* pts, int n, DevBuf& scratch, DevBuf& perm, std::string& err,
                DevBuf* lkeys = nullptr, int B = 0, const unsigned** perm_out = nullptr, const float* qp_fixed = nullptr) {
    PairSort sort(n, 48, s);
    const int bb_parts = 512;
    const size_t need = sort.bytes(true) + carve_bytes<float>(bb_parts * 6) + carve_bytes<float>(4);
    if (!ensure(scratch, need, err) || !ensure(perm, (size_t)n * 4 + 16, err)) return IMLS_ERR_DEVICE;
    char* p = (char*)scratch.p;
    sort.carve_from(p, (unsigned*)perm.p);       // perm's own storage is the second value buffer
    float* bbpart = carve<float>(p, bb_parts * 6);
    const float* qp = carve<float>(p, 4);
    const int L = B > 0 ? (n + B - 1) / B : 0;
    if (lkeys && !ensure(*lkeys, (size_t)L * 8 + 16, err)) return IMLS_ERR_DEVICE;
    if (lkeys) qp = (float*)((unsigned long long*)lkeys->p + L);   // qparams live after the keys
    if (qp_fixed) {
        qp = qp_fixed;
    } else {
        const int nb = bbox_partials(s, pts, n, bb_parts, bbpart);
        k_bbox_final<<<1, kBlock, 0, s>>>(bbpart, nb, const_cast<float*>(qp));
    }
    k_morton<<<grid_for(n), kBlock, 0, s>>>(pts, n, qp, sort.k0, sort.v0);
    sort.run(s);
    if (lkeys) k_leaf_keys<<<grid_for(L), kBlock, 0, s>>>(sort.k0, n, B, (unsigned long long*)lkeys->p);
    if (perm_out) {
        *perm_out = sort.v0;
    } else if (sort.v0 != (unsigned*)perm.p) {
        (void)hipMemcpyAsync(perm.p, sort.v0, (size_t)n * 4, hipMemcpyDeviceToDevice, s);
    }
    return launched("morton sort launch failed", err);
}

}  // namespace

int bbox_partials(hipStream_t s, const float4* pts, int n, int parts, float* part) {
    const int nb = std::min(parts, (int)grid_for(n));
    k_bbox_partial<<<nb, kBlock, 0, s>>>(pts, n, part);
    return nb;
}

void subtree_rounds(hipStream_t s, const TreeScratch& t, int P, int levels, float4* nodes) {
    SubRound r[kSubRounds];
    const int rounds = subtree_plan(t, P, levels, r);   // ≤ 3 < kSubRounds: tree_shape refused deeper trees
    for (int k = 0; k < rounds; ++k)
        k_subtree<<<subtree_blocks(r[k].count), kBlock, 0, s>>>(r[k].in, r[k].count, r[k].D, nodes, r[k].out);
}

int build_target_tree(hipStream_t s, int M, int bucket, DevBuf& lkeys, DevBuf& tpt, DevBuf& tnr, DevBuf& mpt,
                      DevBuf& nodes, DevBuf& scratch, DevBuf& treescratch, DevBuf& permbuf, int* P_out, int* levels_out,
                      std::string& err) {
    if (M <= 0) { *P_out = 0; *levels_out = 0; return IMLS_OK; }
    const int B = bucket;
    TreeShape t;
    if (int rc = tree_shape(M, B, t, err)) return rc;
    const unsigned* perm = nullptr;
    if (int rc = morton_perm(s, (const float4*)tpt.p, M, scratch, permbuf, err, &lkeys, B, &perm)) return rc;
    if (!ensure(treescratch, tree_scratch_bytes(t.P), err) || !ensure(mpt, (size_t)M * 36 + 64, err) ||
        !ensure(nodes, (size_t)(t.P + 1) * 48, err))
        return IMLS_ERR_DEVICE;
    char* p = (char*)treescratch.p;
    const TreeScratch ts = tree_scratch(p, t.P);
    k_gather<<<grid_for(M), kBlock, 0, s>>>((const float4*)tpt.p, (const float4*)tnr.p, perm, M,
                                            (float4*)mpt.p, (float4*)mpt.p + M, (unsigned*)((float4*)mpt.p + 2 * (size_t)M));
    k_leaf_boxes<<<grid_for(t.P), kBlock, 0, s>>>((const float4*)mpt.p, M, B, t.P, ts.leafbox);
    subtree_rounds(s, ts, t.P, t.levels, (float4*)nodes.p);
    if (int rc = launched("index build launch failed", err)) return rc;
    *P_out = t.P;
    *levels_out = t.levels;
    return IMLS_OK;
}

namespace {
// The source order of a small frame (≤ kSmallOrderN points) in ONE launch: the bbox and quantisation
// (k_bbox_partial / k_bbox_final's bodies), the 48-bit Morton keys, and a bitonic sort of (key,
// index) in LDS — the permutation the stable radix sort gives (equal keys keep index order), where
// morton_perm / the batched build take 6-8 launches (a lone frame's critical path: the source is
// ordered after its filter's count arrives, before the first traversal)
__global__ __launch_bounds__(kSmallOrderN / 2) void k_small_order(const float4* __restrict__ pt, int n,
                                                                unsigned* __restrict__ perm) {
    constexpr int T = kSmallOrderN / 2;
    __shared__ unsigned long long sk[kSmallOrderN];
    __shared__ unsigned sv[kSmallOrderN];
    __shared__ float red[6][T];
    __shared__ float qp[4];
    const int t = threadIdx.x;
    Box bx = box_empty();
    float4 p[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int i = t + u * T;
        p[u] = i < n ? pt[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < n) box_add(bx, p[u]);
    }
    block_box<T>(bx, red);
    if (t == 0) box_quantisation(red[0][0], red[1][0], red[2][0], red[3][0], red[4][0], red[5][0], qp);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int i = t + u * T;
        sk[i] = i < n ? morton48(p[u].x, p[u].y, p[u].z, qp) : ~0ull;
        sv[i] = i < n ? (unsigned)i : ~0u;
    }
    __syncthreads();
    for (int size = 2; size <= kSmallOrderN; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i + stride;
            const unsigned long long ki = sk[i], kj = sk[j];
            const unsigned vi = sv[i], vj = sv[j];
            const bool gt = ki > kj || (ki == kj && vi > vj);
            if (gt == ((i & size) == 0)) { sk[i] = kj; sk[j] = ki; sv[i] = vj; sv[j] = vi; }
            __syncthreads();
        }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int i = t + u * T;
        if (i < n) perm[i] = sv[i];
    }
}
}  // namespace

int small_source_order(hipStream_t s, const float4* pts, int N, unsigned* perm, std::string& err) {
    if (N <= 0) return IMLS_OK;
    if (N > kSmallOrderN) { err = "small source order: too many points"; return IMLS_ERR_CAPACITY; }
    k_small_order<<<1, kSmallOrderN / 2, 0, s>>>(pts, N, perm);
    return launched("source order launch failed", err);
}

int source_order(hipStream_t s, int N, DevBuf& spt, DevBuf& scratch, DevBuf& qperm, std::string& err) {
    if (N <= 0) return IMLS_OK;
    if (N <= kSmallOrderN) {
        if (!ensure(qperm, (size_t)N * 4 + 16, err)) return IMLS_ERR_DEVICE;
        return small_source_order(s, (const float4*)spt.p, N, (unsigned*)qperm.p, err);
    }
    return morton_perm(s, (const float4*)spt.p, N, scratch, qperm, err);
}

// The kNN queries' order (imls_knn): the source path's keys and sort under the TARGET's quantisation
// qp (TreeView::qparams) — a query outside the target's box clamps to its border instead of
// stretching a box of the queries' own, so a few far queries do not cost the others their coherence.
int query_order(hipStream_t s, const float4* pts, int n, const float* qp, DevBuf& scratch, DevBuf& perm, std::string& err) {
    if (n <= 0) return IMLS_OK;
    return morton_perm(s, pts, n, scratch, perm, err, nullptr, 0, nullptr, qp);
}

// ---------------------------------------------------------------------------------------------
// Batched builds (imls_register_frames): the target trees and source orders of many frames in one
// launch sequence — per-frame bbox partials, Morton keys with the job index above bit 48 (one radix
// sort orders every frame's points at once; stable, so each frame's permutation is exactly its own
// sort's), the Morton-ordered copies / leaf keys / permutations, leaf boxes and the subtree rounds.
// Every step computes what the per-frame build computes, in the same float operations: the bodies
// are the lone kernels'.
// ---------------------------------------------------------------------------------------------
namespace {

constexpr int kBBoxParts = 64;          // bbox partial blocks per job (grid-stride)

struct JobDev {
    const float4* pts;                  // filtered points (xyz, 0)
    const float4* nrm;                  // filtered normals (targets)
    int n, off;                         // points; offset in the concatenated key array
    int B, P;                           // targets: bucket, padded leaves (B = 0: source)
    float* qp;                          // [4] quantisation (targets: after the leaf keys)
    unsigned long long* lkeys;          // targets: first key of each leaf
    float4 *mpt, *mnr;                  // targets: Morton-ordered copies
    unsigned* ipos;                     // targets: input → Morton position
    float4* nodes;                      // targets: node records
    unsigned* perm;                     // sources: sorted → input index
    float* bbpart;                      // [kBBoxParts × 6]
    float* leafbox;                     // targets: [P × 6]
    SubRound sub[kSubRounds];           // targets: the subtree rounds (count ≤ 1: past the job's last)
};

__global__ __launch_bounds__(kBlock) void k_bbox_b(const JobDev* __restrict__ jobs) {
    const JobDev& J = jobs[blockIdx.y];
    __shared__ float red[6][kBlock];
    const int M = J.n;
    const int nb = min(kBBoxParts, (int)((M + kBlock - 1) / kBlock));
    if ((int)blockIdx.x >= nb) return;
    Box bx = box_empty();
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < M; i += nb * kBlock) box_add(bx, J.pts[i]);
    block_box<kBlock>(bx, red);
    if (threadIdx.x < 6) J.bbpart[blockIdx.x * 6 + threadIdx.x] = red[threadIdx.x][0];
}

// bbox (min / max are exact in any order) → quantisation, one wave per job
__global__ __launch_bounds__(64) void k_qparams_b(const JobDev* __restrict__ jobs) {
    const JobDev& J = jobs[blockIdx.x];
    const int M = J.n;
    if (M <= 0) return;
    const int nb = min(kBBoxParts, (int)((M + kBlock - 1) / kBlock));
    const int t = threadIdx.x;
    float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (t < nb)
        for (int d = 0; d < 3; ++d) { b[d] = J.bbpart[t * 6 + d]; b[3 + d] = J.bbpart[t * 6 + 3 + d]; }
    for (int o = 32; o > 0; o >>= 1)
        for (int d = 0; d < 3; ++d) {
            b[d] = fminf(b[d], __shfl_xor(b[d], o, 64));
            b[3 + d] = fmaxf(b[3 + d], __shfl_xor(b[3 + d], o, 64));
        }
    if (t == 0) box_quantisation(b[0], b[1], b[2], b[3], b[4], b[5], J.qp);
}

// keys tagged with the job index above bit 48
__global__ __launch_bounds__(kBlock) void k_morton_b(const JobDev* __restrict__ jobs, unsigned long long* __restrict__ key,
                                                     unsigned* __restrict__ val) {
    const JobDev& J = jobs[blockIdx.y];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= J.n) return;
    const float4 p = J.pts[i];
    key[(size_t)J.off + i] = ((unsigned long long)blockIdx.y << 48) | morton48(p.x, p.y, p.z, J.qp);
    val[(size_t)J.off + i] = (unsigned)i;
}

// sorted segment of a job → targets: Morton copies, input → Morton positions, leaf first keys;
// sources: the permutation
__global__ __launch_bounds__(kBlock) void k_place_b(const JobDev* __restrict__ jobs, const unsigned long long* __restrict__ key,
                                                    const unsigned* __restrict__ val) {
    const JobDev& J = jobs[blockIdx.y];
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= J.n) return;
    const unsigned j = val[(size_t)J.off + k];
    if (J.B == 0) {
        J.perm[k] = j;
        return;
    }
    const float4 p = J.pts[j];
    J.mpt[k] = make_float4(p.x, p.y, p.z, __uint_as_float(j));
    J.mnr[k] = J.nrm[j];
    J.ipos[j] = (unsigned)k;
    if (k % J.B == 0) J.lkeys[k / J.B] = key[(size_t)J.off + k] & 0xFFFFFFFFFFFFull;
}

__global__ __launch_bounds__(kBlock) void k_leaf_boxes_b(const JobDev* __restrict__ jobs) {
    const JobDev& J = jobs[blockIdx.y];
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (J.B == 0 || b >= J.P) return;
    leaf_box_body(J.mpt, J.n, J.B, b, J.leafbox);
}

// subtree round r of every job (a job past its last round leaves)
__global__ __launch_bounds__(kBlock) void k_subtree_b(const JobDev* __restrict__ jobs, int r) {
    const JobDev& J = jobs[blockIdx.y];
    if (J.B == 0) return;
    const SubRound& R = J.sub[r];
    const int count = R.count;
    if (count <= 1) return;
    const int width = min(count, kBlock);
    if ((int)blockIdx.x >= count / width) return;
    subtree_body(R.in, width, R.D, J.nodes, R.out);
}

}  // namespace

size_t build_job_bytes() { return sizeof(JobDev); }

int build_batch(hipStream_t s, std::vector<BuildJob>& jobs, DevBuf& scratch, DevBuf& table, void* h_table,
                size_t h_table_bytes, std::string& err) {
    const int nj = (int)jobs.size();
    if (nj == 0) return IMLS_OK;
    if ((size_t)nj * sizeof(JobDev) > h_table_bytes) { err = "build table too small"; return IMLS_ERR_CAPACITY; }
    if (nj > 65535) { err = "too many build jobs"; return IMLS_ERR_CAPACITY; }
    size_t total = 0, job_bytes = 0;
    int maxn = 1, maxP = 1;
    for (auto& b : jobs) {
        job_bytes += carve_bytes<float>(kBBoxParts * 6) + carve_bytes<float>(4);
        if (b.n <= 0) continue;
        total += (size_t)b.n;
        maxn = std::max(maxn, b.n);
        if (b.B > 0) {
            TreeShape t;
            if (int rc = tree_shape(b.n, b.B, t, err)) return rc;
            b.P = t.P;
            b.levels = t.levels;
            maxP = std::max(maxP, t.P);
            job_bytes += tree_scratch_bytes(t.P);
        }
    }
    int end_bit = 48;
    while ((1ll << (end_bit - 48)) < nj) ++end_bit;
    PairSort sort((int)total, end_bit, s);
    if (!ensure(scratch, sort.bytes() + job_bytes, err) || !ensure(table, (size_t)nj * sizeof(JobDev) + 256, err))
        return IMLS_ERR_DEVICE;
    char* p = (char*)scratch.p;
    sort.carve_from(p);
    JobDev* J = (JobDev*)h_table;
    size_t off = 0;
    for (int q = 0; q < nj; ++q) {
        const BuildJob& b = jobs[q];
        JobDev d{};
        d.pts = b.pts;
        d.nrm = b.nrm;
        d.n = std::max(b.n, 0);
        d.off = (int)off;
        off += (size_t)d.n;
        d.bbpart = carve<float>(p, kBBoxParts * 6);
        if (b.B > 0 && b.n > 0) {
            d.B = b.B;
            d.P = b.P;
            d.lkeys = b.lkeys;
            d.qp = (float*)(b.lkeys + (b.n + b.B - 1) / b.B);   // the quantisation lives after the leaf keys
            d.mpt = b.mpt;
            d.mnr = b.mpt + b.n;
            d.ipos = (unsigned*)(b.mpt + 2 * (size_t)b.n);
            d.nodes = b.nodes;
            const TreeScratch ts = tree_scratch(p, b.P);
            d.leafbox = ts.leafbox;
            if (subtree_plan(ts, b.P, b.levels, d.sub) < 0) { err = "tree too deep for the batched build"; return IMLS_ERR_CAPACITY; }
        } else {
            d.B = 0;
            d.qp = carve<float>(p, 4);
            d.perm = b.perm;
        }
        J[q] = d;
    }
    const JobDev* jd = (const JobDev*)table.p;
    hipMemcpyAsync(table.p, h_table, (size_t)nj * sizeof(JobDev), hipMemcpyHostToDevice, s);
    const unsigned gx = grid_for((size_t)maxn);
    k_bbox_b<<<dim3(std::min<unsigned>(kBBoxParts, gx), nj), kBlock, 0, s>>>(jd);
    k_qparams_b<<<nj, 64, 0, s>>>(jd);
    k_morton_b<<<dim3(gx, nj), kBlock, 0, s>>>(jd, sort.k0, sort.v0);
    if (total > 0) sort.run(s);
    k_place_b<<<dim3(gx, nj), kBlock, 0, s>>>(jd, sort.k0, sort.v0);
    bool any_tree = false;
    for (auto& b : jobs) any_tree |= b.B > 0 && b.n > 0;
    if (any_tree) {
        k_leaf_boxes_b<<<dim3(grid_for((size_t)maxP), nj), kBlock, 0, s>>>(jd);
        // the grid of round r is the largest tree's; a smaller job's surplus blocks leave
        for (int r = 0, cnt = maxP; r < kSubRounds && cnt > 1; ++r, cnt = subtree_blocks(cnt))
            k_subtree_b<<<dim3(subtree_blocks(cnt), nj), kBlock, 0, s>>>(jd, r);
    }
    return launched("batched index build launch failed", err);
}

}  // namespace imlsgpu
