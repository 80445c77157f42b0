// knn_export.hip — the public kNN query's own kernels (k_knn_prep, k_knn_export, k_knn_export_lane)
// and its launch sequence over the traversals of knn_wave.hip / knn_qwave.hip.
#include "project_common.h"

namespace imlsgpu {
namespace {

// =============================================================================================
// Public kNN query (imls_knn): the neighbours themselves — libnabo NNSearchD::knn with epsilon 0 and
// SORT_RESULTS (imls_icp.cpp:197, 372, 414, 605, 650; laser_odometry.cpp:348).  Stage 1 is the
// traversal (knn_wave.hip / knn_qwave.hip) at the identity pose; k_knn_export is finish_body up to its certificate, then
// the acceptance rule and the rows; k_knn_export_lane is project_lane_body's neighbour heap alone.
// Kernels of their own: k_finish / k_project_lane are not touched (nor their register budgets).
// =============================================================================================
// the traversal's radius for an unbounded query (max_radius = +∞): the fp32 search bound
// (1 + skin)²·r²·kBoxSlack must stay finite — an infinite bound would meet the slot-id keys' finite
// sentinels and inf − inf box tests — and this is beyond any squared distance of points whose fp32
// keys do not overflow (coordinates up to ~1e18).  Only the search is clamped: the acceptance rule
// and the certificate below keep the caller's r², so a query that needs more than the clamped ball
// (fewer than K points in it) is simply uncertified and re-run by the exact per-lane search.
constexpr double kKnnR2Max = 1e37;

__global__ __launch_bounds__(kBlock) void k_knn_prep(const float* __restrict__ src, size_t pstride, size_t cstride, int n,
                                                     const float* __restrict__ qp, float4* __restrict__ qpt,
                                                     double* __restrict__ pose) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 16) pose[threadIdx.x] = (threadIdx.x % 5 == 0) ? 1.0 : 0.0;
    if (i >= n) return;
    const float* p = src + (size_t)i * pstride;
    const float x = p[0], y = p[cstride], z = p[2 * cstride];
    const bool ok = isfinite(x) && isfinite(y) && isfinite(z);
    // a non-finite query never reaches the tree: parked at the target's box corner, flagged in w
    qpt[i] = ok ? make_float4(x, y, z, 0.f) : make_float4(qp[0], qp[1], qp[2], 1.f);
}

// One query's output row.  The lanes of a wave hold Morton-consecutive queries, whose rows lie
// anywhere in the caller's [nq][K] arrays (qperm), so staging a wave's rows through LDS would
// gain no coalescing; instead each lane stores its own contiguous row (4·K and 8·K bytes) as
// 16-byte vectors — ⌈K/4⌉ + ⌈K/2⌉ stores instead of 2·K scalar ones — whenever the rows are 16-B
// aligned (vec bit 0: the index rows, K % 4 == 0; bit 1: the d² rows, K % 2 == 0; both need an
// aligned base: launch_knn), element stores otherwise.  Entries at and past cnt must already
// hold (−1, +∞).
template <int CAP>
__device__ __forceinline__ void knn_store_row(const int (&oi)[CAP], const double (&od)[CAP], int K, int cnt, size_t i,
                                              int vec, int32_t* __restrict__ idx_out, double* __restrict__ d2_out,
                                              int32_t* __restrict__ found_out) {
    int32_t* const ri = idx_out + i * (size_t)K;
    double* const rd = d2_out + i * (size_t)K;
    if (vec & 1) {
#pragma unroll
        for (int j = 0; j + 3 < CAP; j += 4)
            if (j < K) *reinterpret_cast<int4*>(ri + j) = make_int4(oi[j], oi[j + 1], oi[j + 2], oi[j + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < CAP; ++j)
            if (j < K) ri[j] = oi[j];
    }
    if (vec & 2) {
#pragma unroll
        for (int j = 0; j + 1 < CAP; j += 2)
            if (j < K) *reinterpret_cast<double2*>(rd + j) = make_double2(od[j], od[j + 1]);
    } else {
#pragma unroll
        for (int j = 0; j < CAP; ++j)
            if (j < K) rd[j] = od[j];
    }
    if (found_out) found_out[i] = min(cnt, K);
}

// entries moved down by `by` places (the vacated tail: +∞ / none), by the bits of `by`
template <int CAP>
__device__ __forceinline__ void knn_shift_down(double (&d)[CAP], int (&o)[CAP], int by) {
#pragma unroll
    for (int bi = 0; (1 << bi) < CAP; ++bi) {
        const bool s = (by >> bi) & 1;
#pragma unroll
        for (int j = 0; j < CAP; ++j) {
            d[j] = s ? (j + (1 << bi) < CAP ? d[j + (1 << bi) < CAP ? j + (1 << bi) : 0] : kInfD) : d[j];
            o[j] = s ? (j + (1 << bi) < CAP ? o[j + (1 << bi) < CAP ? j + (1 << bi) : 0] : 0x7fffffff) : o[j];
        }
    }
}

template <int KL>
__global__ __launch_bounds__(kWaveBlock) void k_knn_export(
        TreeView t, const float4* __restrict__ qpt, const unsigned* __restrict__ qperm, int N, KnnArgs a, double r2_search,
        const int* __restrict__ lists, const float* __restrict__ wlist, float* __restrict__ caps,
        unsigned* __restrict__ fb_list, unsigned* __restrict__ fb_count, int32_t* __restrict__ idx_out,
        double* __restrict__ d2_out, int32_t* __restrict__ found_out, int vec) {
    const int tid = threadIdx.x, bx = (int)blockIdx.x;
    const int slot = bx * kWaveBlock + tid;
    const bool active = slot < N;
    bool defer = false;
    int i = 0;
    float cap = 0.f;
    if (active) {
        i = (int)qperm[slot];
        const float4 q4 = qpt[i];
        const bool bad = q4.w != 0.f;       // non-finite query: every slot unfound
        const double xd[3] = {q4.x, q4.y, q4.z};
        // the list → exact distances and FILTERED indices (mpt[].w, libnabo's column index): no
        // later stage needs the positions, so the index rides along instead of being re-read on ties
        double ed[KL];
        int eo[KL];
        const float W = wlist[slot];
        {
            int ep[KL];
#pragma unroll
            for (int j = 0; j < KL; ++j) ep[j] = lists[(size_t)j * N + slot];
            // chunked, pinned gathers as in finish_body: a chunk's loads all issue before any is consumed
            constexpr int kCh = 12;
#pragma unroll
            for (int j0 = 0; j0 < KL; j0 += kCh) {
                float4 q[kCh];
#pragma unroll
                for (int u = 0; u < kCh; ++u)
                    if (j0 + u < KL) q[u] = t.mpt[max(ep[j0 + u], 0)];
#pragma unroll
                for (int u = 0; u < kCh; ++u)
                    if (j0 + u < KL) pin_loaded(q[u]);
#pragma unroll
                for (int u = 0; u < kCh; ++u) {
                    const int j = j0 + u;
                    if (j < KL) {
                        ed[j] = exact_d2(xd, q[u].x, q[u].y, q[u].z) + (ep[j] >= 0 ? 0.0 : kInfD);
                        eo[j] = ep[j] >= 0 ? (int)__float_as_uint(q[u].w) : 0x7fffffff;
                    }
                }
            }
        }
        // odd-even transposition sort by the total order (d², filtered index)
        bool swapped = true;
        while (swapped) {
            swapped = false;
#pragma unroll
            for (int par = 0; par < 2; ++par) {
#pragma unroll
                for (int j = par; j + 1 < KL; j += 2) {
                    const bool sw = lessp(ed[j + 1], eo[j + 1], ed[j], eo[j]);
                    const double td = ed[j];
                    const int to = eo[j];
                    ed[j] = sw ? ed[j + 1] : ed[j];
                    eo[j] = sw ? eo[j + 1] : eo[j];
                    ed[j + 1] = sw ? td : ed[j + 1];
                    eo[j + 1] = sw ? to : eo[j + 1];
                    swapped |= sw;
                }
            }
        }
        // acceptance: d² ≤ r² and (ALLOW_SELF_MATCH or d² > DBL_EPSILON).  In the sorted list the
        // self matches are a prefix and the entries beyond r² (or missing) a suffix: the accepted
        // ones are [first, first + cnt)
        const int K = a.K;
        int first = 0, cnt = 0;
#pragma unroll
        for (int j = 0; j < KL; ++j) {
            const bool real = eo[j] != 0x7fffffff;
            const bool self = !a.allow_self && ed[j] <= DBL_EPSILON;
            first += (real && self) ? 1 : 0;
            cnt += (real && !self && ed[j] <= a.r2) ? 1 : 0;
        }
        if (__ballot(first != 0)) knn_shift_down<KL>(ed, eo, first);
        // certificate, on ACCEPTED entries (a query on more than KL − K duplicates of itself has
        // fewer than K accepted entries in a full list and must not return them as its answer):
        // every map point outside a full list has d² ≥ W/(1 + 3.1e-7) (finish_body), outside a
        // partial one lies beyond the searched ball (≥ r2_search) — so the answer is exact iff the
        // largest distance it relies on, the K-th accepted d² or r² when fewer are accepted, is
        // below that
        double dK = 0.0;
#pragma unroll
        for (int j = 0; j < KL; ++j) dK = (j == K - 1) ? ed[j] : dK;
        const double need = cnt >= K ? dK : a.r2;
        const bool full = W < kInfF;
        bool cert = full ? need < (double)W / kCertSlack : need <= r2_search;
        if (a.force_fb && slot % a.force_fb == 0) cert = false;   // test hook (IMLS_OPT_FORCE_FALLBACK)
        if (bad) { cert = true; cnt = 0; }
        defer = !cert;
        // the list's points are real: the exact answer needs none beyond `need` (the fallback's ball)
        cap = (float)(fmin(need, a.r2) * (1.0 + 1e-6));
        if (cert) {
#pragma unroll
            for (int j = 0; j < KL; ++j) {
                ed[j] = j < cnt ? ed[j] : kInfD;
                eo[j] = j < cnt ? eo[j] : -1;
            }
            knn_store_row<KL>(eo, ed, K, cnt, (size_t)i, vec, idx_out, d2_out, found_out);
        }
    }
    // deferred to k_knn_export_lane in slot order in the wave's own region of fb_list (its count in
    // fb_count[wave]): the layout of finish_body — no atomics, nothing depends on timing
    const unsigned long long dm = __ballot(defer);
    const int lanei = tid & 63, w = bx * (kWaveBlock / 64) + (tid >> 6);
    if (defer) {
        fb_list[(size_t)w * 64 + __popcll(dm & ((1ull << lanei) - 1ull))] = (unsigned)i;
        caps[i] = cap;
    }
    if (lanei == 0 && w < (N + 63) / 64) fb_count[w] = (unsigned)__popcll(dm);
}

// The exact per-lane search (project_lane_body's heap alone): the queries k_knn_export deferred
// (qlist / qcount: region w holds qcount[w] ≤ 64 queries, one wave takes a region at a time), or
// every query in qperm order (qlist null: IMLS_TRAVERSAL_LANE).
template <int KCAP>
__global__ __launch_bounds__(kProjBlock) void k_knn_export_lane(
        TreeView t, const float4* __restrict__ qpt, const unsigned* __restrict__ qperm, const unsigned* __restrict__ qlist,
        const unsigned* __restrict__ qcount, const float* __restrict__ caps, int N, KnnArgs a,
        int32_t* __restrict__ idx_out, double* __restrict__ d2_out, int32_t* __restrict__ found_out, int vec) {
    __shared__ uint2 stack[kStackDepth][kProjBlock];
    const int tid = threadIdx.x, lane = tid & 63;
    const int nwaves = (int)gridDim.x * (kProjBlock / 64), nreg = (N + 63) / 64;
    const int K = a.K;
    for (int reg = (int)blockIdx.x * (kProjBlock / 64) + (tid >> 6); reg < nreg; reg += nwaves) {
        const int q = reg * 64 + lane;
        const bool active = qlist ? lane < (int)qcount[reg] : q < N;
        if (!active) continue;
        const int i = (int)(qlist ? qlist[q] : qperm[q]);
        const float4 q4 = qpt[i];
        double ld[KCAP];
        int li[KCAP];
#pragma unroll
        for (int j = 0; j < KCAP; ++j) {
            const bool sentinel = j < KCAP - K;               // capacity K inside KCAP registers
            ld[j] = sentinel ? -1.0 : kInfD;
            li[j] = sentinel ? -1 : 0x7fffffff;
        }
        int cnt = 0;
        if (q4.w == 0.f) {                  // (a non-finite query: every slot unfound)
            const float xf[3] = {q4.x, q4.y, q4.z};
            const double xd[3] = {q4.x, q4.y, q4.z};
            const double r2 = a.r2;
            const double cap = qlist ? fmin(r2, (double)caps[i]) : r2;
            float bf = (float)cap * kBoxSlack + 1e-30f;
            int node = 1, sp = 0;
            const int P = t.P, B = t.B, M = t.M;
            while (true) {
                if (node < P) {
                    const float4* rec = t.nodes + 3 * (size_t)node;
                    const float4 ra = rec[0], rb = rec[1], rc = rec[2];
                    const float dl = box_d2(xf, ra.x, ra.y, ra.z, ra.w, rb.x, rb.y);
                    const float dr = box_d2(xf, rb.z, rb.w, rc.x, rc.y, rc.z, rc.w);
                    const bool vl = dl <= bf, vr = dr <= bf;
                    if (vl && vr) {
                        const bool lfirst = dl <= dr;
                        stack[sp][tid] = make_uint2(lfirst ? 2 * node + 1 : 2 * node, __float_as_uint(lfirst ? dr : dl));
                        ++sp;
                        node = lfirst ? 2 * node : 2 * node + 1;
                        continue;
                    }
                    node = vl ? 2 * node : (vr ? 2 * node + 1 : 0);
                    if (node) continue;
                } else {
                    const int s0 = (node - P) * B, e0 = min(s0 + B, M);
                    for (int k = s0; k < e0; ++k) {
                        const float4 p4 = t.mpt[k];
                        const float ex = p4.x - xf[0], ey = p4.y - xf[1], ez = p4.z - xf[2];
                        const float d32 = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
                        if (d32 > bf) continue;
                        const int oi = (int)__float_as_uint(p4.w);
                        const double d2 = exact_d2(xd, p4.x, p4.y, p4.z);
                        if (!(d2 <= r2 && (a.allow_self || d2 > DBL_EPSILON))) continue;
                        if (lessp(d2, oi, ld[KCAP - 1], li[KCAP - 1])) {
                            bool prev = true;
#pragma unroll
                            for (int j = KCAP - 1; j >= 0; --j) {
                                const bool sh = (j > 0) ? lessp(d2, oi, ld[(j > 0) ? j - 1 : 0], li[(j > 0) ? j - 1 : 0]) : false;
                                const double nd = sh ? ld[(j > 0) ? j - 1 : 0] : (prev ? d2 : ld[j]);
                                const int ni = sh ? li[(j > 0) ? j - 1 : 0] : (prev ? oi : li[j]);
                                ld[j] = nd;
                                li[j] = ni;
                                prev = sh;
                            }
                            bf = (float)fmin(cap, ld[KCAP - 1]) * kBoxSlack + 1e-30f;
                        }
                    }
                    node = 0;
                }
                while (sp > 0) {
                    --sp;
                    const uint2 e = stack[sp][tid];
                    if (__uint_as_float(e.y) <= bf) { node = (int)e.x; break; }
                }
                if (!node) break;
            }
#pragma unroll
            for (int j = 0; j < KCAP; ++j) cnt += (j >= KCAP - K && ld[j] < kInfD) ? 1 : 0;
        }
        knn_shift_down<KCAP>(ld, li, KCAP - K);               // (wave-uniform) the K live slots first
#pragma unroll
        for (int j = 0; j < KCAP; ++j) {
            ld[j] = j < cnt ? ld[j] : kInfD;
            li[j] = j < cnt ? li[j] : -1;
        }
        knn_store_row<KCAP>(li, ld, K, cnt, (size_t)i, vec, idx_out, d2_out, found_out);
    }
}

}  // namespace

void knn_prepare(hipStream_t s, const TreeView& t, const float* src, size_t pstride, size_t cstride, int n, float4* qpt,
                 double* pose) {
    k_knn_prep<<<(n + kBlock - 1) / kBlock, kBlock, 0, s>>>(src, pstride, cstride, n, t.qparams, qpt, pose);
}

void launch_knn(hipStream_t s, const TreeView& t, const float4* qpt, const unsigned* qperm, int n, const double* pose,
                const KnnArgs& a, int lane_mode, int* lists, unsigned* fb_list, unsigned* fb_count, int32_t* idx_out,
                double* d2_out, int32_t* found_out) {
    // 16-byte row stores where every row is 16-B aligned (knn_store_row)
    const int K = a.K;
    const int vec = (((uintptr_t)idx_out % 16 == 0 && K % 4 == 0) ? 1 : 0) | (((uintptr_t)d2_out % 16 == 0 && K % 2 == 0) ? 2 : 0);
    const int regions = (n + 63) / 64;
    const int lane_blocks = std::max(1, std::min((regions + kProjBlock / 64 - 1) / (kProjBlock / 64), 2048));
    // the traversal as a projection launch: K, the (clamped) radius, the traversal choice; the
    // plane_ICP matcher value only switches off the wave-per-query kernel's h-gate search (an IMLS
    // gate: a query with nothing within h would be left an empty list); no done flag, no reuse, no
    // temporal seed, no counters
    ProjectLaunch L{};
    L.t = t;
    L.spt = qpt;
    L.qperm = qperm;
    L.N = n;
    L.pose = pose;
    L.lists = lists;
    L.kp.K = K;
    L.kp.r2 = std::min(a.r2, kKnnR2Max);
    L.kp.h2 = L.kp.r2;
    L.kp.matcher = IMLS_MATCH_PLANE_ICP;
    L.kp.qwave = a.qwave;
    L.kp.packet = 64;
    if (!lane_mode) {
        if (use_qwave(L.kp, n)) launch_knn_qwave(s, L, false);
        else launch_knn_wave(s, L);
    }
    with_list_sizes(K, [&](auto z) {
        constexpr int KL = decltype(z)::KL, KCAP = decltype(z)::KCAP;
        const ListBlock lb = list_block(lists, n, KL);
        if (!lane_mode)
            k_knn_export<KL><<<(n + kWaveBlock - 1) / kWaveBlock, kWaveBlock, 0, s>>>(
                t, qpt, qperm, n, a, L.kp.r2, lb.pos, lb.wlist, lb.caps, fb_list, fb_count, idx_out, d2_out, found_out, vec);
        // the deferred queries, or every query (lane mode)
        k_knn_export_lane<KCAP><<<lane_blocks, kProjBlock, 0, s>>>(t, qpt, qperm, lane_mode ? nullptr : fb_list,
                                                                   lane_mode ? nullptr : fb_count, lb.caps, n, a, idx_out,
                                                                   d2_out, found_out, vec);
    });
}

}  // namespace imlsgpu
