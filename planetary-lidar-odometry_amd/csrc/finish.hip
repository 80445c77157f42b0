// finish.hip — k_finish / k_finish_b: the exact stage, and k_project_lane / k_project_lane_b: the
// exact per-lane search (project.hip's header describes the whole matching step).
#include "exact_stage.h"

namespace imlsgpu {
namespace {

// =============================================================================================
// Exact stage + gates + IMLS (hot kernel 2): one lane per query
// =============================================================================================
// 4 waves/SIMD (≤ 128 VGPRs): the exact stage waits on its gathers, resident waves hide them
#ifndef IMLS_FINISH_WPE
#define IMLS_FINISH_WPE 3
#endif
#define IMLS_FINISH_ATTR __attribute__((amdgpu_waves_per_eu(KL <= 26 ? IMLS_FINISH_WPE : 1)))
template <int KL>
__device__ __forceinline__ void finish_body(TreeView t, const float4* __restrict__ spt,
                                                       const float4* __restrict__ snr,
                                                       const unsigned* __restrict__ qperm, int N,
                                                       const double* __restrict__ pose,
                                                       const int* __restrict__ done, KParams kp,
                                                       const int* __restrict__ lists, const float* __restrict__ wlist,
                                                       float4* __restrict__ cs, float4* __restrict__ cd,
                                                       float4* __restrict__ cn, double* __restrict__ partial1,
                                                       imls_iter_trace* __restrict__ tr,
                                                       unsigned long long* __restrict__ nbr_stats,
                                                       unsigned* __restrict__ fb_list, unsigned* __restrict__ fb_count,
                                                       int bx) {
    if (done && ld_const(done)) return;
    __shared__ double red[kWaveBlock / 64][kNormEq];
    __shared__ double out[kNormEq];
    __shared__ unsigned rej_s[IMLS_NUM_REJ + 3];
    const int tid = threadIdx.x;
    if (tid < IMLS_NUM_REJ + 3) rej_s[tid] = 0;
    __syncthreads();
    const int slot = bx * kWaveBlock + tid;
    const bool active = slot < N;
    const int i = active ? (int)qperm[slot] : 0;
    float xf[3] = {0.f, 0.f, 0.f};
    double ns[3] = {0, 0, 0};
    int cat = -2, kq = 0, i1 = -1, p1 = -1;
    float yf[3] = {0, 0, 0}, nf[3] = {0, 0, 0};
    if (active) {
        // the query's point and normal, then the list (and its bound) beside them: one round trip
        // for both after the query index (the list depends on the slot only)
        const float4 sp4 = spt[i], sn4 = snr[i];
        double ed[KL];
        int ep[KL];
#pragma unroll
        for (int j = 0; j < KL; ++j) ep[j] = lists[(size_t)j * N + slot];
        const float W = wlist[slot];
        transform_query(pose, sp4, sn4, kp.transform_normal, xf, ns);
        const double xd[3] = {xf[0], xf[1], xf[2]};
        // the points in two chunks whose loads all issue before any is consumed (the list's round
        // trip, then two).  The loads are unconditional and pinned (pin_loaded): with
        // `ep ≥ 0 ? exact_d2(…) : ∞` the compiler sank each load into its own branch and waited on
        // it there — 22 dependent round trips per lane, most of this kernel's time
        constexpr int kCh = IMLS_DIST_CHUNK;
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
                if (j < KL) ed[j] = exact_d2(xd, q[u].x, q[u].y, q[u].z) + (ep[j] >= 0 ? 0.0 : kInfD);
            }
        }
        // odd-even transposition sort by (d², index); the fp32 order is already nearly exact.  The
        // index (the filtered index in mpt[].w, libnabo's tie order) is read only for an exact tie
        // of two distances (duplicate points): not carried in registers
        auto oidx = [&](int pos) -> int { return pos >= 0 ? (int)__float_as_uint(t.mpt[pos].w) : 0x7fffffff; };
        bool swapped = true;
        while (swapped) {
            swapped = false;
#pragma unroll
            for (int par = 0; par < 2; ++par) {
#pragma unroll
                for (int j = par; j + 1 < KL; j += 2) {
                    bool sw = ed[j + 1] < ed[j];
                    if (ed[j + 1] == ed[j] && ed[j] < kInfD) sw = oidx(ep[j + 1]) < oidx(ep[j]);
                    const double td = ed[j];
                    const int tp = ep[j];
                    ed[j] = sw ? ed[j + 1] : ed[j];
                    ep[j] = sw ? ep[j + 1] : ep[j];
                    ed[j + 1] = sw ? td : ed[j + 1];
                    ep[j + 1] = sw ? tp : ep[j + 1];
                    swapped |= sw;
                }
            }
        }
        const double r2 = kp.r2;
        const int K = kp.K;
        int cnt_r = 0;
        double d1 = kInfD, dK = 0.0;
#pragma unroll
        for (int j = 0; j < KL; ++j) {
            const bool in = ed[j] <= r2;
            cnt_r += in ? 1 : 0;
            if (in && i1 < 0 && ed[j] > DBL_EPSILON) { d1 = ed[j]; i1 = j; p1 = ep[j]; }
            if (j == K - 1) dK = ed[j];
        }
        const bool full = W < kInfF;
        double need = cnt_r >= K ? dK : r2;
        bool cert = true;
        if (full) {
            // no NN-1 in the list: certified only if no map point within r lies outside it (round 6:
            // before, never — a reused list of an isolated query went to the exact fallback)
            need = i1 < 0 ? r2 : fmax(need, d1);
            cert = cert && (need < (double)W / kCertSlack);
        }
        if (kp.force_fb && slot % kp.force_fb == 0) cert = false;   // test hook (IMLS_OPT_FORCE_FALLBACK)
        if (!cert) {
            // deferred to k_project_lane: listed in slot order in this wave's own region
            // fb_list[w·64, …) (its count in fb_count[w], below) — no atomics, so the fallback's rows
            // (and its slab sums) do not depend on timing
            const unsigned long long dm = __ballot(true);     // the wave's deferring lanes
            const int lanei = tid & 63;
            fb_list[((size_t)bx * kWaveBlock + (tid & ~63)) + __popcll(dm & ((1ull << lanei) - 1ull))] = (unsigned)i;
            cat = -3;
            // the list's own bound for the exact re-run: its points are real, so the exact answer
            // needs no point beyond max(K-th listed key within r, listed NN-1) (r² when either is
            // missing) — the fallback's search ball, instead of the whole radius r
            const double lb = i1 < 0 ? r2 : fmax(cnt_r >= K ? dK : r2, d1);
            cs[i] = make_float4(0.f, 0.f, 0.f, (float)(fmin(lb, r2) * (1.0 + 1e-6)));
        } else {
            cat = kp.matcher ? finish_plane(xf, ns, p1, t, kp, yf, nf)
                             : finish_query<KL, true>(xf, ns, ed, ep, 0, min(K, cnt_r), d1, p1, t, kp, yf, nf, kq, i);
            store_result(i, cat, xf, yf, nf, cs, cd, cn);
        }
    }
    if (cat >= 0) atomicAdd(&rej_s[cat], 1u);
    if (active && cat != -3) {
        if (kq) atomicAdd(&rej_s[IMLS_NUM_REJ], (unsigned)kq);
        if (i1 >= 0) atomicAdd(&rej_s[IMLS_NUM_REJ + 1], 1u);
    }
    if (cat == -3) atomicAdd(&rej_s[IMLS_NUM_REJ + 2], 1u);
    {
        const unsigned long long dm = __ballot(cat == -3);
        if ((tid & 63) == 0) fb_count[bx * (kWaveBlock / 64) + (tid >> 6)] = (unsigned)__popcll(dm);
    }
    __syncthreads();                  // rej_s complete (the slab reduction below may be skipped)
    // pass-1 slabs only for the grid solve chain (frames of ≤ kSmallRows rows: k_solve_small forms
    // pass 1 from the rows); N is block-uniform
    if (N > kSmallRows) {
        double a[6] = {0, 0, 0, 0, 0, 0}, bb = 0.0, one = 0.0;
        if (cat == -1) { plane_row(xf, yf, nf, a, bb); one = 1.0; }
        block_normeq<kWaveBlock>(a, bb, one, red, out);
        if (tid < kNormEq) partial1[(size_t)bx * kNormEq + tid] = out[tid];
    }
    if (tid < IMLS_NUM_REJ && rej_s[tid]) atomicAdd((unsigned long long*)&tr->reject[tid], (unsigned long long)rej_s[tid]);
    if (nbr_stats && tid >= IMLS_NUM_REJ && tid < IMLS_NUM_REJ + 2 && rej_s[tid])
        atomicAdd(&nbr_stats[tid - IMLS_NUM_REJ], (unsigned long long)rej_s[tid]);
    if (nbr_stats && tid == IMLS_NUM_REJ + 2 && rej_s[tid]) atomicAdd(&nbr_stats[5], (unsigned long long)rej_s[tid]);
}

// =============================================================================================
// Per-lane exact traversal (fallback for uncertified queries; IMLS_TRAVERSAL_LANE mode)
// =============================================================================================
template <int KCAP>
__device__ __forceinline__ void project_lane_body(TreeView t, const float4* __restrict__ spt,
                                                             const float4* __restrict__ snr,
                                                             const unsigned* __restrict__ qlist,
                                                             const unsigned* __restrict__ qcount, int N,
                                                             const double* __restrict__ pose,
                                                             const int* __restrict__ done, KParams kp,
                                                             float4* __restrict__ cs, float4* __restrict__ cd,
                                                             float4* __restrict__ cn, double* __restrict__ partial1,
                                                             imls_iter_trace* __restrict__ tr,
                                                             unsigned long long* __restrict__ nbr_stats, int nlog) {
    // (done: the k_finish launch that listed the deferred queries left at once too)
    if (done && ld_const(done)) return;
    __shared__ uint2 stack[kStackDepth][kProjBlock];
    __shared__ double red[kProjBlock / 64][kNormEq];
    __shared__ double out[kNormEq];
    __shared__ unsigned rej_s[IMLS_NUM_REJ + 3];
    const int tid = threadIdx.x;
    if (tid < IMLS_NUM_REJ + 3) rej_s[tid] = 0;
    __syncthreads();
    // nlog logical blocks (one pass-1 slab each) taken by the physical blocks in turn: the slabs do
    // not depend on the physical grid.  A logical block lb works in rounds of kProjBlock queries:
    // every query (lane mode, qlist null) — rows lb·128 + k·nlog·128; deferred queries — the regions
    // k_finish's waves lb, lb + nlog, … listed (qlist[w·64 …], qcount[w] entries each), in wave order
    const int nfb = (N + 63) / 64;
    for (int lb = blockIdx.x; lb < nlog; lb += gridDim.x) {
    double acc_out = 0.0;   // thread tid < 28 accumulates its normal-equation term over rounds
    int fbk = lb, off = 0, base = lb * kProjBlock;
    // deferred queries are rare: the logical block's region counts are read in parallel first, and a
    // block with none writes its zero slab without the region walk (a chain of ~nfb/nlog dependent
    // count loads: ~13 µs per launch on config B with no query deferred)
    bool empty = false;
    if (qlist) {
        int any = 0;
        for (int k = tid; lb + k * nlog < nfb; k += kProjBlock) any |= qcount[lb + k * nlog] != 0u;
        empty = !__syncthreads_or(any);
    }
    for (; !empty;) {
        int q, total;
        size_t at;
        if (qlist) {
            while (fbk < nfb && off >= (int)qcount[fbk]) { fbk += nlog; off = 0; }
            if (fbk >= nfb) break;
            q = off + tid;
            total = (int)qcount[fbk];
            at = (size_t)fbk * 64 + q;
            off += kProjBlock;
        } else {
            if (base >= N) break;
            q = base + tid;
            total = N;
            at = (size_t)q;
            base += nlog * kProjBlock;
        }
        const bool active = q < total;
        const int i = active ? (qlist ? (int)qlist[at] : q) : 0;
        int cat = -2, kq = 0, nn_found = 0;
        float xf[3] = {0, 0, 0}, yf[3] = {0, 0, 0}, nf[3] = {0, 0, 0};
        if (active) {
            double ns[3];
            transform_query(pose, spt[i], snr[i], kp.transform_normal, xf, ns);
            const double xd[3] = {xf[0], xf[1], xf[2]};
            const int K = kp.K;
            double ld[KCAP];
            int li[KCAP];
#pragma unroll
            for (int j = 0; j < KCAP; ++j) {
                const bool sentinel = j < KCAP - K;           // capacity K inside KCAP registers
                ld[j] = sentinel ? -1.0 : kInfD;
                li[j] = sentinel ? -1 : 0x7fffffff;
            }
            double d1 = kInfD;
            int i1 = 0x7fffffff;
            // projected-distance mode (imls_icp.cpp:338-369, 563-596; laser_odometry.cpp:316-341):
            // candidates are the points with ‖p−x‖ < gate_dist and ‖(p−x)×n_s‖ < gate_proj, ranked by
            // the projected distance — the tree only bounds the ‖p−x‖ ball, the list key is proj
            const bool proj = kp.proj != 0;
            const double r2 = proj ? kp.gate_dist * kp.gate_dist : kp.r2;
            // a query deferred by k_finish carries its list's bound in cs[i].w (the search ball cap)
            const double cap = (qlist && !proj) ? fmin(r2, (double)cs[i].w) : r2;
            float bf = (float)cap * kBoxSlack + 1e-30f;
            int node = 1, sp = 0;
            const int P = t.P, B = t.B, M = t.M;
            while (true) {
                if (node < P) {
                    const float4* rec = t.nodes + 3 * (size_t)node;
                    const float4 a = rec[0], b = rec[1], c = rec[2];
                    const float dl = box_d2(xf, a.x, a.y, a.z, a.w, b.x, b.y);
                    const float dr = box_d2(xf, b.z, b.w, c.x, c.y, c.z, c.w);
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
                        const float4 q4 = t.mpt[k];
                        const float ex = q4.x - xf[0], ey = q4.y - xf[1], ez = q4.z - xf[2];
                        const float d32 = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
                        if (d32 > bf) continue;
                        const int oi = (int)__float_as_uint(q4.w);
                        if (proj) {
                            const double dx = (double)q4.x - xd[0], dy = (double)q4.y - xd[1], dz = (double)q4.z - xd[2];
                            const double cx = dy * ns[2] - dz * ns[1], cy = dz * ns[0] - dx * ns[2], cz = dx * ns[1] - dy * ns[0];
                            const double pr = sqrt((cx * cx + cy * cy) + cz * cz);
                            const double dn = sqrt((dx * dx + dy * dy) + dz * dz);
                            if (!(dn < kp.gate_dist && pr < kp.gate_proj)) continue;
                            if (lessp(pr, oi, ld[KCAP - 1], li[KCAP - 1])) {
                                bool prev = true;
#pragma unroll
                                for (int j = KCAP - 1; j >= 0; --j) {
                                    const bool sh = (j > 0) ? lessp(pr, oi, ld[(j > 0) ? j - 1 : 0], li[(j > 0) ? j - 1 : 0]) : false;
                                    const double nd = sh ? ld[(j > 0) ? j - 1 : 0] : (prev ? pr : ld[j]);
                                    const int ni = sh ? li[(j > 0) ? j - 1 : 0] : (prev ? oi : li[j]);
                                    ld[j] = nd;
                                    li[j] = ni;
                                    prev = sh;
                                }
                            }
                            continue;   // fixed bound: every point of the ball is a candidate
                        }
                        const double d2 = exact_d2(xd, q4.x, q4.y, q4.z);
                        if (!(d2 <= r2)) continue;
                        bool changed = false;
                        if (d2 > DBL_EPSILON && lessp(d2, oi, d1, i1)) { d1 = d2; i1 = oi; changed = true; }
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
                            changed = true;
                        }
                        if (changed) bf = (float)fmin(cap, fmax(ld[KCAP - 1], d1)) * kBoxSlack + 1e-30f;
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
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < KCAP; ++j) cnt += (j >= KCAP - K && ld[j] < kInfD) ? 1 : 0;
            if (proj) {
                // NN = the minimum projected distance (min_dist = proj², imls_icp.cpp:585-588); the
                // IMLS list holds proj² as its distances (361-365) — same candidates, same order
                i1 = li[KCAP - K];
                d1 = ld[KCAP - K] * ld[KCAP - K];
#pragma unroll
                for (int j = 0; j < KCAP; ++j) ld[j] = (j >= KCAP - K && ld[j] < kInfD) ? ld[j] * ld[j] : ld[j];
            }
            nn_found = i1 != 0x7fffffff;
            int lpos[KCAP];
#pragma unroll
            for (int j = 0; j < KCAP; ++j) lpos[j] = (li[j] >= 0 && li[j] != 0x7fffffff) ? (int)t.ipos[li[j]] : 0;
            const int p1 = nn_found ? (int)t.ipos[i1] : -1;
            cat = kp.matcher ? finish_plane(xf, ns, p1, t, kp, yf, nf)
                             : finish_query<KCAP>(xf, ns, ld, lpos, KCAP - K, cnt, d1, p1, t, kp, yf, nf, kq, i);
            store_result(i, cat, xf, yf, nf, cs, cd, cn);
        }
        if (cat >= 0) atomicAdd(&rej_s[cat], 1u);
        if (active) {
            if (kq) atomicAdd(&rej_s[IMLS_NUM_REJ], (unsigned)kq);
            if (nn_found) atomicAdd(&rej_s[IMLS_NUM_REJ + 1], 1u);
        }
        if (N > kSmallRows) {           // slabs for the grid solve chain only (see finish_body)
            double a[6] = {0, 0, 0, 0, 0, 0}, bb = 0.0, one = 0.0;
            if (cat == -1) { plane_row(xf, yf, nf, a, bb); one = 1.0; }
            block_normeq<kProjBlock>(a, bb, one, red, out);
            if (tid < kNormEq) acc_out += out[tid];
        }
    }
    if (N > kSmallRows && tid < kNormEq) partial1[(size_t)lb * kNormEq + tid] = acc_out;
    }
    __syncthreads();
    if (tid < IMLS_NUM_REJ && rej_s[tid]) atomicAdd((unsigned long long*)&tr->reject[tid], (unsigned long long)rej_s[tid]);
    if (nbr_stats && tid >= IMLS_NUM_REJ && tid < IMLS_NUM_REJ + 2 && rej_s[tid])
        atomicAdd(&nbr_stats[tid - IMLS_NUM_REJ], (unsigned long long)rej_s[tid]);
}

// ---------------------------------------------------------------------------------------------
// Kernels: one frame (arguments by value) and batched (frame = tab[blockIdx.y]; blocks past the
// frame's own grid leave at once).  Both run the same bodies.
// ---------------------------------------------------------------------------------------------
template <int KL>
__global__ __launch_bounds__(kWaveBlock) IMLS_FINISH_ATTR void k_finish(
        TreeView t, const float4* __restrict__ spt, const float4* __restrict__ snr, const unsigned* __restrict__ qperm,
        int N, const double* __restrict__ pose, const int* __restrict__ done, KParams kp, const int* __restrict__ lists,
        const float* __restrict__ wlist, float4* __restrict__ cs, float4* __restrict__ cd, float4* __restrict__ cn,
        double* __restrict__ partial1, imls_iter_trace* __restrict__ tr, unsigned long long* __restrict__ nbr_stats,
        unsigned* __restrict__ fb_list, unsigned* __restrict__ fb_count) {
    finish_body<KL>(t, spt, snr, qperm, N, pose, done, kp, lists, wlist, cs, cd, cn, partial1, tr, nbr_stats, fb_list,
                    fb_count, (int)blockIdx.x);
}

template <int KCAP>
__global__ __launch_bounds__(kProjBlock) void k_project_lane(
        TreeView t, const float4* __restrict__ spt, const float4* __restrict__ snr, const unsigned* __restrict__ qlist,
        const unsigned* __restrict__ qcount, int N, const double* __restrict__ pose, const int* __restrict__ done,
        KParams kp, float4* __restrict__ cs, float4* __restrict__ cd, float4* __restrict__ cn,
        double* __restrict__ partial1, imls_iter_trace* __restrict__ tr, unsigned long long* __restrict__ nbr_stats) {
    project_lane_body<KCAP>(t, spt, snr, qlist, qcount, N, pose, done, kp, cs, cd, cn, partial1, tr, nbr_stats,
                            kFallbackBlocks);
}

template <int KL>
__global__ __launch_bounds__(kWaveBlock) IMLS_FINISH_ATTR void k_finish_b(const PairDev* __restrict__ tab, KParams kp,
                                                                           int it, int npairs) {
    int f, bx;
    batch_block(kp.xcd, f, bx);
    if (f >= npairs) return;
    const PairDev A = device_view(tab + f);
    if (bx >= finish_blocks_of(A.N)) return;
    finish_body<KL>(A.t, A.spt, A.snr, A.qperm, A.N, A.st.pose, A.st.done, kp, A.lists, list_block(A.lists, A.N, KL).wlist, A.cs,
                    A.cd, A.cn, A.st.partial1, A.trace + it, A.stats, A.fb_list, A.fb_count, bx);
}

template <int KCAP>
__global__ __launch_bounds__(kProjBlock) void k_project_lane_b(const PairDev* __restrict__ tab, KParams kp, int it) {
    const PairDev A = device_view(tab + blockIdx.y);
    project_lane_body<KCAP>(A.t, A.spt, A.snr, A.fb_list, A.fb_count, A.N, A.st.pose, A.st.done, kp, A.cs, A.cd, A.cn,
                            A.st.partial1 + (size_t)finish_blocks_of(A.N) * kNormEq, A.trace + it, A.stats,
                            kFallbackBlocks);
}

}  // namespace

void launch_finish(hipStream_t s, const ProjectLaunch& L) {
    with_list_sizes(L.kp.K, [&](auto z) {
        constexpr int KL = decltype(z)::KL;
        k_finish<KL><<<finish_blocks_of(L.N), kWaveBlock, 0, s>>>(L.t, L.spt, L.snr, L.qperm, L.N, L.pose, L.done, L.kp, L.lists,
                                                                  list_block(L.lists, L.N, KL).wlist, L.cs, L.cd, L.cn,
                                                                  L.partial1, L.tr, L.stats, L.fb_list, L.fb_count);
    });
}

void launch_finish_batch(hipStream_t s, dim3 grid, const PairDev* tab, const KParams& kp, int it, int npairs) {
    with_list_sizes(kp.K, [&](auto z) {
        k_finish_b<decltype(z)::KL><<<grid, kWaveBlock, 0, s>>>(tab, kp, it, npairs);
    });
}

void launch_lane(hipStream_t s, const ProjectLaunch& L, bool deferred) {
    double* p_fb = L.partial1 + (size_t)finish_blocks_of(L.N) * kNormEq;
    with_list_sizes(L.kp.K, [&](auto z) {
        k_project_lane<decltype(z)::KCAP><<<kFallbackBlocks, kProjBlock, 0, s>>>(
            L.t, L.spt, L.snr, deferred ? L.fb_list : nullptr, deferred ? L.fb_count : nullptr, L.N, L.pose, L.done, L.kp, L.cs,
            L.cd, L.cn, p_fb, L.tr, L.stats);
    });
}

void launch_lane_batch(hipStream_t s, dim3 grid, const PairDev* tab, const KParams& kp, int it) {
    with_list_sizes(kp.K, [&](auto z) {
        k_project_lane_b<decltype(z)::KCAP><<<grid, kProjBlock, 0, s>>>(tab, kp, it);
    });
}

}  // namespace imlsgpu
