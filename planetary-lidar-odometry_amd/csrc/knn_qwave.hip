// knn_qwave.hip — k_knn_qwave / k_knn_qwave_f / k_knn_qwave_b: the wave-per-query traversal and the
// exact stage fused behind it (project.hip's header describes the whole matching step).
#include "exact_stage.h"

namespace imlsgpu {
namespace {

#ifdef IMLS_DEBUG_WAVE_TRACE
// diagnostic build: per-wave records of the last fused launch (tools/qwave_dump.py), 16 u32 per wave
__device__ unsigned g_dbg_qwave[kDbgWaves][16];
#endif

// =============================================================================================
// Exact stage, one WAVE per query (a small frame registered alone — the config C/D deployment
// shape, ≤ kSmallRows queries — where k_finish's one-lane-per-query latency chain (~30 µs per
// launch for 2000 queries in 8 blocks) sets the frame latency): lane j holds list entry j, so the
// gathers, the exact distances, the gates and the IMLS weights run across the lanes.  Every value is
// computed by the same expression as k_finish's lane code, the list order is the same (d², index)
// total order (each lane's rank by counting), the IMLS sums accumulate in that order (lane 0 reads
// each term in turn) — the correspondences are the lane kernel's bit for bit.  Rejects are counted
// by integer atomics (order-free).  No pass-1 slabs: frames of ≤ kSmallRows rows are solved by
// k_solve_small, which forms pass 1 from the rows (the same order for every small frame, batched
// or alone, whichever exact stage produced its rows).
// =============================================================================================
__device__ __forceinline__ double rl_f64(double x, int l) {
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readlane((int)(unsigned)(b & 0xffffffffll), l);
    const int hi = __builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

__device__ __forceinline__ double shfl_up_f64(double x) {
    const long long b = __double_as_longlong(x);
    const int lo = __shfl_up((int)(unsigned)(b & 0xffffffffll), 1, 64);
    const int hi = __shfl_up((int)(unsigned)((unsigned long long)b >> 32), 1, 64);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// The exact list of one query by one wave, for a query whose float list failed its certificate
// (round 4: the fused lone-frame path resolves it in place instead of deferring it to the fallback
// launch): project_lane_body's search — the K nearest map points by (exact d², original index) with
// d² ≤ r², NN-1 = the first with d² > DBL_EPSILON, boxes and points pruned by the float bound
// min(cap, max(K-th, NN-1))·slack — with the list in lanes 0..K−1 instead of registers.  Returns
// lane k's entry position (−1 empty); an NN-1 outside the K entries (more than K points within
// DBL_EPSILON of the query) rides in lane K.  stk_n / stk_d: the wave's LDS stack (kWaveStack).
template <int KL>
__device__ int exact_wave_list(const TreeView& t, const KParams& kp, const double xd[3], const float xf[3], double cap,
                               int* stk_n, float* stk_d) {
    static_assert(KL <= 64, "one list entry per lane");
    const int lane = threadIdx.x & 63;
    const int K = kp.K;
    const double r2 = kp.r2;
    double ek = kInfD;
    int eo = 0x7fffffff, ep = -1;
    double d1 = kInfD;
    int o1 = 0x7fffffff, p1 = -1;
    float bf = (float)cap * kBoxSlack + 1e-30f;
    const int P = t.P, B = t.B, M = t.M;
    int node = 1, sp = 0;
    while (true) {
        if (node < P) {
            const int lev = 31 - __builtin_clz(node);
            const int sw = min(kWide, t.levels - lev);
            const int nk = 1 << sw;
            float d = kInfF;
            if (lane < nk) {
                const float4* rec = t.nodes + 3 * (((size_t)node << (sw - 1)) + (lane >> 1));
                const float4 a = rec[0], b = rec[1], c = rec[2];
                d = (lane & 1) ? box_d2(xf, b.z, b.w, c.x, c.y, c.z, c.w) : box_d2(xf, a.x, a.y, a.z, a.w, b.x, b.y);
            }
            const unsigned long long want = __ballot(lane < nk && d <= bf);
            if (want) {
                const int km = __builtin_ctzll(want);
                unsigned long long rest = want & (want - 1);
                while (rest) {
                    const int kk = 63 - __builtin_clzll(rest);
                    rest &= ~(1ull << kk);
                    const float dk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), kk));
                    if (lane == 0) { stk_n[sp] = (node << sw) + kk; stk_d[sp] = dk; }
                    ++sp;
                }
                node = (node << sw) + km;
                continue;
            }
        } else {
            const int base = (node - P) * B, cnt = min(B, M - base);
            double d2 = kInfD;
            int oi = 0x7fffffff;
            bool c = false;
            if (lane < cnt) {
                const float4 q = t.mpt[base + lane];
                const float ex = q.x - xf[0], ey = q.y - xf[1], ez = q.z - xf[2];
                const float d32 = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
                if (d32 <= bf) {
                    d2 = exact_d2(xd, q.x, q.y, q.z);
                    oi = (int)__float_as_uint(q.w);
                    c = d2 <= r2;
                }
            }
            unsigned long long m = __ballot(c);
            while (m) {
                const int j = __builtin_ctzll(m);
                m &= m - 1;
                const double cdd = rl_f64(d2, j);
                const int co = __builtin_amdgcn_readlane(oi, j);
                bool changed = false;
                if (cdd > DBL_EPSILON && (cdd < d1 || (cdd == d1 && co < o1))) {
                    d1 = cdd; o1 = co; p1 = base + j;
                    changed = true;
                }
                const double wk = rl_f64(ek, K - 1);
                const int wo = __builtin_amdgcn_readlane(eo, K - 1);
                if (cdd < wk || (cdd == wk && co < wo)) {
                    const int at = __popcll(__ballot(lane < K && (ek < cdd || (ek == cdd && eo < co))));
                    const double uk = shfl_up_f64(ek);
                    const int uo = __shfl_up(eo, 1, 64), up = __shfl_up(ep, 1, 64);
                    if (lane > at && lane < K) { ek = uk; eo = uo; ep = up; }
                    if (lane == at) { ek = cdd; eo = co; ep = base + j; }
                    changed = true;
                }
                if (changed) bf = (float)fmin(cap, fmax(rl_f64(ek, K - 1), d1)) * kBoxSlack + 1e-30f;
            }
        }
        node = 0;
        while (sp > 0) {
            --sp;
            if (stk_d[sp] <= bf) { node = stk_n[sp]; break; }
        }
        if (!node) break;
    }
    if (p1 >= 0 && !__ballot(lane < K && ep == p1) && lane == K) ep = p1;
    return lane <= K ? ep : -1;
}

// query i (slot `slot`) from its list: lane k < KL holds entry k's map position `pos` (−1 empty),
// W is the list's bound (the traversal's worst key).  Run by k_knn_qwave_f straight after the
// traversal of the same wave (round 4: one launch per iteration fewer); an uncertified query gets its
// exact list in place (exact_wave_list, with the wave's LDS stack stk_n / stk_d) — nothing is deferred.
template <int KL>
__device__ __forceinline__ void finish_q_core(TreeView t, const float4* __restrict__ spt, const float4* __restrict__ snr,
                                              int i, int slot, const double* __restrict__ pose, const KParams& kp,
                                              int pos, float W, float4* __restrict__ cs, float4* __restrict__ cd,
                                              float4* __restrict__ cn, imls_iter_trace* __restrict__ tr,
                                              unsigned long long* __restrict__ nbr_stats, int* stk_n, float* stk_d) {
    static_assert(KL <= 64, "one list entry per lane");
    const int lane = threadIdx.x & 63;
    float xf[3];
    double ns[3];
    transform_query(pose, spt[i], snr[i], kp.transform_normal, xf, ns);
    const double xd[3] = {xf[0], xf[1], xf[2]};
    const bool ent = lane < KL;
    const double r2 = kp.r2;
    const int K = kp.K;
    float4 q;
    double ed, d1, dK;
    int eo, rank, cnt_r, l1, p1, lK;
    bool in;
    auto lane_of_rank = [&](int r) -> int {
        const unsigned long long m = __ballot(ent && rank == r);
        return m ? (int)__builtin_ctzll(m) : -1;
    };
    // the list's exact keys, its (d², index) order (k_finish's sort; empty entries after the real
    // ones, by lane), the count within r, the NN-1 and the K-th
    auto analyse = [&]() {
        q = make_float4(0.f, 0.f, 0.f, 0.f);
        ed = kInfD;
        eo = 0x7fffffff;
        if (pos >= 0) {
            q = t.mpt[pos];
            ed = exact_d2(xd, q.x, q.y, q.z);
            eo = (int)__float_as_uint(q.w);
        }
        rank = 0;
#pragma unroll
        for (int k = 0; k < KL; ++k) {
            const double dk = rl_f64(ed, k);
            const int ok = __builtin_amdgcn_readlane(eo, k);
            rank += (dk < ed || (dk == ed && (ok < eo || (ok == eo && k < lane)))) ? 1 : 0;
        }
        in = ent && ed <= r2;
        cnt_r = __popcll(__ballot(in));
        // NN-1: the first entry in order within r with d² > DBL_EPSILON (no self match)
        int r1 = (in && ed > DBL_EPSILON) ? rank : 0x7fffffff;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) r1 = min(r1, __shfl_xor(r1, o, 64));
        l1 = r1 < 0x7fffffff ? lane_of_rank(r1) : -1;
        d1 = l1 >= 0 ? rl_f64(ed, l1) : kInfD;
        p1 = l1 >= 0 ? __builtin_amdgcn_readlane(pos, l1) : -1;
        lK = lane_of_rank(K - 1);
        dK = lK >= 0 ? rl_f64(ed, lK) : 0.0;
    };
    analyse();
    const bool full = W < kInfF;
    double need = cnt_r >= K ? dK : r2;
    bool cert = true;
    if (full) {
        // no NN-1 in the list: certified only if no map point within r lies outside it (round 6:
        // before, never — a reused list of an isolated query went to the exact fallback)
        need = l1 < 0 ? r2 : fmax(need, d1);
        cert = cert && (need < (double)W / kCertSlack);
    }
    if (kp.force_fb && slot % kp.force_fb == 0) cert = false;   // test hook (IMLS_OPT_FORCE_FALLBACK)
    int cat = -1, kq = 0;
    float yf[3] = {0.f, 0.f, 0.f}, nf[3] = {0.f, 0.f, 0.f};
    if (!cert) {
        // the exact search ball: the list's bound (its points are real, the exact answer needs
        // nothing farther — the bound k_project_lane gets from k_finish through cs.w)
        const double lb = l1 < 0 ? r2 : fmax(cnt_r >= K ? dK : r2, d1);
        const float capf = (float)(fmin(lb, r2) * (1.0 + 1e-6));
        pos = exact_wave_list<KL>(t, kp, xd, xf, fmin(r2, (double)capf), stk_n, stk_d);
        analyse();
        if (nbr_stats && lane == 0) atomicAdd(&nbr_stats[5], 1ull);
    }
    if (kp.matcher) {
        cat = finish_plane(xf, ns, p1, t, kp, yf, nf);
    } else {
        // finish_query, entry j of the ordered list = the lane of rank j
        const int cnt = min(K, cnt_r);
        double nn[3] = {0.0, 0.0, 0.0};
        if (p1 < 0 || d1 > kp.h2) {
            cat = IMLS_REJ_TOO_FAR;                             // imls_icp.cpp:612-625 (Q18)
        } else if (kp.tv) {
            const double4 v = t.tvn[i];
            if (v.w == 0.0) cat = IMLS_REJ_NO_NORMAL;
            nn[0] = v.x; nn[1] = v.y; nn[2] = v.z;
        } else if (!kp.get_normals) {
            cat = IMLS_REJ_INVALID_NORMAL;
        } else {
            const float4 n4 = t.mnr[p1];
            nn[0] = n4.x; nn[1] = n4.y; nn[2] = n4.z;
        }
        if (cat == -1 && !(isfinite(nn[0]) && isfinite(nn[1]) && isfinite(nn[2]))) cat = IMLS_REJ_INVALID_NORMAL;
        if (cat == -1 && kp.angle_on && angle_reject(ns, nn[0], nn[1], nn[2], kp.angle_thr_deg, kp.cos_thr))
            cat = IMLS_REJ_NORMAL_CONSTRAINT;
        if (cat == -1) {
            const bool inl = ent && rank < cnt;
            kq = cnt;
            float4 qn = make_float4(0.f, 0.f, 0.f, 0.f);
            if (inl) qn = t.mnr[pos];
            bool ok = inl && kp.get_normals && isfinite(qn.x) && isfinite(qn.y) && isfinite(qn.z);
            if (ok && kp.angle_on) ok = !angle_reject(ns, qn.x, qn.y, qn.z, kp.angle_thr_deg, kp.cos_thr);
            const unsigned long long accm = __ballot(ok);
            const int nacc = __popcll(accm);
            if (nacc < 3) {
                cat = IMLS_REJ_MLS_FAIL;                        // imls_icp.cpp:463-466
            } else {
                const int lt = lane_of_rank(nacc - 1);          // Q3: L[|S| − 1]
                const double hmax = sqrt(rl_f64(ed, lt)) / 3;
                const double ih2 = 1.0 / (hmax * hmax);          // as finish_query
                double w = 0.0, pr = 0.0;
                if (ok) {
                    const double dx = xd[0] - (double)q.x, dy = xd[1] - (double)q.y, dz = xd[2] - (double)q.z;
                    double dn = dx * dx;
                    dn = dn + dy * dy;
                    dn = dn + dz * dz;
                    w = exp(-dn * ih2);
                    pr = (w * dx) * (double)qn.x;
                    pr = pr + (w * dy) * (double)qn.y;
                    pr = pr + (w * dz) * (double)qn.z;
                }
                // Σ in list order, as the lane code accumulates
                double wsum = 0.0, psum = 0.0;
                for (int r = 0; r < cnt; ++r) {
                    const int l = lane_of_rank(r);
                    if ((accm >> l) & 1ull) {
                        wsum += rl_f64(w, l);
                        psum += rl_f64(pr, l);
                    }
                }
                const double height = psum / (wsum + 1e-5);     // Q4
                if (isnan(height) || isinf(height)) {
                    cat = IMLS_REJ_NAN_INF_HEIGHT;
                } else {
                    yf[0] = (float)(xd[0] - height * nn[0]);    // imls_icp.cpp:719-729
                    yf[1] = (float)(xd[1] - height * nn[1]);
                    yf[2] = (float)(xd[2] - height * nn[2]);
                    nf[0] = (float)nn[0]; nf[1] = (float)nn[1]; nf[2] = (float)nn[2];
                }
            }
        }
    }
    if (lane == 0) {
        store_result(i, cat, xf, yf, nf, cs, cd, cn);
        if (cat >= 0) atomicAdd((unsigned long long*)&tr->reject[cat], 1ull);   // integer: order-free
        if (nbr_stats) {
            if (kq) atomicAdd(&nbr_stats[0], (unsigned long long)kq);
            if (l1 >= 0) atomicAdd(&nbr_stats[1], 1ull);
        }
    }
}

// =============================================================================================
// One wave per query (sparse query sets, e.g. FPS-sampled scans of the config-C stream): no packet
// union — each query walks only its own neighbourhood — and the top-KL list is spread over the
// lanes (lane k holds entry k, sorted), so every step is wave-uniform: inner nodes are scalar
// loads, a leaf is one coalesced load with one point per lane, an insertion is a ballot + shuffle.
// Output contract identical to k_knn_wave (positions [KL][N], worst key W per query).
// =============================================================================================
// FUSED (k_knn_qwave_f, a small frame alone): the wave goes on to the exact stage of its query
// (finish_q_core) with the list still in its lanes, an uncertified list resolved in the same wave
// (exact_wave_list) — nothing is deferred.  Extra arguments unused otherwise.
template <int KL, bool FUSED = false>
__device__ __forceinline__ void knn_qwave_body(TreeView t, const float4* __restrict__ spt,
                                                          const unsigned* __restrict__ qperm, int N,
                                                          const double* __restrict__ pose,
                                                          const int* __restrict__ done, KParams kp,
                                                          const double* __restrict__ delta,
                                                          int* __restrict__ lists, float* __restrict__ wlist,
                                                          float4* __restrict__ xref, float* __restrict__ nref,
                                                          int use_prev, unsigned long long* __restrict__ nbr_stats,
                                                          int bx, const QFinishArgs& fa = QFinishArgs{}) {
    static_assert(KL <= 64, "one list entry per lane");
    if (done && ld_const(done)) return;
    __shared__ int snode[kWaveBlock / 64][kWaveStack];
    __shared__ float sdist[kWaveBlock / 64][kWaveStack];
    __shared__ int fnode[kWaveBlock / 64][kFStack];      // frontier traversal
    __shared__ float fdist[kWaveBlock / 64][kFStack];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slot = __builtin_amdgcn_readfirstlane(bx * (kWaveBlock / 64) + wv);
    if (slot >= N) return;
#ifdef IMLS_DEBUG_WAVE_TRACE
    const long long dbg_q0 = wall_clock64();
#endif
    float xf[3];
    {
        double ns[3];
        transform_query(pose, spt[qperm[slot]], make_float4(0.f, 0.f, 0.f, 0.f), 0, xf, ns);
    }
    float lkey = kInfF;     // lane k < KL: entry k of the ascending list
    int lpos = -1;
    const float r2s = (float)(kp.r2 * kSearchR2) * kBoxSlack + 1e-30f;   // the search bound (radius (1 + skin)·r)
    // h-gate search (IMLS matcher): a query with no map point within h is rejected as too far
    // whatever lies between h and r (imls_icp.cpp:612-625), so while the list holds nothing within
    // h the traversal bound is h², not r² (27× less volume for isolated queries, the launch's tail);
    // a point found within h re-runs the traversal at the r bound (bounds never grow mid-walk)
    const float h2s = (float)kp.h2 * kBoxSlack + 1e-30f;
    bool hmode = false;
    float bnd = r2s;
    const int P = t.P, B = t.B, M = t.M;
    // insert (c, cp): entries ordered by (key, position); the tail shifts up by one lane
    auto insert = [&](float c, int cp) {
        const unsigned long long before = __ballot(lane < KL && (lkey < c || (lkey == c && lpos < cp)));
        const int at = __popcll(before);
        const float uk = __shfl_up(lkey, 1, 64);
        const int up = __shfl_up(lpos, 1, 64);
        if (lane > at && lane < KL) { lkey = uk; lpos = up; }
        if (lane == at) { lkey = c; lpos = cp; }
        bnd = fminf(hmode ? h2s : r2s, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lkey), KL - 1)));
    };
    auto worst = [&]() { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lkey), KL - 1)); };
    int seed_lo = 0, seed_hi = -1, seed_leaf = -1;
    bool greedy = !use_prev;
    bool skip = false;
    float wskip = kInfF;
    if (use_prev) {
        double rf = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double e = ld_const(delta + r * 4 + c) - (r == c ? 1.0 : 0.0);
                rf += e * e;
            }
        const double d3 = ld_const(delta + 3), d7 = ld_const(delta + 7), d11 = ld_const(delta + 11);
        const float tn = (float)sqrt(d3 * d3 + d7 * d7 + d11 * d11);
        const float disp = tn + (float)sqrt(rf) * sqrtf(xf[0] * xf[0] + xf[1] * xf[1] + xf[2] * xf[2]);
        greedy = disp * disp > kReseed * wlist[slot];
    }
    float wlow = -1.0f;
    if (!greedy && kp.reuse) skip = verlet_skip(xref[slot], nref[slot], xf, r2s, wskip, wlow);
    if (skip) {
        // the list stays in place
    } else if (!greedy) {
        // prefill: previous list re-measured at the new pose.  Its ≤ KL distinct points all fit, so
        // inserting them one by one (the list empty, the bound r² until the last) leaves exactly
        // those within r² in (key, position) order: a bitonic sort of the lanes gives that order in
        // log²(KL)/2 exchange steps instead of KL dependent insertions (the re-traversing waves that
        // set a steady iteration's launch time all start here)
        const int pos = lane < KL ? lists[(size_t)lane * N + slot] : -1;
        float d = kInfF;
        if (pos >= 0) {
            const float4 q = t.mpt[pos];
            const float ex = q.x - xf[0], ey = q.y - xf[1], ez = q.z - xf[2];
            d = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
        }
        const bool in = pos >= 0 && d <= bnd;
        float sk = in ? d : kInfF;
        int sp = in ? pos : -1;
        constexpr int W = KL <= 32 ? 32 : 64;
#pragma unroll
        for (int size = 2; size <= W; size <<= 1) {
#pragma unroll
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                const float ok = __shfl_xor(sk, stride, 64);
                const int op = __shfl_xor(sp, stride, 64);
                const bool asc = (lane & size) == 0, low = (lane & stride) == 0;
                const bool other_less = ok < sk || (ok == sk && op < sp);
                const bool other_more = sk < ok || (sk == ok && sp < op);
                if (asc == low ? other_less : other_more) { sk = ok; sp = op; }
            }
        }
        if (lane < KL) { lkey = sk; lpos = sp; }
        bnd = fminf(r2s, worst());
    } else {
        // seed: the leaf of the query's own Morton key ± seed_half Morton neighbours
        const unsigned long long qk = morton48(xf[0], xf[1], xf[2], t.qparams);
        int lo = 0, hi = t.L - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (t.lkeys[mid] <= qk) lo = mid;
            else hi = mid - 1;
        }
        seed_lo = max(0, lo - kSeedHalf);
        seed_hi = min(t.L - 1, lo + kSeedHalf);
        seed_leaf = lo;
        for (int leaf = seed_lo; leaf <= seed_hi; ++leaf) {
            const int base = leaf * B, cnt = min(B, M - base);
            float d = kInfF;
            if (lane < cnt) {
                const float4 q = t.mpt[base + lane];
                const float ex = q.x - xf[0], ey = q.y - xf[1], ez = q.z - xf[2];
                d = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
            }
            unsigned long long m = __ballot(lane < cnt && d <= bnd);
            while (m) {
                const int j = __builtin_ctzll(m);
                m &= m - 1;
                const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), j));
                if (c <= bnd && c < worst()) insert(c, base + j);
            }
        }
    }
    unsigned n_inner = 0, n_leaf = 0;
    if (nbr_stats && lane == 0 && skip) atomicAdd(&nbr_stats[kStatSkipped], 1ull);
    auto nearest = [&]() { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(lkey))); };
    if (!skip && kp.matcher == IMLS_MATCH_IMLS && !(nearest() <= h2s)) {
        hmode = true;
        bnd = fminf(bnd, h2s);
    }
    for (int pass = 0; pass < 2; ++pass) {
    int node = 0, sp = 0;
    if (!skip) {
        // bottom-up start (round 4): the start leaf — the query's Morton leaf (greedy) or the leaf of
        // its nearest listed point — and the boxes of the siblings along its root path in ONE
        // parallel load (lane k: the sibling of the leaf's ancestor k levels up; a node's box sits in
        // its parent's record).  The leaf and those siblings' subtrees partition the tree, so every
        // sibling within the bound is stacked (nearest level on top) and the walk begins at the leaf:
        // the same leaves are reachable as from the root, without the ⌈levels/3⌉ dependent descent
        const int p0 = __builtin_amdgcn_readfirstlane(lpos);
        const int sl = greedy ? seed_leaf : (p0 >= 0 ? p0 / B : -1);
        node = 1;
        if (sl >= 0) {
            const int ln = P + sl;
            float d = kInfF;
            int sn = 0;
            if (lane < t.levels) {
                sn = (ln >> lane) ^ 1;
                const float4* rec = t.nodes + 3 * (size_t)(sn >> 1);
                const float4 a = rec[0], b = rec[1], c = rec[2];
                d = (sn & 1) ? box_d2(xf, b.z, b.w, c.x, c.y, c.z, c.w) : box_d2(xf, a.x, a.y, a.z, a.w, b.x, b.y);
            }
            const unsigned long long want = __ballot(lane < t.levels && d <= bnd * kBoxSlack);
            if ((want >> lane) & 1ull) {
                const int at = __popcll(want >> (lane + 1));
                snode[wv][at] = sn;
                sdist[wv][at] = d;
            }
            sp = __popcll(want);
            node = ln;
        }
    }
    if (node) {
        // Frontier traversal (round 4): each step takes up to 8 stacked entries within the bound and
        // gives each an 8-lane group — an inner node's group tests the boxes of its descendants
        // `sw` levels down (one record per lane pair), a leaf's group measures its points (B / 8 per
        // lane) — so a query whose ball spans many leaves walks them 8 at a time instead of one
        // dependent step per node (the steady-state iterations' tail: 2 % of the queries, 5-10
        // leaves and 11-16 inner steps each, set the launch time).  Candidates are inserted before
        // the wanted children are stacked (lower lanes on top), so the bound they face is current.
        // The same nodes are pruned by the same test (box d² > bound·slack, the bound only shrinks):
        // exactness is the DFS's.  Near capacity (> kFBatchMax entries) one entry per step keeps the
        // growth to the DFS's depth × 7.
        if (lane < sp) { fnode[wv][lane] = snode[wv][lane]; fdist[wv][lane] = sdist[wv][lane]; }
        if (lane == 0) { fnode[wv][sp] = node; fdist[wv][sp] = 0.0f; }
        int fsp = sp + 1;
        const int ppl = (B + 7) >> 3;
#ifdef IMLS_DEBUG_WAVE_TRACE
        int dbg_steps = 0;
#endif
        while (fsp > 0) {
#ifdef IMLS_DEBUG_WAVE_TRACE
            if (++dbg_steps > 20000 || fsp > kFStack) {
                if (lane == 0)
                    printf("frontier stuck: slot %d pass %d steps %d fsp %d sp0 %d node0 %d bnd %g P %d levels %d B %d M %d\n",
                           slot, pass, dbg_steps, fsp, sp, node, (double)bnd, P, t.levels, B, M);
                break;
            }
#endif
            const int lim = fsp > kFBatchMax ? 1 : 8;
            const int idx = fsp - 1 - lane;
            int en = 0;
            float ed = kInfF;
            if (idx >= 0) { en = fnode[wv][idx]; ed = fdist[wv][idx]; }
            const unsigned long long vm = __ballot(idx >= 0 && ed <= bnd * kBoxSlack);
            unsigned long long rem = vm, taken = 0;
            int gsrc[8];
            int ng = 0;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                gsrc[g] = 0;
                if (g < lim && rem) {
                    const int b = __builtin_ctzll(rem);
                    gsrc[g] = b;
                    taken |= 1ull << b;
                    rem &= rem - 1;
                    ++ng;
                }
            }
            fsp -= (ng == lim) ? (64 - __builtin_clzll(taken)) : min(fsp, 64);
            if (!ng) continue;
            const int g = lane >> 3, gl = lane & 7;
            int src = gsrc[0];
#pragma unroll
            for (int k = 1; k < 8; ++k) src = g == k ? gsrc[k] : src;
            const int gnode = __shfl(en, src, 64);
            const bool gact = g < ng;
            const bool ginner = gact && gnode < P, gleaf = gact && gnode >= P;
            n_inner += __popcll(__ballot(ginner && gl == 0));
            n_leaf += __popcll(__ballot(gleaf && gl == 0));
            // every lane's loads of the step issue together — its node record (inner groups) and its
            // B / 8 leaf points (leaf groups) — from clamped addresses, the values selected after:
            // loads behind the group / count tests became one branch and one wait per load
            float cdist = kInfF;
            int child = 0;
            int sw = 0;
            if (ginner) sw = min(kWide, t.levels - (31 - __builtin_clz(gnode)));   // ≤ 8 descendants: one per lane
            const bool gbox = ginner && gl < (1 << sw);
            const float4* rec = t.nodes + 3 * (gbox ? (((size_t)gnode << (sw - 1)) + (gl >> 1)) : (size_t)1);
            const float4 ra = rec[0], rb = rec[1], rc = rec[2];
            int lbase = 0, lcnt = 0;
            if (gleaf) {
                const int leaf = gnode - P;
                if (leaf < seed_lo || leaf > seed_hi) {
                    lbase = leaf * B;
                    lcnt = min(B, M - lbase);
                }
            }
            float4 lq[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int j = gl + 8 * k;
                lq[k] = t.mpt[(k < ppl && j < lcnt) ? lbase + j : 0];
            }
            pin_loaded(ra);
            pin_loaded(rb);
            pin_loaded(rc);
#pragma unroll
            for (int k = 0; k < 8; ++k) pin_loaded(lq[k]);
            if (gbox) {
                cdist = (gl & 1) ? box_d2(xf, rb.z, rb.w, rc.x, rc.y, rc.z, rc.w) : box_d2(xf, ra.x, ra.y, ra.z, ra.w, rb.x, rb.y);
                child = (gnode << sw) + gl;
            }
            float pd[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int j = gl + 8 * k;
                const float ex = lq[k].x - xf[0], ey = lq[k].y - xf[1], ez = lq[k].z - xf[2];
                const float d = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
                pd[k] = (k < ppl && j < lcnt) ? d : kInfF;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k >= ppl) break;
                unsigned long long m = __ballot(pd[k] <= bnd && pd[k] < worst());
                while (m) {
                    const int j = __builtin_ctzll(m);
                    m &= m - 1;
                    const float cd = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pd[k]), j));
                    const int cp = __builtin_amdgcn_readlane(lbase + gl + 8 * k, j);
                    if (cd <= bnd && cd < worst() && !__ballot(lane < KL && lpos == cp)) insert(cd, cp);
                }
            }
            const unsigned long long want = __ballot(child != 0 && cdist <= bnd * kBoxSlack);
            if ((want >> lane) & 1ull) {
                // rank among the wanted lanes above this one (a 64-bit shift by 64 is not 0 here)
                const int at = fsp + (lane == 63 ? 0 : __popcll(want >> (lane + 1)));
                fnode[wv][at] = child;
                fdist[wv][at] = cdist;
            }
            fsp += __popcll(want);
        }
    }
    if (!hmode) break;
    if (!(nearest() <= h2s)) {
        // no map point within h: too far whatever the rest of the list holds — leave an empty list
        // (k_finish: no NN-1 → "too far"; need_key = ∞ → never reused without a traversal)
        lkey = kInfF;
        lpos = -1;
        break;
    }
    hmode = false;                     // a point within h: the full-r search, from the root
    bnd = fminf(r2s, worst());
    }
    if (skip) {
        if (lane == 0) wlist[slot] = wskip;
    } else {
        if (lane < KL) lists[(size_t)lane * N + slot] = lpos;
        const bool lpos_any = __ballot(lane < KL && lpos >= 0) != 0ull;
        float lkr[KL];   // the list gathered to every lane for the reuse key
#pragma unroll
        for (int k = 0; k < KL; ++k) lkr[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lkey), k));
        // an h-mode list left empty was searched only to h: never reused (need ∞)
        const float nk = lpos_any ? need_key<KL>(lkr, (float)kp.r2, kp.K) : kInfF;
        if (lane == 0) {
            const float wk = worst();
            wlist[slot] = wk;
            xref[slot] = make_float4(xf[0], xf[1], xf[2], wk < kInfF ? wk : r2s);
            nref[slot] = nk;
        }
    }
    if (nbr_stats && lane == 0) {
        atomicAdd(&nbr_stats[2], (unsigned long long)n_leaf);
        atomicAdd(&nbr_stats[3], (unsigned long long)n_inner);
        atomicAdd(&nbr_stats[4], 1ull);
    }
    if constexpr (FUSED) {
#ifdef IMLS_DEBUG_WAVE_TRACE
        const long long dbg_q1 = wall_clock64();
#endif
        // the list as finish_q_core reads it: in the lanes, or (Verlet skip) still in memory
        const int pos = lane < KL ? (skip ? lists[(size_t)lane * N + slot] : lpos) : -1;
        finish_q_core<KL>(t, spt, fa.snr, (int)qperm[slot], slot, pose, kp, pos, skip ? wskip : worst(), fa.cs, fa.cd,
                          fa.cn, fa.tr, nbr_stats, snode[wv], sdist[wv]);
#ifdef IMLS_DEBUG_WAVE_TRACE
        // per-wave record of the last fused launch: start / traversal end / finish end (100 MHz
        // clock, low 32 bits), Verlet skip, leaves, inner steps, hardware id
        if (lane == 0 && slot < kDbgWaves) {
            unsigned* r = g_dbg_qwave[slot];
            r[0] = (unsigned)dbg_q0; r[1] = (unsigned)dbg_q1; r[2] = (unsigned)wall_clock64();
            r[3] = skip ? 1u : 0u; r[4] = n_leaf; r[5] = n_inner; r[6] = greedy ? 1u : 0u;
            r[7] = (unsigned)__builtin_amdgcn_s_getreg((23 << 0) | (0 << 6) | (31 << 11));   // HW_ID / HW_ID1
        }
#endif
    }
}

template <int KL>
__global__ __launch_bounds__(kWaveBlock) void k_knn_qwave(
        TreeView t, const float4* __restrict__ spt, const unsigned* __restrict__ qperm, int N,
        const double* __restrict__ pose, const int* __restrict__ done, KParams kp, const double* __restrict__ delta,
        int* __restrict__ lists, float* __restrict__ wlist, float4* __restrict__ xref, float* __restrict__ nref,
        int use_prev, unsigned long long* __restrict__ nbr_stats) {
    knn_qwave_body<KL>(t, spt, qperm, N, pose, done, kp, delta, lists, wlist, xref, nref, use_prev, nbr_stats,
                       (int)blockIdx.x);
}

template <int KL>
__global__ __launch_bounds__(kWaveBlock) void k_knn_qwave_f(
        TreeView t, const float4* __restrict__ spt, const unsigned* __restrict__ qperm, int N,
        const double* __restrict__ pose, const int* __restrict__ done, KParams kp, const double* __restrict__ delta,
        int* __restrict__ lists, float* __restrict__ wlist, float4* __restrict__ xref, float* __restrict__ nref,
        int use_prev, unsigned long long* __restrict__ nbr_stats, QFinishArgs fa) {
    knn_qwave_body<KL, true>(t, spt, qperm, N, pose, done, kp, delta, lists, wlist, xref, nref, use_prev, nbr_stats,
                             (int)blockIdx.x, fa);
}

template <int KL>
__global__ __launch_bounds__(kWaveBlock) void k_knn_qwave_b(const PairDev* __restrict__ tab, KParams kp, int use_prev,
                                                            int npairs) {
    int f, bx;
    batch_block(kp.xcd, f, bx);
    if (f >= npairs) return;
    const PairDev A = device_view(tab + f);
    if (!use_qwave(kp, A.N) || bx * (kWaveBlock / 64) >= A.N) return;
    const ListBlock lb = list_block(A.lists, A.N, KL);
    knn_qwave_body<KL>(A.t, A.spt, A.qperm, A.N, A.st.pose, A.st.done, kp, A.st.delta, lb.pos, lb.wlist, lb.xref, lb.nref,
                       use_prev, A.stats, bx);
}

}  // namespace

// sparse query sets (≤ kQwaveAutoN queries, e.g. FPS-sampled frames): one wave per query, with the
// exact stage in the same kernel (on the longer list lone_kl) for a lone frame of ≤ kSmallRows
void launch_knn_qwave(hipStream_t s, const ProjectLaunch& L, bool fused) {
    const int blocks = (L.N + kWaveBlock / 64 - 1) / (kWaveBlock / 64);
    with_list_sizes(L.kp.K, [&](auto z) {
        constexpr int KL = decltype(z)::KL;
        const ListBlock lb = list_block(L.lists, L.N, fused ? lone_kl<KL>() : KL);
        if (fused)
            k_knn_qwave_f<lone_kl<KL>()><<<blocks, kWaveBlock, 0, s>>>(L.t, L.spt, L.qperm, L.N, L.pose, L.done, L.kp, L.delta,
                                                                        lb.pos, lb.wlist, lb.xref, lb.nref, L.use_prev, L.stats,
                                                                        QFinishArgs{L.snr, L.cs, L.cd, L.cn, L.tr});
        else
            k_knn_qwave<KL><<<blocks, kWaveBlock, 0, s>>>(L.t, L.spt, L.qperm, L.N, L.pose, L.done, L.kp, L.delta, lb.pos,
                                                          lb.wlist, lb.xref, lb.nref, L.use_prev, L.stats);
    });
}

void launch_knn_qwave_batch(hipStream_t s, dim3 grid, const PairDev* tab, const KParams& kp, int use_prev, int npairs) {
    with_list_sizes(kp.K, [&](auto z) {
        k_knn_qwave_b<decltype(z)::KL><<<grid, kWaveBlock, 0, s>>>(tab, kp, use_prev, npairs);
    });
}

}  // namespace imlsgpu

#ifdef IMLS_DEBUG_WAVE_TRACE
// debug build only: per-wave records of the last k_knn_qwave_f launch (16 u32 per wave)
extern "C" int imls_debug_qwaves(unsigned* out, int nwaves) {
    const int n = nwaves < imlsgpu::kDbgWaves ? nwaves : imlsgpu::kDbgWaves;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(imlsgpu::g_dbg_qwave), (size_t)n * 64) == hipSuccess ? n : -1;
}
#endif
