// exact_stage.h — the gates, the IMLS projection, the plane_ICP projection and the pass-1 rows of
// one query, shared by the lane exact stage (finish.hip) and the wave one (knn_qwave.hip).
#pragma once
#include "project_common.h"

namespace imlsgpu {
namespace {

// imls_icp.cpp:442-451 / 681-692: acos(ns·n/(|ns||n|))·180/π > threshold; NaN passes (Q8).
// cthr = cos(threshold): away from it (|ca − cthr| > 1e-9, where the evaluated angle is ≥ 5e-8°
// from the threshold — ~6 orders above its rounding error) the comparison is decided without the
// fp64 acos; inside that band, and for NaN or ca < −1 (acos → NaN → passes), as the reference.
__device__ __forceinline__ bool angle_reject(const double ns[3], double n0, double n1, double n2, double thr,
                                             double cthr) {
    // fp32 screen: |ca₃₂ − ca₆₄| ≤ ~1e-6 (inputs rounded to float: 6e-8 each, the dot and the two
    // squared norms ≤ 3 ulp of their term sums, v_rsq ≤ 2 ulp — Cauchy–Schwarz bounds the dot's
    // terms by |ns||n|), so outside ±1e-5 of cos(θ) (and of −1) the fp32 cosine decides what the
    // fp64 evaluation below decides; squared-norm products outside [1e-20, 1e20] (denormal / huge /
    // NaN normals) and the band go to fp64
    {
        const float s0 = (float)ns[0], s1 = (float)ns[1], s2 = (float)ns[2];
        const float m0 = (float)n0, m1 = (float)n1, m2 = (float)n2;
        const float a = __builtin_fmaf(s0, s0, __builtin_fmaf(s1, s1, s2 * s2));
        const float b = __builtin_fmaf(m0, m0, __builtin_fmaf(m1, m1, m2 * m2));
        const float d = __builtin_fmaf(s0, m0, __builtin_fmaf(s1, m1, s2 * m2));
        const float ab = a * b;
        if (ab > 1e-20f && ab < 1e20f) {
            const float ca = d * __builtin_amdgcn_rsqf(ab);
            const float c = (float)cthr;
            if (ca > c + 1e-5f) return false;
            if (ca < c - 1e-5f && ca > -1.0f + 1e-5f) return true;
        }
    }
    double dot = ns[0] * n0;
    dot = dot + ns[1] * n1;
    dot = dot + ns[2] * n2;
    double a = ns[0] * ns[0];
    a = a + ns[1] * ns[1];
    a = a + ns[2] * ns[2];
    double b = n0 * n0;
    b = b + n1 * n1;
    b = b + n2 * n2;
    const double s = sqrt(a) * sqrt(b);
    // the same two decisions without the division: outside ±2e-9 of cthr, dot vs (cthr ± 2e-9)·s
    // decides exactly what ca = dot/s vs cthr ± 1e-9 decides (the division's rounding is ~1e-16
    // relative), and dot ≥ −s(1 − 1e-12) certifies ca ≥ −1; anything else (the bands, zero / ∞ /
    // NaN denominators) takes the reference's own evaluation below
    if (dot > (cthr + 2e-9) * s) return false;
    if (dot < (cthr - 2e-9) * s && dot >= -s * (1.0 - 1e-12)) return true;
    const double ca = dot / s;
    if (ca > cthr + 1e-9) return false;
    if (ca < cthr - 1e-9 && ca >= -1.0) return true;
    const double angle = acos(ca) * 180.0 / M_PI;
    return angle > thr;
}

// Gates + ImplicitMLSFunction + projection for one query given its exact neighbour list
// L = (ld[j], lpos[j]) for j ∈ [first, first+cnt) sorted by (d², index) and its NN-1 (d1, p1);
// positions are Morton positions (mpt/mnr: the neighbours of a query share cache lines).
// Returns the reject category or −1 (valid, yf/nf filled).  kq counts the returned neighbours.
// LAZY_D: ld is not read — the one distance the IMLS bandwidth needs (L[target], Q3) is recomputed
// from its point (the same fp64 expression, so the same bits), letting the caller's fp64 list die
// after the certification (k_finish's register budget).
template <int CAP, bool LAZY_D = false>
__device__ int finish_query(const float xf[3], const double ns[3], const double (&ld)[CAP], const int (&lpos)[CAP],
                            int first, int cnt, double d1, int p1, const TreeView& t, const KParams& kp, float yf[3],
                            float nf[3], int& kq, int qi) {
    if (p1 < 0) return IMLS_REJ_TOO_FAR;                      // InvalidIndex → counted as too far (Q18)
    if (d1 > kp.h2) return IMLS_REJ_TOO_FAR;                  // imls_icp.cpp:620
    double nn[3];
    if (kp.tv) {
        // imls_icp.cpp:634-643: the query's own voted normal (tv.hip); a zero tensor has none
        const double4 v = t.tvn[qi];
        if (v.w == 0.0) return IMLS_REJ_NO_NORMAL;
        nn[0] = v.x; nn[1] = v.y; nn[2] = v.z;
    } else {
        if (!kp.get_normals) return IMLS_REJ_INVALID_NORMAL;  // recompute branch under libnabo semantics (Q1)
        const float4 n4 = t.mnr[p1];
        nn[0] = n4.x; nn[1] = n4.y; nn[2] = n4.z;
    }
    if (!(isfinite(nn[0]) && isfinite(nn[1]) && isfinite(nn[2]))) return IMLS_REJ_INVALID_NORMAL;
    if (kp.angle_on && angle_reject(ns, nn[0], nn[1], nn[2], kp.angle_thr_deg, kp.cos_thr)) return IMLS_REJ_NORMAL_CONSTRAINT;
    const double xd[3] = {xf[0], xf[1], xf[2]};
    unsigned long long acc = 0ull;
    int nacc = 0;
    // the normals in chunks of 8 (the loads of a chunk issue together; 24 VGPRs in flight, not 3·CAP)
    constexpr int kChunk = 8;
#pragma unroll
    for (int j0 = 0; j0 < CAP; j0 += kChunk) {
        float4 qn[kChunk];
#pragma unroll
        for (int u = 0; u < kChunk; ++u) {
            const int j = j0 + u;
            const bool inl = j < CAP && j >= first && j < first + cnt;
            qn[u] = t.mnr[inl ? lpos[j < CAP ? j : 0] : p1];
        }
#pragma unroll
        for (int u = 0; u < kChunk; ++u) {
            const int j = j0 + u;
            const bool inl = j < CAP && j >= first && j < first + cnt;
            if (inl) {
                ++kq;
                // get_normals=false without count mode (TV's IMLS neighbours): every normal is ∞ (Q1)
                bool ok = kp.get_normals && isfinite(qn[u].x) && isfinite(qn[u].y) && isfinite(qn[u].z);
                if (ok && kp.angle_on) ok = !angle_reject(ns, qn[u].x, qn[u].y, qn[u].z, kp.angle_thr_deg, kp.cos_thr);
                if (ok) { acc |= 1ull << j; ++nacc; }
            }
        }
    }
    if (nacc < 3) return IMLS_REJ_MLS_FAIL;                   // imls_icp.cpp:463-466
    const int target = first + nacc - 1;                      // Q3: index into L, not into S
    // the accepted neighbours' points and normals in chunks of 8, every load of a chunk issued (and
    // pinned) before any term is formed — the first chunk with the bandwidth point L[target]; a term
    // is added as `accepted ? term : 0`, the same bits as skipping it (both sums start at +0 and so
    // are never −0: s + 0 = s)
    constexpr int kIChunk = IMLS_IMLS_CHUNK;
    float4 qp[kIChunk], qn[kIChunk];
    auto load_chunk = [&](int j0) {
#pragma unroll
        for (int u = 0; u < kIChunk; ++u) {
            const int j = j0 + u;
            const int pj = (j < CAP && (acc & (1ull << j))) ? lpos[j < CAP ? j : 0] : p1;
            qp[u] = t.mpt[pj];
            qn[u] = t.mnr[pj];
        }
    };
    auto pin_chunk = [&]() {
#pragma unroll
        for (int u = 0; u < kIChunk; ++u) {
            pin_loaded(qp[u]);
            pin_loaded(qn[u]);
        }
    };
    double dsel = 0.0;
    if (LAZY_D) {
        int ptg = p1;
#pragma unroll
        for (int j = 0; j < CAP; ++j) ptg = (j == target) ? lpos[j] : ptg;
        const float4 q = t.mpt[ptg];
        load_chunk(0);
        pin_loaded(q);
        pin_chunk();
        dsel = exact_d2(xd, q.x, q.y, q.z);
    } else {
#pragma unroll
        for (int j = 0; j < CAP; ++j) dsel = (j == target) ? ld[j] : dsel;
        load_chunk(0);
        pin_chunk();
    }
    const double hmax = sqrt(dsel) / 3;
    // exp(−‖x−p‖² / h / h) (imls_icp.cpp:470) with one reciprocal per query instead of two divisions
    // per neighbour: w moves by ≤ 2 ulp, y (stored as float) almost never (the 1e-5 y contract)
    const double ih2 = 1.0 / (hmax * hmax);
    double wsum = 0.0, psum = 0.0;
#pragma unroll
    for (int j0 = 0; j0 < CAP; j0 += kIChunk) {
        if (j0 > 0) {
            if (!__ballot((acc >> j0) != 0ull)) break;          // no lane has a later neighbour
            if (!__ballot((acc >> j0) & ((1ull << kIChunk) - 1ull))) continue;     // none in this chunk
            load_chunk(j0);
            pin_chunk();
        }
#pragma unroll
        for (int u = 0; u < kIChunk; ++u) {
            const int j = j0 + u;
            if (j >= CAP) break;
            const bool a = (acc >> j) & 1ull;
            if (!__ballot(a)) continue;                         // wave-uniform
            const double dx = xd[0] - (double)qp[u].x, dy = xd[1] - (double)qp[u].y, dz = xd[2] - (double)qp[u].z;
            double dn = dx * dx;
            dn = dn + dy * dy;
            dn = dn + dz * dz;
            const double w = exp(-dn * ih2);
            double pr = (w * dx) * (double)qn[u].x;
            pr = pr + (w * dy) * (double)qn[u].y;
            pr = pr + (w * dz) * (double)qn[u].z;
            wsum += a ? w : 0.0;
            psum += a ? pr : 0.0;
        }
    }
    const double height = psum / (wsum + 1e-5);               // Q4
    if (isnan(height) || isinf(height)) return IMLS_REJ_NAN_INF_HEIGHT;
    yf[0] = (float)(xd[0] - height * nn[0]);                  // imls_icp.cpp:719-729
    yf[1] = (float)(xd[1] - height * nn[1]);
    yf[2] = (float)(xd[2] - height * nn[2]);
    nf[0] = (float)nn[0]; nf[1] = (float)nn[1]; nf[2] = (float)nn[2];
    return -1;
}

// plane_ICP_proj's loop body after the NN-1 search (laser_odometry.cpp:352-396): unfound → "no
// normal" (the bounds check; no h gate — min_dist is unused) or, in projected-distance mode, an
// empty candidate list → "too far" (336-340); map normal finite, angle gate,
// y = x − ((x−p)·n)·n in double, stored as float.
__device__ int finish_plane(const float xf[3], const double ns[3], int p1, const TreeView& t, const KParams& kp,
                            float yf[3], float nf[3]) {
    if (p1 < 0) return kp.proj ? IMLS_REJ_TOO_FAR : IMLS_REJ_NO_NORMAL;   // empty candidate list: 336-340
    const float4 n4 = t.mnr[p1];
    const double nn[3] = {n4.x, n4.y, n4.z};
    if (!(isfinite(nn[0]) && isfinite(nn[1]) && isfinite(nn[2]))) return IMLS_REJ_INVALID_NORMAL;
    if (kp.angle_on && angle_reject(ns, nn[0], nn[1], nn[2], kp.angle_thr_deg, kp.cos_thr)) return IMLS_REJ_NORMAL_CONSTRAINT;
    const float4 q = t.mpt[p1];
    const double xd[3] = {xf[0], xf[1], xf[2]};
    const double v0 = xd[0] - (double)q.x, v1 = xd[1] - (double)q.y, v2 = xd[2] - (double)q.z;
    double pd = v0 * nn[0];
    pd = pd + v1 * nn[1];
    pd = pd + v2 * nn[2];
    yf[0] = (float)(xd[0] - pd * nn[0]);
    yf[1] = (float)(xd[1] - pd * nn[1]);
    yf[2] = (float)(xd[2] - pd * nn[2]);
    nf[0] = (float)nn[0]; nf[1] = (float)nn[1]; nf[2] = (float)nn[2];
    return -1;
}

// Row of the point-to-plane system for a valid correspondence (solver.cpp:95-103).
__device__ __forceinline__ void plane_row(const float xf[3], const float yf[3], const float nf[3], double a[6], double& b) {
    const double s0 = xf[0], s1 = xf[1], s2 = xf[2];
    const double d0 = yf[0], d1 = yf[1], d2 = yf[2];
    const double n0 = nf[0], n1 = nf[1], n2 = nf[2];
    a[0] = n2 * s1 - n1 * s2;
    a[1] = n0 * s2 - n2 * s0;
    a[2] = n1 * s0 - n0 * s1;
    a[3] = n0; a[4] = n1; a[5] = n2;
    b = n0 * (d0 - s0);
    b = b + n1 * (d1 - s1);
    b = b + n2 * (d2 - s2);
}

// Block-reduce the 28 normal-equation terms into out[0..27] (valid in threads < 28 after return).
template <int NT>
__device__ void block_normeq(const double a[6], double b, double one, double (*red)[kNormEq], double* out) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = r; c < 6; ++c) {
            const double v = wave_total(a[r] * a[c]);
            if (lane == 63) red[wv][k] = v;
            ++k;
        }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const double v = wave_total(a[r] * b);
        if (lane == 63) red[wv][21 + r] = v;
    }
    {
        const double v = wave_total(one);
        if (lane == 63) red[wv][27] = v;
    }
    __syncthreads();
    if (threadIdx.x < kNormEq) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) s += red[w][threadIdx.x];
        out[threadIdx.x] = s;
    }
    __syncthreads();
}

__device__ __forceinline__ void store_result(int i, int cat, const float xf[3], const float yf[3], const float nf[3],
                                             float4* cs, float4* cd, float4* cn) {
    cs[i] = make_float4(xf[0], xf[1], xf[2], cat == -1 ? 1.f : 0.f);
    // y and n are read only behind the valid flag (Rows::get, the RANSAC compaction, imls_project):
    // rejected rows skip them
    if (cat == -1) {
        cd[i] = make_float4(yf[0], yf[1], yf[2], 0.f);
        cn[i] = make_float4(nf[0], nf[1], nf[2], 0.f);
    }
}

}  // namespace
}  // namespace imlsgpu
