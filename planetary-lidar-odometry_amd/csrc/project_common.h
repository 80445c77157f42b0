// project_common.h — what more than one matching unit uses (knn_wave.hip, knn_qwave.hip, finish.hip,
// knn_export.hip and the host side, project.hip): the traversal constants and tuning macros, the
// list helpers, the DPP reductions, the launch geometry, the K → list-size table, and the host
// launchers the kernel units export to each other.
#pragma once
#include <algorithm>
#include <cfloat>

#include "internal.h"
#include "geom.h"

// v_writelane_b32: `old` with lane `sel`'s value replaced by the wave-uniform `v` (every lane
// takes part, whatever exec says); v and sel must be wave-uniform.  The documented builtin where
// the compiler has it; the clang of ROCm 7.2 has none, and there the LLVM intrinsic
// llvm.amdgcn.writelane (AMDGPUUsage) is declared under its own name — a declaration, not inline
// assembly: the kernel holds no asm beyond empty pins.
#if defined(__has_builtin) && __has_builtin(__builtin_amdgcn_writelane)
__device__ __forceinline__ int imls_amdgcn_writelane(int v, int sel, int old) {
    return __builtin_amdgcn_writelane(v, sel, old);
}
#else
__device__ int imls_amdgcn_writelane(int v, int sel, int old) __asm("llvm.amdgcn.writelane");
#endif

namespace imlsgpu {
namespace {

constexpr double kInfD = __builtin_huge_val();
constexpr float kInfF = __builtin_huge_valf();
constexpr int kWaveBlock = 256;
// constant address space view of read-only device data: wave-uniform loads through it are scalar
typedef float kf4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(4))) const kf4v kconst_f4;
// a value an earlier launch wrote and the whole wave reads (the done flag, the last Δ): through the
// constant address space, i.e. scalar loads — not a per-lane (flat, in the batched kernels) load
__device__ __forceinline__ int ld_const(const int* p) { return *(const __attribute__((address_space(4))) int*)p; }
__device__ __forceinline__ double ld_const(const double* p) { return *(const __attribute__((address_space(4))) double*)p; }
constexpr int kFallbackBlocks = 64;
constexpr int kFallbackBlocksBatched = 4;   // physical blocks per frame of a large batch (same slabs)
constexpr int kFinishPerBlock = kWaveBlock;   // queries per k_finish block = per pass-1 slab
static_assert(kFinishPerBlock == kPass1Block && kFallbackBlocks == kPass1Fallback, "pass-1 slab layout (solve.hip)");
constexpr int kWideMax = 8;         // packet traversal: children tested per step (2^wide, wide ≤ 3)
constexpr int kWaveStack = 64;       // its stack: ≤ 7 entries per step × ⌈23/3⌉ steps
constexpr int kFStack = 256;        // frontier traversal's stack per wave (see knn_qwave_body)
constexpr int kFBatchMax = 128;     // above this many entries: one entry per step (DFS growth ≤ 8 × 7)
// frontier stack bound: a step at ≤ kFBatchMax entries pushes ≤ 8 groups × 8 children; above it one
// entry per step grows the stack by ≤ 7 per descent step, and a walk descends ≤ ⌈(kStackDepth−1)/kWide⌉
// steps (the index refuses deeper trees, index.hip) — so fsp never exceeds kFStack
static_assert(kFBatchMax + 64 + 7 * ((24 + 2) / 3) <= kFStack, "frontier stack bound");
#ifndef IMLS_SEED_CHUNK
#define IMLS_SEED_CHUNK 8
#endif
constexpr int kSeedChunk = IMLS_SEED_CHUNK;   // per-lane reseed: points loaded per batch
constexpr int kSeedTab = 1024;                // seed search: coarse leaf-key table entries in LDS (8 KB)
// traversal constants (measured in rounds 1-4; no runtime selectors)
constexpr int kSeedHalf = 1;        // a seed scans the query's Morton leaf ± 1 neighbour leaf
constexpr float kReseed = 0.25f;    // temporal seed unless displacement² > kReseed · previous worst key
#ifndef IMLS_BC_GROUP
#define IMLS_BC_GROUP 4
#endif
constexpr int kBcGroup = IMLS_BC_GROUP;          // broadcast leaf scan: points per scalar-load group
#ifndef IMLS_SPARSE_LANES
#define IMLS_SPARSE_LANES 20
#endif
constexpr int kSparseLanes = IMLS_SPARSE_LANES;    // a leaf wanted by ≤ this many lanes is scanned per lane, not per point
constexpr int kWide = 3;            // binary levels descended per traversal step (8 boxes per step)
constexpr float kBoxSlack = 1.0f + 2e-6f;     // fp32 box / point distance vs exact: ≤ 3.1e-7 rel.
// Round 6: the traversals search radius (1 + skin)·r, not r.  A query with fewer than K map points
// within r ("underfull": the far, sparse part of a scan) relies on EVERY point within r; its list from
// a search of radius r could never be reused (no skin: any move may bring a point inside r), so it
// re-walked the whole r-ball every ICP iteration — the converged iterations' tail.  Searched to
// (1 + skin)·r, its list certifies reuse while the query moves < skin·r / 2 (need = r², verlet_skip).
// Dense queries are unaffected (their bound is the KL-th key ≪ r² after the seed / prefill); k_finish
// still counts only the points within r.
#ifndef IMLS_UNDER_SKIN
#define IMLS_UNDER_SKIN 0.05
#endif
constexpr double kSearchR2 = (1.0 + IMLS_UNDER_SKIN) * (1.0 + IMLS_UNDER_SKIN);   // search r² / r²
constexpr double kCertSlack = 1.0 + 4e-7;
// list length for K ≤ 20 (the shipped K = 20; with_list_sizes below)
#ifndef IMLS_B_KL
#define IMLS_B_KL 22
#endif
#ifndef IMLS_DIST_CHUNK
#define IMLS_DIST_CHUNK 22
#endif
#ifndef IMLS_IMLS_CHUNK
#define IMLS_IMLS_CHUNK 4
#endif
#ifdef IMLS_DEBUG_WAVE_TRACE
constexpr int kDbgWaves = 8192;   // diagnostic build: per-wave records kept per traversal unit
#endif

__device__ __forceinline__ bool lessp(double da, int ia, double db, int ib) {
    return da < db || (da == db && ia < ib);
}

// min(a, b) of non-NaN floats (a plain select: fminf canonicalises both operands first)
__device__ __forceinline__ float fmin_nn(float a, float b) { return a < b ? a : b; }

// Keeps a gather where it is issued: the empty asm consumes the loaded registers, so the compiler
// cannot sink the load into the conditional block that uses it (and wait on it there, one
// dependent round trip per gather) — the loads of a chunk all issue before any is waited on.
__device__ __forceinline__ void pin_loaded(const float4& v) { asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z)); }

// Keys-only sorted insertion into the ascending list (precondition d < lk[KL−1]): key k becomes
// med3(lk[k−1], d, lk[k]) — the keys are sorted and never NaN — one v_med3 per slot.
template <int KL>
__device__ __forceinline__ void insert_key(float (&lk)[KL], float d) {
#pragma unroll
    for (int k = KL - 1; k >= 1; --k) lk[k] = __builtin_amdgcn_fmed3f(lk[k - 1], d, lk[k]);
    lk[0] = fmin_nn(d, lk[0]);
}


// Verlet-list reuse (neighbour lists with a skin, as in molecular dynamics): a query's list was
// built at xr.xyz with the guarantee that every map point outside it has fp32 key ≥ xr.w, and
// nr = the key its exact answer relied on there (the K-th key within r, or the NN-1 key if
// larger; ∞ when fewer than K points were within r).  At the new position x, |x − xr| = D:
//   * every point outside the list is at exact distance ≥ √xr.w − D          (lower bound W'),
//   * the answer needs distances ≤ √nr + D (those K points are still there)   (upper bound U),
// so the list — unchanged, not even re-read — still holds the exact answer when U < W'.
// fp32 keys carry ≤ 3.1e-7 relative error and D ≤ 3e-7: the 1e-6 factors and the 1e-5 margin
// cover both; k_finish re-certifies in fp64 against W' (a failure there only costs the exact
// fallback).  Returns true when the traversal can be skipped; w_out = W' (also when the stale
// bound U fails: w_low = W' whenever it is positive, else −1 — the prefilled list, re-measured at x,
// may still certify itself against it, see knn_wave_body).
__device__ __forceinline__ bool verlet_skip(float4 xr, float nr, const float xf[3], float r2s, float& w_out,
                                            float& w_low) {
    const float dx = xf[0] - xr.x, dy = xf[1] - xr.y, dz = xf[2] - xr.z;
    const float D = sqrtf(__builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz))) * (1.0f + 1e-6f) + 1e-6f;
    const float g = sqrtf(xr.w) * (1.0f - 1e-6f) - D;
    w_low = g > 0.f ? fminf(g * g, r2s) : -1.0f;
    if (!(g > 0.f) || !(nr < kInfF)) return false;
    const float u = sqrtf(nr) * (1.0f + 1e-6f) + D;
    const float w = fminf(g * g, r2s);
    w_out = w;
    return u * u * (1.0f + 1e-5f) < w;
}

// The key a fresh list's exact answer relies on (see verlet_skip): max(K-th key within r, NN-1
// key), ∞ when fewer than K keys are within r or no NN-1 exists.  lk ascending.
template <int KL>
__device__ __forceinline__ float need_key(const float (&lk)[KL], float r2, int K) {
    const float r2f = r2 * (1.0f + 1e-6f);
    int cnt_r = 0;
    float dK = kInfF, d1 = kInfF;
#pragma unroll
    for (int j = 0; j < KL; ++j) {
        const bool in = lk[j] <= r2f;
        cnt_r += in ? 1 : 0;
        if (in && d1 == kInfF && lk[j] > 1e-15f) d1 = lk[j];
        if (j == K - 1) dK = lk[j];
    }
    // fewer than K within r: the answer is every point within r (none when no NN-1 exists either)
    return cnt_r >= K ? fmaxf(dK, d1) : (IMLS_UNDER_SKIN > 0 ? r2f : kInfF);
}

// ---------------------------------------------------------------------------------------------
// Slot-id keys (the LDS-list traversal): a lane's top-KL list is its KL keys in registers, kept
// ascending, each key = the fp32 squared distance with its low IDB mantissa bits replaced by the id
// of the LDS slot that holds the point's position.  An insertion evicts the list's last key, whose
// slot takes the new position (one ds_write at a lane-specific address) and whose id the new key
// inherits; the keys move by med3 alone (one VALU per slot) — the positions never move, where the
// register list moves every position with two selects per slot (88 → ~26 VALU per insertion).
//
// Truncation keeps the search exact.  A point is inserted iff trunc(d) < trunc(max key), i.e.
// d < thr = float(bits(max) & ~IDM); thr only falls during the walk, so every point never inserted
// has d ≥ thr_final, and an evicted point's truncated key was ≥ the new maximum's — every point
// outside the final list has d32 ≥ thr_final, which is the W this traversal reports (≤ 2^(IDB−23)
// below the full-precision KL-th key: k_finish's fp64 certificate against W is unchanged).
// Upper bounds taken from a key (need_key_ids, the Verlet reuse) round up: d ≤ float(bits | IDM).
// Empty slots hold finite sentinels kIdSentinel | id (above every real key, never NaN for med3).
// ---------------------------------------------------------------------------------------------
template <int KL>
struct IdKeys {
    static constexpr unsigned IDM = KL <= 32 ? 31u : 63u;
    static constexpr unsigned kSentinel = 0x7F7FFFFFu & ~IDM;
    __device__ static __forceinline__ float lo(float k) { return __uint_as_float(__float_as_uint(k) & ~IDM); }
    __device__ static __forceinline__ float hi(float k) { return __uint_as_float(__float_as_uint(k) | IDM); }
    __device__ static __forceinline__ unsigned id(float k) { return __float_as_uint(k) & IDM; }
    __device__ static __forceinline__ float make(float d, unsigned s) { return __uint_as_float((__float_as_uint(d) & ~IDM) | s); }
    __device__ static __forceinline__ float empty(unsigned s) { return __uint_as_float(kSentinel | s); }
    __device__ static __forceinline__ bool real(float k) { return (__float_as_uint(k) & ~IDM) < kSentinel; }
};

// need_key over slot-id keys: max(K-th key within r, NN-1 key), every bound rounded up (a key's
// point lies in [lo, hi]); ∞ when fewer than K keys are surely within r or no NN-1 exists.
template <int KL>
__device__ __forceinline__ float need_key_ids(const float (&lk)[KL], float r2, int K) {
    using I = IdKeys<KL>;
    const float r2f = r2 * (1.0f + 1e-6f);
    int cnt_r = 0;
    float dK = kInfF, d1 = kInfF;
#pragma unroll
    for (int j = 0; j < KL; ++j) {
        const float up = I::hi(lk[j]);
        const bool in = I::real(lk[j]) && up <= r2f;
        cnt_r += in ? 1 : 0;
        if (in && d1 == kInfF && I::lo(lk[j]) > 1e-15f) d1 = up;
        if (j == K - 1) dK = up;
    }
    return cnt_r >= K ? fmaxf(dK, d1) : (IMLS_UNDER_SKIN > 0 ? r2f : kInfF);   // (need_key)
}

// Wave-wide reductions on the vector pipe (DPP; every lane of the wave active).  dpp_i: lane i takes
// the value of the lane CTRL names, or `old` where that lane lies outside the row or ROWS excludes
// lane i's row.  wave_reduce: an inclusive scan along each row of 16 (row_shr 1, 2, 4, 8), then lane
// 15 of rows 0 and 2 into rows 1 and 3 (row_bcast:15) and lane 31 into rows 2 and 3 (row_bcast:31):
// lane 63 holds the wave's total, which wave_last hands to the scalar side.
constexpr int kDppShr1 = 0x111, kDppShr2 = 0x112, kDppShr4 = 0x114, kDppShr8 = 0x118;
constexpr int kDppBcast15 = 0x142, kDppBcast31 = 0x143;
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ int dpp_i(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, ROWS, 0xf, false); }
struct RedOr { static constexpr int id = 0; __device__ static __forceinline__ int op(int a, int b) { return a | b; } };
struct RedAdd { static constexpr int id = 0; __device__ static __forceinline__ int op(int a, int b) { return a + b; } };
template <class R>
__device__ __forceinline__ int wave_reduce(int v) {
    v = R::op(v, dpp_i<kDppShr1>(R::id, v));
    v = R::op(v, dpp_i<kDppShr2>(R::id, v));
    v = R::op(v, dpp_i<kDppShr4>(R::id, v));
    v = R::op(v, dpp_i<kDppShr8>(R::id, v));
    v = R::op(v, dpp_i<kDppBcast15, 0xa>(R::id, v));
    return R::op(v, dpp_i<kDppBcast31, 0xc>(R::id, v));
}
__device__ __forceinline__ int wave_last(int v) { return __builtin_amdgcn_readlane(v, 63); }

struct QFinishArgs {
    const float4* snr;
    float4 *cs, *cd, *cn;
    imls_iter_trace* tr;
};

// k_finish blocks of a frame (one pass-1 slab each, before the kFallbackBlocks fallback slabs)
__host__ __device__ __forceinline__ int finish_blocks_of(int N) { return (N + kFinishPerBlock - 1) / kFinishPerBlock; }
// traversal blocks for packets of qp queries per wave
__host__ __device__ __forceinline__ int knn_blocks_of(int N, int qp) {
    const int per = qp * (kWaveBlock / 64);
    return (N + per - 1) / per;
}
// traversal choice (launch_project): one wave per query for sparse query sets, packets otherwise
__host__ __device__ __forceinline__ bool use_qwave(const KParams& kp, int N) {
    return kp.qwave > 0 || (kp.qwave < 0 && N <= kQwaveAutoN);
}
// one-frame launches of a small frame (≤ kSmallRows queries, solved by k_solve_small from its rows):
// the exact stage fused into the wave-per-query traversal (k_knn_qwave_f), nothing deferred — one
// projection launch per ICP iteration
__host__ __forceinline__ bool fused_stage(const KParams& kp, int N) { return use_qwave(kp, N) && N <= kSmallRows; }

// The (frame, block) a batched block works on.  xcd: blocks are dealt round-robin over the 8 XCDs
// (b and b + 8 share one, MI355X_MICROARCH.md §Workgroup dispatch), so frame f takes the blocks of
// one round-robin slot (f mod 8) — its blocks share that XCD's L2 (a frame's map and tree),
// instead of every frame being spread over all eight.  grid.y is then padded to a multiple of 8.
__device__ __forceinline__ void batch_block(int xcd, int& frame, int& bx) {
    if (!xcd) {
        frame = (int)blockIdx.y;
        bx = (int)blockIdx.x;
        return;
    }
    const unsigned nx = gridDim.x;
    const unsigned p = blockIdx.x + blockIdx.y * nx;
    const unsigned s = p >> 3;
    frame = (int)((p & 7u) + 8u * (s / nx));
    bx = (int)(s % nx);
}

// The lone small frame's list (k_knn_qwave_f): entry k in lane k, so a longer list costs the wave no
// registers — K + 12 entries instead of K + 2 give the Verlet certificate a longer skin (√W − √need:
// the 32nd vs the 20th neighbour's distance instead of the 22nd), so fewer steady-iteration queries
// re-traverse (the slowest 2 % set each launch's length).  The list is read only by the same kernel.
#ifndef IMLS_LONE_EXTRA
#define IMLS_LONE_EXTRA 10
#endif
template <int KL>
constexpr int lone_kl() { return KL + IMLS_LONE_EXTRA <= kMaxKL ? KL + IMLS_LONE_EXTRA : kMaxKL; }

// K → (list length KL of the float traversals, heap capacity KCAP of the exact per-lane search): the
// one table every launcher instantiates its kernels from.  f is called with the rung's KSizes tag.
// K ≤ 20 (the shipped 20): two slack entries certify every query on config B (KL 21 left a few
// uncertified → the slow exact fallback, −30 %; KL 22 vs 24 measured +6.7 % pairs/s, 4 in flight)
template <int KL_, int KCAP_>
struct KSizes {
    static constexpr int KL = KL_, KCAP = KCAP_;
};
template <class F>
void with_list_sizes(int K, F&& f) {
    if (K <= 8) f(KSizes<12, 8>{});
    else if (K <= 16) f(KSizes<20, 16>{});
    else if (K <= 20) f(KSizes<IMLS_B_KL, 20>{});
    else f(KSizes<36, 32>{});
}

}  // namespace

// Host launchers of the kernel units, called from project.hip and knn_export.hip (a kernel template is
// instantiated where it is launched).  Hidden: internal to the library, out of its dynamic symbol
// table.  Each takes the list sizes of its K's rung (with_list_sizes); the batched ones launch over
// `grid` = (blocks of the largest frame, frames).
#pragma GCC visibility push(hidden)
// knn_wave.hip — the packet traversal
void launch_knn_wave(hipStream_t s, const ProjectLaunch& L);
void launch_knn_wave_batch(hipStream_t s, dim3 grid, const PairDev* tab, const KParams& kp, int use_prev, int npairs);
// knn_qwave.hip — one wave per query; fused: with the exact stage in the same kernel (k_knn_qwave_f)
void launch_knn_qwave(hipStream_t s, const ProjectLaunch& L, bool fused);
void launch_knn_qwave_batch(hipStream_t s, dim3 grid, const PairDev* tab, const KParams& kp, int use_prev, int npairs);
// finish.hip — the exact stage, and the exact per-lane search over the queries it deferred
// (deferred) or over every query (lane mode), into the kFallbackBlocks slabs behind k_finish's
void launch_finish(hipStream_t s, const ProjectLaunch& L);
void launch_finish_batch(hipStream_t s, dim3 grid, const PairDev* tab, const KParams& kp, int it, int npairs);
void launch_lane(hipStream_t s, const ProjectLaunch& L, bool deferred);
void launch_lane_batch(hipStream_t s, dim3 grid, const PairDev* tab, const KParams& kp, int it);
#pragma GCC visibility pop

}  // namespace imlsgpu
