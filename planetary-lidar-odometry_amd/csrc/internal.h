// internal.h — shared declarations of the HIP IMLS-ICP path (gfx950 only).
//
// HBM layout (SoA-of-float4, 16-B aligned, one record per point):
//   target, filtered order   : tpt[M]  = (x, y, z, 0)      tnr[M] = (nx, ny, nz, 0)
//   target, Morton order     : mpt[M]  = (x, y, z, bits(filtered index))   ← leaf scans
//   tree (implicit, complete): node i ∈ [1, P) holds the AABBs of children 2i, 2i+1 as
//                              3 float4 (lo_l.xyz, hi_l.x | hi_l.yz, lo_r.xy | lo_r.z, hi_r.xyz);
//                              leaf node P + b = bucket b = mpt[b·B, min((b+1)·B, M)).
//   source, filtered order   : spt[N], snr[N] float4
//   correspondences, per source index (uncompacted): cs[N] = (x, valid), cd[N] = (y, ·),
//                              cn[N] = (n, ·) float4 — source order is implicit in the index.
#pragma once
#include <algorithm>
#include <cstddef>
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/imls_gpu.h"

namespace imlsgpu {

constexpr int kBlock = 256;            // threads per block for streaming kernels
constexpr int kProjBlock = 128;        // threads per block for the projection kernel
constexpr int kStackDepth = 24;        // traversal stack entries per lane (tree depth ≤ 24)
constexpr int kHistBins = 65536;       // residual histogram bins (top 16 bits of float |r|: 1/128 octave)
constexpr int kCandCap = 8192;         // exact-select candidates handled in LDS per boundary bin
constexpr int kNormEq = 28;            // 21 (JᵀJ upper) + 6 (Jᵀb) + 1 (row count)

// Device-side per-iteration record, laid out as imls_iter_trace.
static_assert(sizeof(imls_iter_trace) == 16 * 8 * 2 + 8 * 8, "trace layout");

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// Grow-only device buffers (api_support.hip).  A buffer being replaced may still be read by work already
// enqueued on any of the library's streams, and hipFree would wait for the whole device (every
// context's work in flight, and the host).  So the old buffer is RETIRED instead: an event is
// recorded on every registered stream of its device that still has work, and the buffer is handed
// out again (to any grow of a size it fits) only once all of those events have completed; retired
// buffers are freed at teardown (imls_destroy).  devbuf_grow(b, bytes, alloc): no-op when b holds
// `bytes`, else b becomes a buffer of ≥ alloc bytes (alloc ≥ bytes: the caller's headroom).
bool devbuf_grow(DevBuf& b, size_t bytes, size_t alloc);
void devbuf_retire(DevBuf& b);         // b → retired (empty afterwards)
// the streams the library enqueues on (context, upload and caller-set streams), reference counted
void register_stream(hipStream_t s, int device);
void unregister_stream(hipStream_t s);
// teardown: free every retired buffer of `device` (hipFree waits for the device)
void release_retired(int device);
// scratch layouts: the next n elements of T at p, p moved on to the following 256-B boundary
template <typename T>
constexpr size_t carve_bytes(size_t n) { return (n * sizeof(T) + 255) / 256 * 256; }
template <typename T>
T* carve(char*& p, size_t n) {
    T* r = reinterpret_cast<T*>(p);
    p += carve_bytes<T>(n);
    return r;
}

// Parameters the kernels need, in a flat POD copied by value into launches.
struct KParams {
    double h2, r2, cos_thr;   // cos_thr = cos(angle_thr_deg · π/180): the angle gates' fast path
    double angle_thr_deg;
    int K;                    // search_number
    int angle_on;
    int get_normals;
    int transform_normal;
    int correspond_number;
    int solve_method;
    double ls_threshold;
    double delta_dist, delta_angle;
    int matcher;              // imls_match_method: 0 IMLS, 1 plane_ICP (NN-1 tangent-plane projection)
    int proj;                 // projected-distance candidate rule (brute force in the reference)
    double gate_dist, gate_proj;   // proj mode: ‖p−x‖ < gate_dist and ‖(p−x)×n_s‖ < gate_proj
    // traversal tuning: documented runtime options (imls_set_option, include/imls_gpu.h), fixed
    // constants otherwise (project_common.h: kSeedHalf, kReseed, kSparseLanes, kWide)
    int qwave;                // traversal: −1 auto (one wave per query up to kQwaveAutoN queries), 0 packets, 1 wave per query
    int packet;               // packet traversal: queries per wave in this launch (64, or 32 / 16: see pk_small)
    int pk_small, pk_iters;   // the first pk_iters ICP iterations (mostly seeding lanes) use pk_small-query packets
    int pk_batch;             // … in batched launches too (imls_register_frames; off: measured slower there)
    int reuse;                // Verlet reuse of a query's list without traversal while its certificate holds
    int force_fb;             // test hook: every force_fb-th query slot's list treated as uncertified (0 off)
    int xcd;                  // batched projection: frames grouped per XCD round-robin slot (−1 auto: ≥ 16 frames)
    int tv;                   // tensor-voting normals (use_tensor_voting && !get_normals, IMLS matcher)
    int tv_k;                 // use_tensor_voting.k (≤ kTvMaxK)
    double tv_sigma, tv_thr;  // use_tensor_voting.sigma, .distance_threshold
    float tv_skin;            // TV ball lists reused while the query moved ≤ skin (m); 0 = every iteration walks the tree
    int robust_loss;          // imls_robust_loss (solve_method IMLS_SOLVE_ROBUST only, as the next two)
    int robust_iters;         // K: re-weighted 6×6 solves per robust solve (1 … 32)
    double robust_scale;      // c of ψ(r; c)
};
// the parameters of ICP iteration `it`'s projection launch (packet size of the traversal)
inline KParams kp_at(const KParams& k, int it) {
    KParams r = k;
    r.packet = it >= 0 && it < k.pk_iters ? k.pk_small : 64;
    return r;
}
constexpr int kTvMaxK = 64;    // tensor-voting kNN size handled on device
constexpr int kTvList = 64;    // TV skin list: ball(ρ + skin) members stored per query (more: not stored)
// per-query TV state behind TreeView::tvn, arrays of N: voted normal (double4), skin reference
// (float4: x, count), skin list (kTvList Morton positions), summed tensor (9 doubles)
constexpr size_t kTvBytesPerQuery = 32 + 16 + 4 * kTvList + 72;

struct TreeView {
    const float4* mpt;        // map points in Morton order, w = original index (bits)
    const float4* mnr;        // their normals, same order
    const unsigned* ipos;     // original index → Morton position
    const float4* nodes;      // 3 float4 per internal node, index 1..P-1 (entry 0 unused)
    const float4* tpt;
    const float4* tnr;
    int M, B, P, levels;
    const unsigned long long* lkeys;   // [L] Morton key of each leaf's first point (seed search)
    const float* qparams;              // [4] Morton quantisation: bbox lo xyz, scale
    int L;                             // leaves holding points
    const float4* mten;                // TV: input tensors in Morton order, 2 float4 per point
                                       //     (xx, xy, xz, yy | yz, zz, 0, 0), or null
    const double4* tvn;                // TV: per source index, the voted normal + found flag (w)
};

// 48-bit Morton code with isotropic quantisation (one scale for all axes keeps buckets compact);
// shared by the index build and the query-side seed search so both quantise identically.
__device__ __forceinline__ unsigned long long spread3_16(unsigned v) {
    unsigned long long x = v & 0xFFFFull;
    x = (x | (x << 16)) & 0x0000FF0000FFull;
    x = (x | (x << 8)) & 0x00F00F00F00Full;
    x = (x | (x << 4)) & 0x0C30C30C30C3ull;
    x = (x | (x << 2)) & 0x249249249249ull;
    return x;
}
__device__ __forceinline__ unsigned long long morton48(float x, float y, float z, const float* __restrict__ qp) {
    const float qmax = 65535.f, sc = qp[3];
    const unsigned qx = (unsigned)fminf(fmaxf((x - qp[0]) * sc, 0.f), qmax);
    const unsigned qy = (unsigned)fminf(fmaxf((y - qp[1]) * sc, 0.f), qmax);
    const unsigned qz = (unsigned)fminf(fmaxf((z - qp[2]) * sc, 0.f), qmax);
    return spread3_16(qx) | (spread3_16(qy) << 1) | (spread3_16(qz) << 2);
}

// Sum of v over the wave's 64 lanes, valid in lane 63 only: an inclusive scan of each 16-lane row by
// DPP row shifts (1, 2, 4, 8), then row_bcast:15 and row_bcast:31 carry the row totals into lane 63 —
// VALU moves only (a __shfl_xor butterfly is 12 ds_bpermute LDS round trips per fp64 sum).  A fixed
// association: the same bits on every run and in every kernel that uses it.
template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp_add_f64(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(unsigned long long)b, CTRL, ROWS, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)((unsigned long long)b >> 32), CTRL, ROWS, 0xf, true);
    return v + __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
__device__ __forceinline__ double wave_total(double v) {
    v = dpp_add_f64<0x111, 0xf>(v);    // row_shr:1
    v = dpp_add_f64<0x112, 0xf>(v);    // row_shr:2
    v = dpp_add_f64<0x114, 0xf>(v);    // row_shr:4
    v = dpp_add_f64<0x118, 0xf>(v);    // row_shr:8  → lane 15 of each row holds its row's sum
    v = dpp_add_f64<0x142, 0xa>(v);    // row_bcast:15 into rows 1 and 3
    v = dpp_add_f64<0x143, 0xc>(v);    // row_bcast:31 into rows 2 and 3 → lane 63 holds the total
    return v;
}

// The wave's totals of 28 values per lane (a[28..31] = 0): recursive halving — at lane bit 2h each
// lane keeps one half of its 2h values and adds the partner's copy of that half (32 fp64 exchanges,
// where 28 wave_total reductions issue 168 DPP steps); lane 2k returns value k's total.  A fixed
// association, shared by the solve kernels' normal-equation reductions (block_sum28 and block_normeq
// of solve_common.h, k_collect); the projection kernels keep wave_total (their 64 extra VGPRs spill
// the traversal's 96-register budget).
__device__ __forceinline__ double xor_f64(double v, int m) {
    const long long b = __double_as_longlong(v);
    const int lo = __shfl_xor((int)(unsigned)(b & 0xffffffffll), m, 64);
    const int hi = __shfl_xor((int)(unsigned)((unsigned long long)b >> 32), m, 64);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
template <int H>
__device__ __forceinline__ void wave_halve(double (&a)[32], int lane) {
    const bool up = (lane & (2 * H)) != 0;
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const double send = up ? a[i] : a[H + i];
        const double keep = up ? a[H + i] : a[i];
        a[i] = keep + xor_f64(send, 2 * H);
    }
    if constexpr (H > 1) wave_halve<H / 2>(a, lane);   // static indices at every level (no stack array)
}
__device__ __forceinline__ double wave_sum28(double (&a)[32]) {
    const int lane = threadIdx.x & 63;
    wave_halve<16>(a, lane);
    return a[0] + xor_f64(a[0], 1);
}

// What a solve leaves for the pose-info pass (pose_info.hip) — written ONLY through a non-null
// SolveState::info (imls_capture_pose_info on), with ordinary vector stores: the two ends of a trimmed
// solve's kept interval in the total order (|r₁| bits, row), the first solution the keys were taken
// under, the vector the solve turned into Δ, DRPM's six probabilities.
struct InfoExport {
    unsigned long long key_lo, key_hi;
    unsigned row_lo, row_hi;
    double x0[6], x[6], prob[6];
    int kind;                 // InfoKind of the last solve that succeeded (0: none since the reset)
    int iteration;            // the trace index of that solve
    int degenerate;           // DRPM took the SNR-weighted branch
    int pad;
};
// (kInfoRobust: every valid row, weight u·ψ(a·x0 − b): x0 = x^{K−1}, the vector the last weights were taken under)
enum InfoKind { kInfoNone = 0, kInfoAll = 1, kInfoTrim = 2, kInfoDrpm = 3, kInfoRobust = 4 };

// Solver scratch living in device memory (one per context).
struct SolveState {
    double* pose;             // [16] current rPose
    double* delta;            // [16] last Δ
    double* x0;               // [8]  first LS solution
    int* done;                // [1]  frame finished (converged / too few / failed)
    int* status;              // [1]  imls_frame_status
    int* iters;               // [1]  iterations run
    unsigned* hist;           // [kHistBins]
    unsigned* coarse;         // [kHistBins / 256] the same histogram, 256 bins per entry
    unsigned* cand_count;     // [2]
    unsigned long long* cand_lo;   // [kCandCap*?] (key bits) pairs with row index
    unsigned* cand_lo_row;
    unsigned long long* cand_hi;
    unsigned* cand_hi_row;
    int* sel;                 // [8] select metadata: b_lo, b_hi, c_lo, c_hi, lower, upper, nvalid
    double* partial1;         // [blocks × kNormEq] pass-1 block partials
    double* partial2;         // [blocks × kNormEq] pass-2 block partials
    double* keys;             // [N] |r|
    imls_iter_trace* trace;   // [iterations]
    int partial_cap;
    InfoExport* info;         // null unless pose-info capture is on (then every solve exports)
};

// RANSAC state of one context (ransac.hip), carved from its RANSAC scratch by ransac_frame() (solve.h).
struct RansacDev {
    int* rng;          // [34] glibc state (persistent)
    int* counts;       // [kHypMax]
    double* T;         // [kHypMax × 16]
    int* best;         // [1]
    int* evaluated;    // [1]
    int* rdone;        // [1] RANSAC finished (early exit or max iterations)
    double* bestT;     // [16]
    int* active;       // [1] the frame was still running when this solve began
};
struct DrpmDev {
    double* H;         // [36] row-major
    double* g;         // [6]
    double* U;         // [36] eigenvectors as columns: U[k·6 + r] = component r of vector k
    double* ev;        // [6] ascending
    double* slabs;     // [blocks × kDrpmSlab]
};
struct RansacFrame {
    double* all;       // [10·cap] the compacted valid correspondences (fp64 Rows layout)
    double* inl;       // [10·cap] the inliers of the best Δ with their weights
    int* blkcnt;       // [nb + 1] compaction block counts → offsets
    double* blkw;      // [nb + 1] compaction block Σw
    int *cnt_all, *cnt_in;
    double* wsum;      // Σw of the inliers
    RansacDev R;
    DrpmDev Dv;
    int cap;           // max(N, 1)
};

// One registration of a batched launch (imls_register_frames): everything a per-iteration kernel
// reads or writes for that frame.  The batch's table of these lives in device memory; a batched
// kernel takes its frame from tab[blockIdx.y] (a wave-uniform, read-only load: scalar) and runs the
// same body as the single-frame kernel, so a frame gives bit-identical results either way.
struct PairDev {
    TreeView t;
    const float4* spt;
    const float4* snr;
    const unsigned* qperm;
    int N;
    float4 *cs, *cd, *cn;
    int* lists;                        // [KL][N] + worst keys + xref/nref (prevnn_bytes)
    SolveState st;
    imls_iter_trace* trace;            // [iterations]
    unsigned long long* stats;         // traversal / neighbour counters
    unsigned* fb_list;                 // uncertified queries (exact fallback) + their count
    unsigned* fb_count;
    RansacFrame rf;                    // RANSAC scratch (solve_method RANSAC), else zero
    int recompute_normals;             // map normals (count mode) to compute into t.mnr before the batch
};

// The batched kernels' view of their frame's record.  A pointer loaded from the frame table is
// generic to the compiler, so every access through it was a FLAT load — counted on vmcnt and lgkmcnt
// alike, so consuming one also waits for the kernel's LDS traffic, and a flat load after an LDS store
// it might alias waits for that store (k_knn_wave_b 181 vs k_knn_wave 166 µs per launch on config
// B's pair, profiles/r05_flat/).  The table holds HBM pointers only: device_view loads each pointer
// field as a global-address-space value, and the address-space inference turns every access through
// it into a global load.  (Host code never sees the qualifier: it is defined for the device pass only.)
#if defined(__HIP_DEVICE_COMPILE__)
#define IMLS_GAS __attribute__((address_space(1)))
#else
#define IMLS_GAS
#endif
__device__ __forceinline__ const void* gfield(const void* base, size_t off) {
    typedef const void IMLS_GAS* gvp;
    return (const void*)*reinterpret_cast<const gvp*>(reinterpret_cast<const char*>(base) + off);
}
#define IMLS_GLOBAL_FIELD(A, pa, f) (A).f = (decltype((A).f))gfield((pa), offsetof(PairDev, f))
__device__ __forceinline__ PairDev device_view(const PairDev* pa) {
    PairDev A = *pa;
    IMLS_GLOBAL_FIELD(A, pa, t.mpt); IMLS_GLOBAL_FIELD(A, pa, t.mnr); IMLS_GLOBAL_FIELD(A, pa, t.ipos);
    IMLS_GLOBAL_FIELD(A, pa, t.nodes); IMLS_GLOBAL_FIELD(A, pa, t.tpt); IMLS_GLOBAL_FIELD(A, pa, t.tnr);
    IMLS_GLOBAL_FIELD(A, pa, t.lkeys); IMLS_GLOBAL_FIELD(A, pa, t.qparams); IMLS_GLOBAL_FIELD(A, pa, t.mten);
    IMLS_GLOBAL_FIELD(A, pa, t.tvn);
    IMLS_GLOBAL_FIELD(A, pa, spt); IMLS_GLOBAL_FIELD(A, pa, snr); IMLS_GLOBAL_FIELD(A, pa, qperm);
    IMLS_GLOBAL_FIELD(A, pa, cs); IMLS_GLOBAL_FIELD(A, pa, cd); IMLS_GLOBAL_FIELD(A, pa, cn);
    IMLS_GLOBAL_FIELD(A, pa, lists); IMLS_GLOBAL_FIELD(A, pa, trace); IMLS_GLOBAL_FIELD(A, pa, stats);
    IMLS_GLOBAL_FIELD(A, pa, fb_list); IMLS_GLOBAL_FIELD(A, pa, fb_count);
    IMLS_GLOBAL_FIELD(A, pa, st.pose); IMLS_GLOBAL_FIELD(A, pa, st.delta); IMLS_GLOBAL_FIELD(A, pa, st.x0);
    IMLS_GLOBAL_FIELD(A, pa, st.done); IMLS_GLOBAL_FIELD(A, pa, st.status); IMLS_GLOBAL_FIELD(A, pa, st.iters);
    IMLS_GLOBAL_FIELD(A, pa, st.hist); IMLS_GLOBAL_FIELD(A, pa, st.coarse); IMLS_GLOBAL_FIELD(A, pa, st.cand_count);
    IMLS_GLOBAL_FIELD(A, pa, st.cand_lo); IMLS_GLOBAL_FIELD(A, pa, st.cand_lo_row); IMLS_GLOBAL_FIELD(A, pa, st.cand_hi);
    IMLS_GLOBAL_FIELD(A, pa, st.cand_hi_row); IMLS_GLOBAL_FIELD(A, pa, st.sel); IMLS_GLOBAL_FIELD(A, pa, st.partial1);
    IMLS_GLOBAL_FIELD(A, pa, st.partial2); IMLS_GLOBAL_FIELD(A, pa, st.keys); IMLS_GLOBAL_FIELD(A, pa, st.trace);
    IMLS_GLOBAL_FIELD(A, pa, st.info);
    return A;
}

// A rigid pose (rows 0-2 of the row-major 4×4) handed to a kernel by value: launch arguments live in
// the constant address space, so a wave reads it with one set of scalar loads (as transform_query's).
struct Pose12 { double T[12]; };
// float(P·[p;1]) and float(R·n) in transform_query's arithmetic (geom.h): double products summed in
// order, no contraction (the build's -ffp-contract=off), one rounding to float per component.
__device__ __forceinline__ void pose_point(const Pose12& P, float x, float y, float z, float nx, float ny, float nz,
                                           float o[3], float on[3]) {
    const double pd[3] = {x, y, z}, nd[3] = {nx, ny, nz};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double v = P.T[r * 4 + 0] * pd[0];
        v = v + P.T[r * 4 + 1] * pd[1];
        v = v + P.T[r * 4 + 2] * pd[2];
        v = v + P.T[r * 4 + 3] * 1.0;
        o[r] = (float)v;
        double w = P.T[r * 4 + 0] * nd[0];
        w = w + P.T[r * 4 + 1] * nd[1];
        w = w + P.T[r * 4 + 2] * nd[2];
        on[r] = (float)w;
    }
}

// voxel_map.hip — the voxel map's update (imls_voxel_map_update): candidates = the old
// map's rows then the scan's, one 64-bit voxel key each from the stored floats, a stable radix sort,
// the first `cap` rows of every key kept, gathered in that order into `out`.
struct VoxelGrid {                     // by value in the launches, as Pose12
    Pose12 P;                          // map ← scan
    double voxel;                      // double(voxel_size)
    double r2;                         // double(max_range)², +inf: no range test drops anything
    unsigned long long cap;            // max_per_voxel
    int identity;                      // the pose is exactly I: scan rows keep their bits
};
// the update's record, device and pinned host copy: words of VoxelRec
enum VoxelRec {
    kVoxKept = 0, kVoxVoxels, kVoxScanNonfinite, kVoxScanGrid, kVoxScanRange, kVoxScanFull, kVoxMapGrid, kVoxMapRange,
    kVoxMapTrimmed, kVoxRecWords = 16
};
// map: SoA6 [6][n_old]; scan_in: SoA6 [6][n] in the scan frame; scan_out: [6][n], receives the scan in
// the map frame (may be scan_in); out: ≥ 6·(n_old + n) floats, receives the new map as SoA6 [6][kept].
// h_rec (pinned, kVoxRecWords words) is valid once the stream has passed the call.
int voxel_map_merge(hipStream_t s, const float* map, size_t n_old, const float* scan_in, float* scan_out, size_t n,
                    const VoxelGrid& g, float* out, DevBuf& scratch, unsigned* h_rec, std::string& err);

// project.hip
// k_knn_wave → k_finish (+ the exact k_project_lane fallback for uncertified queries); lane_mode
// runs every query through k_project_lane.  partial1 receives project_blocks(N) slabs.
struct ProjectLaunch {
    TreeView t;
    const float4 *spt, *snr;
    const unsigned* qperm;
    int N;
    const double* pose;
    const int* done;
    const double* delta;               // last pose increment (read when use_prev)
    KParams kp;
    float4 *cs, *cd, *cn;
    double* partial1;                  // project_blocks(N) slabs
    imls_iter_trace* tr;               // the iteration's trace slot
    unsigned long long* stats;
    unsigned *fb_list, *fb_count;
    int* lists;                        // the frame's list block (ListBlock), kept across ICP iterations (temporal seed)
    int lane_mode, use_prev;
    hipEvent_t* marks;                 // 3 events recorded before k_knn_wave, between it and k_finish, and
                                       // after k_finish (timing), or null
};
#pragma GCC visibility push(hidden)
void launch_project(hipStream_t s, const ProjectLaunch& L);
#pragma GCC visibility pop
constexpr int kMaxKL = 46;       // list entries per query at most (the lone-frame path: K + 12 for K ≤ 32, capped)
// The list block of a frame of N queries whose lists hold KL entries: the positions pos[KL][N] (row
// pitch N) with the worst keys wlist[N] as row KL, then — after kMaxKL + 1 rows, whatever KL is — the
// per-query reference position + list guarantee xref[N] and the key the list's answer relied on
// nref[N]; a kNN query set's block ends with the deferred queries' search caps[N].  256-B aligned parts.
struct ListBlock {
    int* pos;
    float* wlist;
    float4* xref;
    float* nref;
    float* caps;                       // kNN blocks only (knn_list_bytes)
    static __host__ __device__ size_t part(size_t bytes) { return (bytes + 255) / 256 * 256; }
    static __host__ __device__ size_t pos_bytes(int N) { return part((size_t)(kMaxKL + 1) * N * 4); }
    static __host__ __device__ size_t bytes(int N) { return pos_bytes(N) + part((size_t)N * 20) + 512; }
};
__host__ __device__ inline ListBlock list_block(int* lists, int N, int KL) {
    ListBlock b;
    b.pos = lists;
    b.xref = reinterpret_cast<float4*>(reinterpret_cast<char*>(lists) + ListBlock::pos_bytes(N));
    b.wlist = reinterpret_cast<float*>(lists + (size_t)KL * N);
    b.nref = reinterpret_cast<float*>(b.xref + N);
    b.caps = reinterpret_cast<float*>(reinterpret_cast<char*>(lists) + ListBlock::bytes(N));
    return b;
}
inline size_t prevnn_bytes(int N) { return ListBlock::bytes(N); }
// Public kNN query (imls_knn / imls_knn_device): the same two stages over a query set of its own.
// knn_prepare: queries (component c of point i at src[i·pstride + c·cstride]) → qpt[n] (xyz, flag:
// a non-finite query is parked at the target's box corner with flag 1 — the tree never sees a NaN
// — and gets an all-unfound row), and the identity pose the traversal kernels read.
void knn_prepare(hipStream_t s, const TreeView& t, const float* src, size_t pstride, size_t cstride, int n, float4* qpt,
                 double* pose);
// Stage 1 (k_knn_wave / k_knn_qwave, unchanged) at the identity pose, then k_knn_export and the exact
// k_knn_export_lane over its deferred queries; lane_mode: every query through k_knn_export_lane.
// Outputs: rows [n][K] of (filtered index, fp64 d²) ascending by (d², index), unfound slots (−1, +∞),
// found[n] (nullable).  lists: knn_list_bytes(n) bytes; fb_count / fb_list as k_finish's.
struct KnnArgs {
    int K;
    double r2;                         // acceptance: d² ≤ r2 (+∞: unbounded)
    int allow_self;                    // 0: entries with d² ≤ DBL_EPSILON are dropped
    int qwave, force_fb;               // KParams::qwave / force_fb
};
void launch_knn(hipStream_t s, const TreeView& t, const float4* qpt, const unsigned* qperm, int n, const double* pose,
                const KnnArgs& a, int lane_mode, int* lists, unsigned* fb_list, unsigned* fb_count, int32_t* idx_out,
                double* d2_out, int32_t* found_out);
// list block of n kNN queries (ListBlock; xref / nref: the traversal's Verlet outputs, unread here)
inline size_t knn_list_bytes(int n) { return ListBlock::bytes(n) + ListBlock::part((size_t)n * 4); }
constexpr int kKnnChunk = 1 << 18;     // queries per launch sequence of imls_knn (larger sets: consecutive chunks)

constexpr int kStatSkipped = 6;   // nbr_stats slot: lanes whose list was reused without traversal
int project_blocks(int N);
constexpr int kPass1Block = 256;       // queries per k_finish block (one pass-1 slab each)
constexpr int kPass1Fallback = 64;     // k_project_lane fallback blocks (one slab each, after the k_finish slabs)
// Batched projection: one launch per kernel for all `npairs` frames of tab (device), iteration
// `it` (trace slot), every frame at its own pose / done flag.  n_host: the frames' N (grid shapes).
void launch_project_batch(hipStream_t s, const PairDev* tab, const int* n_host, int npairs, const KParams& kp, int it,
                          int use_prev);

// sizes of the solve chain that the projection and the API read (the solver's launchers: solve.h)
constexpr int kQwaveAutoN = 16384;  // auto traversal choice: one wave per query up to this many queries
constexpr int kSmallRows = 4096;    // float-row frames up to this are solved by one block (k_solve_small)
__host__ __device__ __forceinline__ int solve_blocks(int N) { return (N + kBlock - 1) / kBlock; }   // row blocks of the grid chain

// normals.hip — map normals recomputed from the map (get_normals=false, count mode), Morton order
int launch_map_normals(hipStream_t s, const TreeView& t, int K, double r_normal, float4* out);
int launch_map_normals_batch(hipStream_t s, const PairDev* tab, int npairs, int maxM, int K, double r_normal);

// tv.hip — tensor voting (VoteForAny, imls_icp.cpp:171-296): the voted normal of every source point
// at the current pose → tvn[N]; input tensors gathered to Morton order once per target
void launch_tv_vote(hipStream_t s, const TreeView& t, const float4* spt, int N, const double* pose, const int* done,
                    const KParams& kp, double4* tvn, int use_prev);
void launch_tensor_gather(hipStream_t s, const float* ten6_in, size_t n_in, const unsigned* kept, const float4* mpt, int M,
                          float4* mten);
void launch_tv_vote_batch(hipStream_t s, const PairDev* tab, const int* n_host, int npairs, const KParams& kp,
                          int use_prev);

// Transfer accounting of a producer call (imls_sweep_info): bytes copied each way and host waits.
struct Xfer {
    uint64_t h2d = 0, d2h = 0, syncs = 0;
};

// scanreg.hip — ring-neighbourhood PCA normals + geometric-features presample (imls_ring_normals_pca)
// Device form: the cloud as float4 (x, y, z, ·) in HBM (d_pts; null: h_pts is uploaded), the rows
// left in `mem` (valid until its next use).  Host traffic: the ring offsets and the block table up,
// 24 bytes of counts down behind one wait.
struct PcaDev {
    const unsigned* idx;
    const float *nrm, *ev, *evec, *feat;
    const unsigned char* fl;
    const int* ring_off;               // [n_rings + 1]
    size_t rows;
    int n;
};
int ring_pca_dev(hipStream_t s, const imls_pca_params& p, const float4* d_pts, const float4* h_pts, const int32_t* sizes,
                 int n_rings, DevBuf& mem, hipEvent_t* marks, PcaDev* out, uint64_t counters[2], std::string& err,
                 Xfer* x = nullptr);
int ring_pca_run(hipStream_t s, const imls_pca_params& p, const float* xyz, size_t stride, const int32_t* sizes,
                 int n_rings, DevBuf& mem, hipEvent_t* marks, uint32_t* index_out, float* normal_out,
                 float* evals_out, float* evecs_out, float* features_out, uint8_t* flags_out, size_t* n_out,
                 uint64_t counters[2], std::string& err);

// front.hip — scan front end: NaN + range filter, ring assignment, relative time (imls_scan_front_end)
// Device form: the sweep as SoA xyz [3][n] in HBM (d_soa3; null: h_soa3 is uploaded), laserCloud
// left in `mem` as (x, y, z, intensity) records with the input index of each.  One wait, 288 bytes
// of counts down.
struct FrontDev {
    const float4* out;
    const unsigned* idx;
};
int front_end_dev(hipStream_t s, const imls_front_params& p, const float* d_soa3, const float* h_soa3, size_t n_in,
                  DevBuf& mem, FrontDev* out, int32_t* ring_sizes, size_t* n_out, std::string& err, Xfer* x = nullptr);
int front_end_run(hipStream_t s, const imls_front_params& p, const float* xyz_host, size_t stride, size_t n_in,
                  DevBuf& mem, float* out_xyzi, uint32_t* out_index, int32_t* ring_sizes, size_t* n_out,
                  std::string& err);

// sample.hip — samplePointCloud "normal" / "major_axis" (imls_sample_point_cloud)
int sample_run(hipStream_t s, const imls_sample_params& p, const float* xyz, const float* nrm, size_t stride, size_t n,
               const int32_t* cand, size_t n_cand, const float* last_xyz, size_t last_stride, size_t m, DevBuf& mem,
               hipEvent_t* marks, int32_t* sampled_out, size_t* n_sampled, float* bin_weights_out, std::string& err);
// the two sampling kernels on device buffers (sweep.hip reuses them)
struct FpsJob {
    int off, n, k, first, out;   // points [off, off+n) of the packed bin clouds; k samples → out[out, out+k); n = 0: no job
};
void launch_major_avg(hipStream_t s, const float4* spt, const float4* snr, int ns, const float4* last, int m,
                      const float4* cbox, float r, float r_proj, int* cnt_out, float* avg_out);
void launch_fps(hipStream_t s, const float4* pts, const FpsJob* jobs, int n_jobs, double* md, unsigned char* taken, int* out);
// randomSampling's shuffle (566-582) as positions: std::shuffle permutes positions whatever the
// contents, so the first min(k, size) entries of the shuffled 0 … size−1 index any bin of that size
void shuffle_positions(uint32_t seed, int size, int k, std::vector<int>& out);
// randomSampling (566-582) alone: the first min(max_points, n_cand) entries of the seeded shuffle
void sample_random_host(const int32_t* cand, size_t n_cand, int32_t max_points, uint32_t shuffle_seed,
                        int32_t* sampled_out, size_t* n_sampled);

// presample.hip — curvature presample (imls_presample_curvature)
int presample_curvature_run(hipStream_t s, const imls_curvature_params& p, const float* xyz, size_t stride,
                            const int32_t* sizes, int n_rings, const uint32_t* row_index, const uint8_t* row_flags,
                            size_t n_rows, DevBuf& mem, hipEvent_t* marks, float* curvature_out, int32_t* candidates_out,
                            size_t* n_cand, std::string& err);

// the stencil and the candidate compaction on device buffers: curv [n], keep / pos / cand [n_rows]
void curvature_enqueue(hipStream_t s, const imls_curvature_params& p, const float4* pts, const int* ring_off, int n_rings,
                       int n, const unsigned* row_index, const unsigned char* row_flags, int n_rows, float* curv,
                       unsigned* keep, unsigned* pos, int* cand, void* cub_tmp, size_t cub_bytes);

// three_axis.hip — threeAxisSampling (imls_sample_three_axis)
// keys and per-list top-k on device buffers: ga / gb [nc] float4, gc [nc] float2 (k_ta_keys' inputs),
// keys [9·nc], out [9·k], nan [1] (zeroed by the caller)
void three_axis_enqueue(hipStream_t s, const float4* ga, const float4* gb, const float2* gc, int nc, int k,
                        unsigned long long* keys, int* out, unsigned long long* nan);
int three_axis_run(hipStream_t s, int points_per_list, const float* xyz, const float* nrm, size_t stride, size_t n,
                   const float* evals, const int32_t* cand, size_t n_cand, DevBuf& mem, hipEvent_t* marks,
                   int32_t* sampled_out, size_t* n_sampled, uint64_t* nan_keys, std::string& err);

// deskew.hip — per-point motion compensation from relTime (imls_deskew, imls_sweep_set_motion;
// TransformToStart / TransformToEnd, laser_odometry.cpp:62-114).  The motion (start ← end) as the
// kernel takes it, by value like Pose12: rotation axis and angle, translation, Rᵀ (row-major).
struct DeskewArg {
    double a[3], theta, t[3], Rt[9];
    int to_start;                      // IMLS_DESKEW_TO_START: stop at the sweep-start frame
};
// The host work of one call: IMLS_ERR_ARG (err set) for a non-finite entry or θ ≥ π/2; *identity
// when M is exactly I (the caller then launches nothing).
int deskew_prepare(const double M[16], int to_frame, DeskewArg* out, bool* identity, std::string& err);
// (x, y, z, intensity) records and, nullable, (nx, ny, nz, ·) records, in place on stream s
void deskew_enqueue(hipStream_t s, const DeskewArg& A, float scan_period, float4* xyzi, float4* nrm, size_t n);
// host arrays of any stride: pack, upload, the same launch, download (floats past the 4th / 3rd kept)
int deskew_host(hipStream_t s, const DeskewArg& A, float scan_period, float* xyzi, size_t stride, size_t n, float* nrm,
                size_t nstride, DevBuf& mem, hipEvent_t* marks, std::string& err);

// sweep.hip — a raw sweep to pcl_cloud / pcl_surface_cloud in HBM (imls_sweep_process) and the
// sampler stage on device inputs (imls_sample_point_cloud_device)
struct SweepSet {                      // one of the two rotating cloud sets
    DevBuf soa6, side, flat, rows, prev4, cbox;   // side: intensity [n] | curvature [n]
    size_t n_filtered = 0, n_flat = 0, cap_filtered = 0;
};
struct SweepState {
    SweepSet set[2];
    int cur = 0;                       // the set holding the last sweep's clouds
    bool has = false;                  // a sweep ran since creation / reset
    uint64_t counter = 1;              // scan_registration.cpp:64
    bool deskew_on = false;            // imls_sweep_set_motion: deskew the front end's records with `deskew`
    DeskewArg deskew{};
    DevBuf raw, raw3, cand, scratch, rec;
};
// Launch kinds of the timing ABI (imls_kernel_timing / imls_timing_intervals, and the Python side):
// the values are public (include/imls_gpu.h documents each) and do not change.
enum TimingKind {
    kTimeProject = 0,     // projection (all its kernels)
    kTimeIndex = 1,       // index build (all its kernels)
    kTimeSolve = 2,       // solve chain
    kTimeKnnWave = 3,     // k_knn_wave alone
    kTimeFinish = 4,      // k_finish alone
    kTimeRingPca = 5,     // k_ring_pca
    kTimeMajorAvg = 6,    // k_major_avg
    kTimeFrontEnd = 7,    // imls_scan_front_end
    kTimeKnnQuery = 8,    // imls_knn / imls_knn_device
    kTimeThreeAxis = 9,   // imls_sample_three_axis
    kTimeCurvature = 10,  // imls_presample_curvature
    kTimeSweep = 11,      // sweep sampler / compaction / cloud assembly (recorded by sweep.hip)
    kTimeDeskew = 12,     // deskew kernel
    kTimePoseInfo = 13,   // pose-info kernels (k_info_rows, k_info_final)
    kTimeVoxelMap = 14,   // voxel-map update (keys, sort, cap, gather)
    kTimingKinds = 15
};
// timing hook of the caller: a pair of events that will be harvested as `kind`, or false (timing off)
typedef bool (*SweepMark)(void* owner, int kind, hipEvent_t ev[2]);
struct SweepEnv {
    hipStream_t s;
    DevBuf *front_mem, *pca_mem;
    SweepMark mark;
    void* owner;
    std::string* err;
};
int sweep_run(SweepEnv& e, SweepState& st, const imls_sweep_params& p, const float* h_xyz, const float* d_xyz,
              size_t stride, size_t n, imls_sweep_info* info);
int sweep_download(SweepEnv& e, SweepState& st, int which, void* records, size_t cap, size_t* n, int32_t* sampled_index);
int sampler_run(SweepEnv& e, SweepState& st, const imls_sample_params& p, const float* d_soa6, size_t n,
                const int32_t* d_cand, size_t n_cand, const float* d_last_soa6, size_t m, int32_t* d_sampled,
                size_t* n_sampled, float* d_weights, uint64_t* nan_normals);
std::vector<DevBuf*> sweep_buffers(SweepState& st);

}  // namespace imlsgpu
