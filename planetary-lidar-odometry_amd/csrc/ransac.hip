// ransac.hip — SolveMotionEstimationProblemRANSAC (solver.cpp:222-385) with farthestPointSampling
// (common.cpp:19-82) on device.  The row compaction is compact_rows.hip, the DRPM final drpm.hip.
//
// Data flow per RANSAC solve (all on the context's stream, no host sync):
//   1. the valid correspondences (float rows, source order) are compacted, order kept, into fp64
//      rows S/D/N — the reference's std::vector<Vector3d> inputs; the TOO_FEW gate
//      (laser_odometry.cpp:570-576) runs on their count;
//   2. hypotheses in chunks (ransac_chunks): k_ransac_hyp runs one hypothesis per block at
//      a time — its glibc rand() draw (the FPS start index) by the jump table below, FPS (two
//      arg-max passes, first index wins ties as the sequential `>` does), the 3×6 column-pivoted
//      Householder QR basic solution (Eigen ColPivHouseholderQR, not normal equations: a rank-3
//      system squared would misjudge the rank), Δ, and the inlier count; k_ransac_select (one
//      wave) scans the chunk in order with the reference's strict `>` and early exit
//      (best > ⌊pct·N⌋) and commits exactly the draws consumed; later chunks return at once;
//   3. inliers of the best Δ are compacted (order kept) with weights
//      w = √a < h₂ ? a : 2h₂√a − h₂², a = e^{−|r|}, h₂ = huber·distance (solver.cpp:334-356),
//      normalised by Σw (361-364; the division happens where the weight is read);
//   4. final solve: LS (trimmed, RANSAC's own threshold) / weighted LS through the LS chain on the
//      fp64 inlier rows, or DRPM (launch_drpm).
// Batched frames (imls_register_frames, launch_ransac_batch): every step above is one launch for
// all frames (grid y = frame, the same bodies; each frame keeps its own count, rand() stream, chunk
// progress and done flag).
// The rand() jump table is a __device__ variable, which belongs to one unit (the library is built
// without relocatable device code): its readers — the hypothesis kernels, the select kernels and
// k_drpm_head_small, which runs the select body — live here, as does the debug build's g_dbg_ransac.
#include <algorithm>
#include <mutex>
#include <vector>

#include "compact_rows.h"
#include "drpm_common.h"

namespace imlsgpu {
namespace {

// threads per hypothesis: one wave for small frames (its serial part — QR, Δ by one lane — then
// overlaps with other hypotheses on the same CU instead of idling three more waves), four for
// large ones (the three passes over the rows dominate).  Exact either way (arg-max and counts).
constexpr int kHypSmallRows = 4096;
__host__ __device__ constexpr int hyp_block_of(int cap) { return cap <= kHypSmallRows ? 64 : 256; }
constexpr int kHypUnroll = 8;        // FPS passes: rows per thread whose loads are in flight together
constexpr int kHypGrid = 8192;        // batched hypothesis grid (blocks stride over the running frames' items)
#ifdef IMLS_DEBUG_WAVE_TRACE
// phase clocks (100 MHz ticks) of block 0's hypothesis [0..5] and of k_drpm_head_small [8..13];
// [6], [14]: call counts (tools/ransac_probe.py with the debug build)
__device__ unsigned long long g_dbg_ransac[16];
#define RSTAMP(k) do { if (dbg_on) { g_dbg_ransac[k] += wall_clock64() - dbg_t; dbg_t = wall_clock64(); } } while (0)
#else
#define RSTAMP(k) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------------
// glibc random() TYPE_3 (what rand() returns): state = a ring of 31 words + front / rear indices
// (st[31], st[32]; rear = front − 3 mod 31).  rand() adds ring[rear] into ring[front], returns that
// word >> 1 and advances both: the word sequence is x_i = x_{i−31} + x_{i−3} (mod 2^32), and with
// s_j = ring[(front + j) % 31] = x_{i−31+j} the k-th next word is x_{i+k} = Σ_j C[k][j]·s_j (mod 2^32)
// for fixed integer rows C[k] (C[m−31] = e_m for m < 31, C[k] = C[k−31] + C[k−3]).  So the draw of
// every hypothesis of a chunk is an independent 31-term dot product with the committed state (no
// serial replay), and committing `used` draws rebuilds the ring in one parallel step.  Integer
// arithmetic mod 2^32: exact in any summation order.
// ---------------------------------------------------------------------------------------------
__device__ unsigned g_rand_jump[kHypMax * 31];   // C[k][j], k < kHypMax (host-built, ransac_init_tables)

// x_{i+k} from the committed state; called by a whole wave (lanes < 31 hold one term each)
__device__ __forceinline__ unsigned rand_word_ahead(const int* __restrict__ st, int k) {
    const int lane = threadIdx.x & 63;
    unsigned term = 0u;
    if (lane < 31) {
        const int f = st[31];
        term = g_rand_jump[(size_t)k * 31 + lane] * (unsigned)st[(f + lane) % 31];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) term += (unsigned)__shfl_xor((int)term, o, 64);
    return term;
}

// commit `used` draws: ring'[(front + used + j) % 31] = x_{i+used−31+j}; called by one whole wave
__device__ __forceinline__ void rand_commit(int* __restrict__ st, int used) {
    const int lane = threadIdx.x & 63;
    const int f = st[31], r = st[32];
    const unsigned sj = lane < 31 ? (unsigned)st[(f + lane) % 31] : 0u;   // s_j in lane j
    unsigned sv[31];                                                      // … and in every lane
#pragma unroll
    for (int j = 0; j < 31; ++j) sv[j] = (unsigned)__builtin_amdgcn_readlane((int)sj, j);
    const unsigned kept = (unsigned)__shfl((int)sj, used + lane, 64);     // x_{i+used−31+j} = s_{used+j}
    const int idx = used - 31 + lane;
    unsigned acc = 0u;
    if (lane < 31 && idx >= 0) {
#pragma unroll
        for (int j = 0; j < 31; ++j) acc += g_rand_jump[(size_t)idx * 31 + j] * sv[j];
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 31) st[(f + used + lane) % 31] = (int)(idx < 0 ? kept : acc);
    if (lane == 0) { st[31] = (f + used) % 31; st[32] = (r + used) % 31; }
}

// the valid-row compaction's post step on its own (host fp64 rows arrive compact): the gate on the
// count and the reset of the selection state
__global__ void k_ransac_begin(const int* __restrict__ count, int correspond_number, int update_pose, SolveState st,
                               imls_iter_trace* tr, RansacDev R) {
    const CompactPost P{1, correspond_number, update_pose, st, tr, R};
    if (threadIdx.x || compact_skip(P)) return;
    compact_post(P, *count);
}

// block arg-max of (value, index): larger value, then smaller index
template <int NT>
__device__ __forceinline__ void argmax_pair(double& v, int& i, double* sv, int* si) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { sv[wv] = v; si[wv] = i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < NT / 64; ++k)
            if (sv[k] > sv[0] || (sv[k] == sv[0] && si[k] < si[0])) { sv[0] = sv[k]; si[0] = si[k]; }
    }
    __syncthreads();
    v = sv[0];
    i = si[0];
    __syncthreads();
}

// Eigen ColPivHouseholderQR(3×6).solve(b): basic solution (free unknowns zero), by one wave.  Lane
// c < 6 holds column c of A (a[r] = A[r][c]) with its norms and original index: the pivot search
// reads the six norms, a swap exchanges two lanes' columns, the Householder vector of column k is
// formed by every lane from lane k's column (the same scalar expressions, so the same bits
// everywhere), and the update and the norm downdate of the columns right of k run on their own
// lanes — Eigen's operations in Eigen's order, each on the lane that owns the column, so x is the
// sequential routine's result bit for bit.  The back-substitution (3×3) runs on every lane from the
// gathered factor.  (The QR on a single lane took 4.8 µs per hypothesis block, tools/ransac_probe.py
// phase clocks.)
__device__ void colpiv_qr3_wave(double a[3], double b[3], double x[6]) {
    constexpr int RR = 3, C = 6, S = 3;
    const int lane = threadIdx.x & 63;
    const double eps = DBL_EPSILON;
    double nu, nd;
    int perm = lane;
    {
        double sq = 0;
#pragma unroll
        for (int r = 0; r < RR; ++r) sq += a[r] * a[r];
        nu = nd = sqrt(sq);
    }
    double maxnorm = 0;
#pragma unroll
    for (int k = 0; k < C; ++k) maxnorm = fmax(maxnorm, readlane_f64(nu, k));
    const double thr_helper = (maxnorm * eps) * (maxnorm * eps) / (double)RR;
    const double ndt = sqrt(eps);
    int nonzero = S;
    double maxpivot = 0;
    double hc[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        int big = k;
        double bv = readlane_f64(nu, k);
#pragma unroll
        for (int j = k + 1; j < C; ++j) {
            const double nj = readlane_f64(nu, j);
            if (nj > bv) { bv = nj; big = j; }
        }
        if (nonzero == S && bv * bv < thr_helper * (double)(RR - k)) nonzero = k;
        if (big != k) {                       // wave-uniform: exchange the columns of lanes k and big
            double ak[RR], ab[RR];
#pragma unroll
            for (int r = 0; r < RR; ++r) { ak[r] = readlane_f64(a[r], k); ab[r] = readlane_f64(a[r], big); }
            const double nuk = readlane_f64(nu, k), nub = readlane_f64(nu, big);
            const double ndk = readlane_f64(nd, k), ndb = readlane_f64(nd, big);
            const int pk = __builtin_amdgcn_readlane(perm, k), pb = __builtin_amdgcn_readlane(perm, big);
            if (lane == k) {
#pragma unroll
                for (int r = 0; r < RR; ++r) a[r] = ab[r];
                nu = nub; nd = ndb; perm = pb;
            } else if (lane == big) {
#pragma unroll
                for (int r = 0; r < RR; ++r) a[r] = ak[r];
                nu = nuk; nd = ndk; perm = pk;
            }
        }
        // makeHouseholderInPlace on column k, rows k..RR−1 (every lane, from lane k's column)
        double col[RR];
#pragma unroll
        for (int r = 0; r < RR; ++r) col[r] = readlane_f64(a[r], k);
        const double c0 = col[k];
        double tail = 0;
#pragma unroll
        for (int r = k + 1; r < RR; ++r) tail += col[r] * col[r];
        double tau, beta, v[RR];
        if (tail <= DBL_MIN) {
            tau = 0;
            beta = c0;
#pragma unroll
            for (int r = k + 1; r < RR; ++r) v[r] = 0;
        } else {
            beta = sqrt(c0 * c0 + tail);
            if (c0 >= 0) beta = -beta;
#pragma unroll
            for (int r = k + 1; r < RR; ++r) v[r] = col[r] / (c0 - beta);
            tau = (beta - c0) / beta;
        }
        hc[k] = tau;
        if (lane == k) {
            a[k] = beta;
#pragma unroll
            for (int r = k + 1; r < RR; ++r) a[r] = v[r];
        }
        if (fabs(beta) > maxpivot) maxpivot = fabs(beta);
        if (lane > k && lane < C) {
            if (tau != 0) {
                double tmp = a[k];
#pragma unroll
                for (int r = k + 1; r < RR; ++r) tmp += v[r] * a[r];
                a[k] -= tau * tmp;
#pragma unroll
                for (int r = k + 1; r < RR; ++r) a[r] -= tau * v[r] * tmp;
            }
            if (nu != 0) {
                double temp = fabs(a[k]) / nu;
                temp = (1 + temp) * (1 - temp);
                temp = temp < 0 ? 0 : temp;
                const double r2 = nu / nd;
                const double temp2 = temp * r2 * r2;
                if (temp2 <= ndt) {
                    double sq = 0;
#pragma unroll
                    for (int r = k + 1; r < RR; ++r) sq += a[r] * a[r];
                    nd = nu = sqrt(sq);
                } else {
                    nu *= sqrt(temp);
                }
            }
        }
    }
    // the factor's first S columns and the permutation, on every lane; the one-lane solve from here
    double A[RR][S];
    int pm[S];
#pragma unroll
    for (int c = 0; c < S; ++c) {
#pragma unroll
        for (int r = 0; r < RR; ++r) A[r][c] = readlane_f64(a[r], c);
        pm[c] = __builtin_amdgcn_readlane(perm, c);
    }
    const double thr = eps * (double)S;
    int nz = 0;
#pragma unroll
    for (int i = 0; i < S; ++i) nz += (i < nonzero && fabs(A[i][i]) > thr * maxpivot) ? 1 : 0;
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = 0;
    if (nz == 0) return;
#pragma unroll
    for (int k = 0; k < S; ++k) {
        if (k < nz) {
            const double tau = hc[k];
            if (RR - k == 1) {
                b[k] *= 1 - tau;
            } else if (tau != 0) {
                double tmp = b[k];
#pragma unroll
                for (int r = k + 1; r < RR; ++r) tmp += A[r][k] * b[r];
                b[k] -= tau * tmp;
#pragma unroll
                for (int r = k + 1; r < RR; ++r) b[r] -= tau * A[r][k] * tmp;
            }
        }
    }
#pragma unroll
    for (int i = S - 1; i >= 0; --i) {
        if (i < nz) {
            double sacc = b[i];
#pragma unroll
            for (int j = i + 1; j < S; ++j)
                if (j < nz) sacc -= A[i][j] * b[j];
            b[i] = sacc / A[i][i];
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        double val = 0;
#pragma unroll
        for (int i = 0; i < S; ++i)
            if (i < nz && pm[i] == c) val = b[i];
        x[c] = val;
    }
}

// Hypothesis h of the current chunk, by one block: its draw (the FPS start) from the committed
// rand() state, FPS(3), the 3×6 QR, Δ, its inlier count.
template <int NT>
__device__ __forceinline__ void ransac_hyp_one(const double* __restrict__ S, const double* __restrict__ Dp,
                                               const double* __restrict__ Np, int n, const RansacDev& R,
                                               double dist_thr, int h) {
    __shared__ double sv[NT / 64];
    __shared__ int si[NT / 64];
    __shared__ double T[16];
    __shared__ int cnt_s[NT / 64];
#ifdef IMLS_DEBUG_WAVE_TRACE
    const bool dbg_on = blockIdx.x == 0 && threadIdx.x == 0 && h == 0;
    long long dbg_t = wall_clock64();
    if (dbg_on) g_dbg_ransac[6] += 1;
#endif
    const int f0 = (int)(rand_word_ahead(R.rng, h) >> 1) % n;   // rand() % n (solver.cpp / common.cpp:49)
    // The two FPS passes: the taken points' coordinates in registers, each thread's rows in groups of
    // kHypUnroll whose loads are all issued before the first compare (round 6: the loop reloaded
    // s_f0 and waited on every row's load in turn — one L2 round trip per row, the lone frame's
    // k_ransac_hyp 31 µs per chunk).  A thread still visits its rows in ascending order and keeps the
    // first maximum (strict `>`), so the arg-max — larger value, then smaller index — is unchanged.
    const double a0 = S[3 * (size_t)f0], a1 = S[3 * (size_t)f0 + 1], a2 = S[3 * (size_t)f0 + 2];
    auto dist = [](double x0, double x1, double x2, const double (&b)[3]) {   // pdist(s, a, b): ‖s_a − s_b‖
        const double dx = x0 - b[0], dy = x1 - b[1], dz = x2 - b[2];
        return sqrt((dx * dx + dy * dy) + dz * dz);
    };
    auto load_rows = [&](int i0, double (&p)[kHypUnroll][3]) {
#pragma unroll
        for (int u = 0; u < kHypUnroll; ++u) {
            const size_t i3 = 3 * (size_t)min(i0 + u * NT, n - 1);
            p[u][0] = S[i3]; p[u][1] = S[i3 + 1]; p[u][2] = S[i3 + 2];
        }
    };
    // pass 1: farthest from f0 (common.cpp:48-66: strict `>` from −1, taken points skipped)
    double bv = -1.0;
    int bi = 0x7fffffff;
    for (int i0 = threadIdx.x; i0 < n; i0 += kHypUnroll * NT) {
        double p[kHypUnroll][3];
        load_rows(i0, p);
#pragma unroll
        for (int u = 0; u < kHypUnroll; ++u) {
            const int i = i0 + u * NT;
            if (i >= n || i == f0) continue;
            const double md = dist(a0, a1, a2, p[u]);
            if (md > bv) { bv = md; bi = i; }
        }
    }
    argmax_pair<NT>(bv, bi, sv, si);
    RSTAMP(0);
    const int f1 = bi;
    // pass 2: farthest from {f0, f1} by the running minimum distance
    const double c0 = S[3 * (size_t)f1], c1 = S[3 * (size_t)f1 + 1], c2 = S[3 * (size_t)f1 + 2];
    bv = -1.0;
    bi = 0x7fffffff;
    for (int i0 = threadIdx.x; i0 < n; i0 += kHypUnroll * NT) {
        double p[kHypUnroll][3];
        load_rows(i0, p);
#pragma unroll
        for (int u = 0; u < kHypUnroll; ++u) {
            const int i = i0 + u * NT;
            if (i >= n || i == f0 || i == f1) continue;
            const double md = fmin(dist(a0, a1, a2, p[u]), dist(c0, c1, c2, p[u]));
            if (md > bv) { bv = md; bi = i; }
        }
    }
    argmax_pair<NT>(bv, bi, sv, si);
    RSTAMP(1);
    const int f2 = bi;
    if (threadIdx.x < 64) {                   // wave 0: lane c builds column c of the 3×6 system
        const int id[3] = {f0, f1, f2};
        const int lane = threadIdx.x, cc = lane < 6 ? lane : 0;
        double a[3], b[3], x[6];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int k = id[r];
            const double s0 = S[3 * k], s1 = S[3 * k + 1], s2 = S[3 * k + 2];
            const double d0 = Dp[3 * k], d1 = Dp[3 * k + 1], d2 = Dp[3 * k + 2];
            const double n0 = Np[3 * k], n1 = Np[3 * k + 1], n2 = Np[3 * k + 2];
            const double col[6] = {n2 * s1 - n1 * s2, n0 * s2 - n2 * s0, n1 * s0 - n0 * s1, n0, n1, n2};
            double v = col[0];
#pragma unroll
            for (int c = 1; c < 6; ++c) v = cc == c ? col[c] : v;
            a[r] = v;
            double bb = n0 * (d0 - s0);
            bb = bb + n1 * (d1 - s1);
            bb = bb + n2 * (d2 - s2);
            b[r] = bb;
        }
        colpiv_qr3_wave(a, b, x);
        RSTAMP(2);
        if (lane == 0) {
            double D[16];
            delta_from_x(x, D);
            RSTAMP(3);
#pragma unroll
            for (int k = 0; k < 16; ++k) T[k] = D[k];
        }
    }
    __syncthreads();
    int c = 0;
    for (int i = threadIdx.x; i < n; i += NT) {
        const size_t i3 = 3 * (size_t)i;
        const double s0 = S[i3], s1 = S[i3 + 1], s2 = S[i3 + 2];
        double tp[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) tp[r] = ((T[r * 4] * s0 + T[r * 4 + 1] * s1) + T[r * 4 + 2] * s2) + T[r * 4 + 3];
        const double dist = fabs(((tp[0] - Dp[i3]) * Np[i3] + (tp[1] - Dp[i3 + 1]) * Np[i3 + 1]) + (tp[2] - Dp[i3 + 2]) * Np[i3 + 2]);
        c += dist < dist_thr ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) cnt_s[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int k = 0; k < NT / 64; ++k) tot += cnt_s[k];
        R.counts[h] = tot;
    }
    if (threadIdx.x < 16) R.T[(size_t)h * 16 + threadIdx.x] = T[threadIdx.x];
    RSTAMP(4);
}
// one frame: hypotheses blockIdx.x, blockIdx.x + gridDim.x, … of the chunk.
// base > 0 (a lone frame's second chunk, its hypotheses base … base + chunk − 1 of the same draw
// sequence): nothing is selected or committed between the chunks — every block first looks for a
// hypothesis of the first chunk above the inlier minimum (the first chunk's selection would have
// stopped RANSAC there) and leaves if there is one; one selection over both chunks follows (at the head
// of k_drpm_head_small), which is the two sequential selections' result: the first exceeding
// hypothesis ends the scan, the first maximum before it wins, exactly `used` draws are committed.
template <int NT>
__global__ __launch_bounds__(NT) void k_ransac_hyp(const double* __restrict__ rows, const int* __restrict__ count,
                                                   int cap, RansacDev R, double dist_thr, int chunk,
                                                   const int* __restrict__ done, int base, double min_pct) {
    if (*done || *R.rdone) return;
    const int n = *count;
    if (base > 0) {
        __shared__ int hit;
        const int min_inliers = (int)(min_pct * (double)n);   // as ransac_select_body
        if (threadIdx.x == 0) hit = 0;
        __syncthreads();
        for (int h = threadIdx.x; h < base; h += NT)
            if (R.counts[h] > min_inliers) hit = 1;
        __syncthreads();
        if (hit) return;
    }
    const size_t c3 = 3 * (size_t)cap;
    for (int h = blockIdx.x; h < chunk; h += gridDim.x)
        ransac_hyp_one<NT>(rows, rows + c3, rows + 2 * c3, n, R, dist_thr, base + h);
}

// Sequential semantics of the hypothesis loop (solver.cpp:244-326) over one chunk, by one wave: the
// loop stops at the first hypothesis whose count exceeds ⌊pct·N⌋ (best > min_inliers first holds
// there, since best ≤ min_inliers on entry); best / bestT follow the strict `>` (first maximum
// wins); exactly the draws consumed are committed.
__device__ __forceinline__ void ransac_select_body(const int* __restrict__ count, const RansacDev& R, int chunk,
                                                   int max_iterations, double min_pct) {
    const int lane = threadIdx.x & 63;
    const int n = *count;
    const int min_inliers = (int)(min_pct * (double)n);
    int best = *R.best, bi = -1, used = chunk;
    for (int base = 0; base < chunk; base += 64) {
        const int h = base + lane;
        const int c = h < chunk ? R.counts[h] : INT_MIN;
        const unsigned long long sm = __ballot(h < chunk && c > min_inliers);
        const int lim = sm ? (int)__builtin_ctzll(sm) : 63;
        int v = lane <= lim ? c : INT_MIN, vi = h;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int ov = __shfl_xor(v, o, 64), oi = __shfl_xor(vi, o, 64);
            if (ov > v || (ov == v && oi < vi)) { v = ov; vi = oi; }
        }
        if (v > best) { best = v; bi = vi; }
        if (sm) { used = base + lim + 1; break; }
    }
    if (bi >= 0 && lane < 16) R.bestT[lane] = R.T[(size_t)bi * 16 + lane];
    rand_commit(R.rng, used);                 // commit exactly the draws consumed
    if (lane == 0) {
        *R.best = best;
        const int evaluated = *R.evaluated + used;
        *R.evaluated = evaluated;
        if (used < chunk || best > min_inliers || evaluated >= max_iterations) *R.rdone = 1;
    }
}
__global__ __launch_bounds__(64) void k_ransac_select(const int* __restrict__ count, RansacDev R, int chunk,
                                                     int max_iterations, double min_pct, const int* __restrict__ done) {
    if (*done || *R.rdone) return;
    ransac_select_body(count, R, chunk, max_iterations, min_pct);
}

// RANSAC's own trace record behind an LS / weighted-LS final (the DRPM final writes it itself).
// Launched only with a trace slot: the body's null test (the stand-alone DRPM's) folds away.
__global__ void k_ransac_trace(const int* __restrict__ count_all, RansacDev R, imls_iter_trace* tr) {
    __builtin_assume(tr != nullptr);
    ransac_trace_t0(R, count_all, tr);
}

// ---------------------------------------------------------------------------------------------
// The lone frame's DRPM head in ONE launch (round 6; frames of ≤ kSmallRows rows registered alone,
// the config C/D deployment shape): the inlier compaction, pass 1 of the weighted normal equations
// over the inliers and the eigendecomposition — three launches before (k_compact_one, k_rows_pass1,
// k_drpm_eig) — preceded by the last hypothesis chunk's selection (k_ransac_select, round 6).  One
// 1024-thread block runs them between block barriers; pass 1 runs as "virtual blocks" — block b of
// k_rows_pass1's grid is done by the 256-thread group (b mod 4) in round b / 4, with the same
// thread ↔ row mapping, the same per-wave reductions and the same slab order, and the slab sum by
// the first 256 threads as k_drpm_eig does it — so every value is the chain's bit for bit: the
// row terms are block_normeq's (normeq_terms) and the H / g fill and the eigendecomposition are
// k_drpm_eig's (drpm_eig_tail), the same code (the batched frames keep the chain: alone and batched
// agree).  The noise terms and the solve stay
// grid / one-block launches: fused into this block as well (virtual noise blocks, measured) the
// frame's DRPM took 102.7 µs per ICP iteration against the chain's 70 (one CU for the noise phase,
// its registers at 2 waves per SIMD; profiles/r06_ransac/).
// ---------------------------------------------------------------------------------------------
constexpr int kHeadThreads = 1024;
struct SelectArgs {                   // the last hypothesis chunk's selection (k_ransac_select's arguments)
    const int* count;
    int chunk, max_iterations;
    double min_pct;
};
__global__ __launch_bounds__(kHeadThreads) void k_drpm_head_small(SelectArgs sel, Source isrc, int cap, CompactOut out,
                                                                  CompactPost P, Rows rows, int b1, SolveState st,
                                                                  DrpmDev Dv) {
    __shared__ double red_ne[kHeadThreads / 64][kNormEq];
    __shared__ double acc[kNormEq];
    // pass 1's slabs stay in LDS (round 6: through st.partial1 the slab sum waited on a global round trip)
    __shared__ double slab[kSmallRows / kBlock][kNormEq];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, grp = tid >> 8, t = tid & 255;
    if (compact_skip(P)) return;
#ifdef IMLS_DEBUG_WAVE_TRACE
    const bool dbg_on = tid == 0;
    long long dbg_t = wall_clock64();
    if (dbg_on) g_dbg_ransac[14] += 1;
#endif
    // 0. the last chunk's selection (k_ransac_select: skipped once RANSAC finished in an earlier chunk),
    // by wave 0; its bestT feeds the compaction below
    if (!*P.R.rdone) {
        if (tid < 64) ransac_select_body(sel.count, P.R, sel.chunk, sel.max_iterations, sel.min_pct);
        __threadfence_block();
        __syncthreads();
    }
    RSTAMP(8);
    // 1. the inliers of the best Δ with their weights (k_compact_one, kind 2: an empty set fails the solve)
    compact_one_body(isrc, cap, out, P);
    __threadfence_block();
    __syncthreads();
    RSTAMP(9);
    // 2. pass 1 over the inlier rows (k_rows_pass1<kBlock>, which runs whether or not the frame is done:
    // slab b = rows [256b, 256b + 256))
    for (int base = 0; base < b1; base += kHeadThreads / kBlock) {
        const int b = base + grp, i = b * kBlock + t;
        double a[6] = {0, 0, 0, 0, 0, 0}, bb = 0, wt = 1, cnt = 0;
        if (b < b1 && i < cap && rows.get(i, a, bb, wt)) {
            const double sw = sqrt(wt);
            for (int k = 0; k < 6; ++k) a[k] = sw * a[k];
            bb = sw * bb;
            cnt = 1;
        }
        double v[32];
        normeq_terms(a, bb, cnt, v);
        const double sum = wave_sum28(v);
        if (!(lane & 1) && (lane >> 1) < kNormEq) red_ne[wv][lane >> 1] = sum;
        __syncthreads();
        if (t < kNormEq && b < b1) {
            double sacc = 0.0;
            for (int w = 0; w < kBlock / 64; ++w) sacc += red_ne[grp * (kBlock / 64) + w][t];
            slab[b][t] = sacc;
        }
        __syncthreads();
    }
    RSTAMP(10);
    // 3. H, g and the eigendecomposition (k_drpm_eig: a finished frame stops here; 256 threads reduce
    // the slabs, wave 0 solves)
    if (*st.done) return;
    double loc[kNormEq];
#pragma unroll
    for (int k = 0; k < kNormEq; ++k) loc[k] = 0.0;
    if (tid < 256)
        for (int b = tid; b < b1; b += 256)
#pragma unroll
            for (int k = 0; k < kNormEq; ++k) loc[k] += slab[b][k];
    double a32[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) a32[k] = k < kNormEq ? loc[k] : 0.0;
    const double sum = wave_sum28(a32);
    if (wv < 4 && !(lane & 1) && (lane >> 1) < kNormEq) red_ne[wv][lane >> 1] = sum;
    __syncthreads();
    if (tid < kNormEq) {
        double sacc = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) sacc += red_ne[w][tid];
        acc[tid] = sacc;
    }
    __syncthreads();
    if (tid >= 64) return;
    RSTAMP(11);
    const int sweeps = drpm_eig_tail(acc, Dv);   // H, g, the eigendecomposition: k_drpm_eig's
    RSTAMP(12);
#ifdef IMLS_DEBUG_WAVE_TRACE
    if (dbg_on) g_dbg_ransac[13] += (unsigned long long)sweeps;
#else
    (void)sweeps;
#endif
}
#ifdef IMLS_DEBUG_WAVE_TRACE
}  // namespace
}  // namespace imlsgpu
extern "C" int imls_debug_ransac(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(imlsgpu::g_dbg_ransac), 128) == hipSuccess ? 0 : -1;
}
namespace imlsgpu {
namespace {
#endif

// ---------------------------------------------------------------------------------------------
// Batched RANSAC kernels (launch_ransac_batch): frame = tab[blockIdx.y], the same bodies as the
// one-frame kernels above; the frame's RANSAC scratch is A.rf, its pose update always on.
// ---------------------------------------------------------------------------------------------
// The chunk's hypotheses of the frames still running, spread evenly over the grid: each block first
// lists the running frames (done / RANSAC-finished ones drop out), then strides over
// (frame, hypothesis) items — one frame without an early exit gets the whole grid, not a slice.
template <int NT>
__global__ __launch_bounds__(NT) void k_ransac_hyp_b(const PairDev* __restrict__ tab, int npairs, int chunk,
                                                            double dist_thr) {
    __shared__ int sact[kMaxRansacBatch];
    __shared__ int swc[NT / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int na = 0;
    for (int base = 0; base < npairs; base += NT) {
        bool act = false;
        if (base + t < npairs) act = !*tab[base + t].st.done && !*tab[base + t].rf.R.rdone;
        const unsigned long long m = __ballot(act);
        if (lane == 0) swc[wv] = __popcll(m);
        __syncthreads();
        int off = na, tot = na;
        for (int k = 0; k < NT / 64; ++k) {
            off += k < wv ? swc[k] : 0;
            tot += swc[k];
        }
        if (act) sact[off + __popcll(m & ((1ull << lane) - 1ull))] = base + t;
        na = tot;
        __syncthreads();
    }
    const long long items = (long long)na * chunk;
    for (long long q = blockIdx.x; q < items; q += gridDim.x) {
        const int fr = __builtin_amdgcn_readfirstlane(sact[q % na]);
        const int h = (int)(q / na);
        const PairDev A = device_view(tab + fr);
        const size_t c3 = 3 * (size_t)A.rf.cap;
        ransac_hyp_one<NT>(A.rf.all, A.rf.all + c3, A.rf.all + 2 * c3, *A.rf.cnt_all, A.rf.R, dist_thr, h);
    }
}
__global__ __launch_bounds__(64) void k_ransac_select_b(const PairDev* __restrict__ tab, int chunk, int max_iterations,
                                                        double min_pct) {
    const PairDev A = device_view(tab + blockIdx.y);
    if (*A.st.done || *A.rf.R.rdone) return;
    ransac_select_body(A.rf.cnt_all, A.rf.R, chunk, max_iterations, min_pct);
}
__global__ void k_ransac_trace_b(const PairDev* __restrict__ tab, int it) {
    const PairDev A = device_view(tab + blockIdx.y);
    __builtin_assume(A.trace + it != nullptr);
    ransac_trace_t0(A.rf.R, A.rf.cnt_all, A.trace + it);
}

// Hypothesis chunks.  Each hypothesis takes its own rand() word (the h-th ahead of the chunk's state)
// and the select commits exactly the words used, so any chunking gives the same result; chunks only
// trade wasted work after an early exit against launches.  Batched frames: 16 (the usual early exit:
// the shipped 95 % inlier bar is mostly met by the first hypotheses), 256, then up to kHypMax
// (throughput: a frame that exits early wastes little of the shared grid).  A frame alone (lone =
// true, the deployment shape): 272, then up to kHypMax — the first two batched chunks in one launch
// (both fit one wave of blocks, so the merged launch takes about as long as the 16; round 6: a lone
// 1600-row frame without an early exit ran 3 hypothesis + 3 select launches per ICP iteration).
std::vector<int> ransac_chunks(int max_iterations, bool lone = false) {
    std::vector<int> v;
    for (int started = 0; started < max_iterations;) {
        const int want = lone ? (started == 0 ? 272 : kHypMax) : (started == 0 ? 16 : started == 16 ? 256 : kHypMax);
        const int cn = std::min(want, max_iterations - started);
        v.push_back(cn);
        started += cn;
    }
    return v;
}

// The RANSAC scratch of a frame of cap ≥ 1 rows, laid out from p on, every piece on a 256-B boundary;
// p ends behind the last piece, so the one sequence both carves the scratch and sizes it.
RansacFrame ransac_carve(char*& p, int cap, int* rng) {
    const size_t c = (size_t)cap;
    const int nb = solve_blocks(cap);
    RansacFrame F{};
    F.cap = cap;
    F.all = carve<double>(p, 10 * c + 8);
    F.inl = carve<double>(p, 10 * c + 8);
    F.blkcnt = carve<int>(p, nb + 1);
    F.blkw = carve<double>(p, nb + 1);
    F.cnt_all = carve<int>(p, 1);
    F.cnt_in = carve<int>(p, 1);
    F.wsum = carve<double>(p, 1);
    F.R.rng = rng;
    F.R.counts = carve<int>(p, kHypMax);
    F.R.T = carve<double>(p, (size_t)kHypMax * 16);
    F.R.best = carve<int>(p, 1);
    F.R.evaluated = carve<int>(p, 1);
    F.R.rdone = carve<int>(p, 1);
    F.R.bestT = carve<double>(p, 16);
    F.R.active = carve<int>(p, 1);
    F.Dv = drpm_carve(p, nb);
    return F;
}

}  // namespace

size_t ransac_bytes(int cap) {
    char* p = nullptr;                 // a null base: the end of the carve is its size
    ransac_carve(p, std::max(cap, 1), nullptr);
    return (size_t)reinterpret_cast<uintptr_t>(p);
}

RansacFrame ransac_frame(void* scratch, int cap, int* rng) {
    char* p = (char*)scratch;
    return ransac_carve(p, std::max(cap, 1), rng);
}

void launch_ransac(hipStream_t s, const SolveLaunch& L) {
    const KParams& kp = L.kp;
    const RansacParams& rp = L.ransac;
    SolveState st = L.st;
    const int cap = std::max(L.N, 1);
    const size_t c = (size_t)cap;
    const RansacFrame F = ransac_frame(L.scratch, cap, L.rng);
    const RansacDev& R = F.R;
    const int* done = L.st.done;
    // what follows a compaction (kind 1: the count gate and the selection reset; 2: the empty-set check)
    auto post = [&](int kind) { return CompactPost{kind, kp.correspond_number, L.update_pose, L.st, L.tr, R}; };

    // 1. compact the valid correspondences (fp64 rows from the host API are already compact), then
    //    the count gate and the selection reset
    if (!L.rows_are_double) {
        launch_compact(s, Source::valid(L.cs, L.cd, L.cn), L.N, CompactOut::valid(F), post(1), F);
    } else {
        (void)hipMemcpyAsync(F.all, L.rows_d, 9 * c * 8, hipMemcpyDeviceToDevice, s);
        launch_set_count(s, F.cnt_all, L.N);
        k_ransac_begin<<<1, 64, 0, s>>>(F.cnt_all, kp.correspond_number, L.update_pose, L.st, L.tr, R);
    }
    // 2. hypotheses in chunks, 256 threads per hypothesis (a lone frame's chunk has ~1 block per CU, so
    // the per-thread row chains, not the CU's occupancy, set the time: 64-thread blocks took 26.8 µs
    // per 272-hypothesis chunk on a 1600-row frame).  A small DRPM frame's last selection runs at the
    // head of k_drpm_head_small (one launch fewer per ICP iteration).
    // Two chunks whose draws fit the jump table (the shipped 5000 hypotheses: 272 + 4728) run without a
    // selection between them (k_ransac_hyp, base > 0): one selection over both, at the head.
    const std::vector<int> chunks = ransac_chunks(rp.max_iterations, true);
    const bool fold_select = rp.final_method == IMLS_FINAL_DRPM && cap <= kSmallRows;
    const bool one_select = fold_select && chunks.size() == 2 && chunks[0] + chunks[1] <= kHypMax;
    int sel_chunk = chunks.back();
    if (one_select) {
        k_ransac_hyp<256><<<chunks[0], 256, 0, s>>>(F.all, F.cnt_all, cap, R, rp.distance_threshold, chunks[0], done, 0, 0.0);
        k_ransac_hyp<256><<<chunks[1], 256, 0, s>>>(F.all, F.cnt_all, cap, R, rp.distance_threshold, chunks[1], done,
                                                    chunks[0], rp.min_inliers_percentage);
        sel_chunk = chunks[0] + chunks[1];
    } else {
        for (size_t ci = 0; ci < chunks.size(); ++ci) {
            const int cn = chunks[ci];
            k_ransac_hyp<256><<<cn, 256, 0, s>>>(F.all, F.cnt_all, cap, R, rp.distance_threshold, cn, done, 0, 0.0);
            if (!(fold_select && ci + 1 == chunks.size()))
                k_ransac_select<<<1, 64, 0, s>>>(F.cnt_all, R, cn, rp.max_iterations, rp.min_inliers_percentage, done);
        }
    }

    // 3. inliers of the best Δ with their Huber-like weights (order kept), Σw; an empty set stops.  A
    // small DRPM frame: the compaction, pass 1 and the eigendecomposition in one launch (the chain's values)
    const Source isrc = Source::inliers(F, rp.distance_threshold, rp.huber_threshold * rp.distance_threshold);
    double* inl = F.inl;
    const Rows rows{nullptr, nullptr, nullptr, inl, inl + 3 * c, inl + 6 * c, inl + 9 * c, 1, F.cnt_in, F.wsum};
    if (fold_select) {
        const SelectArgs sel{F.cnt_all, sel_chunk, rp.max_iterations, rp.min_inliers_percentage};
        k_drpm_head_small<<<1, kHeadThreads, 0, s>>>(sel, isrc, cap, CompactOut::inliers(F), post(2), rows, solve_blocks(cap),
                                                     L.st, F.Dv);
    } else {
        launch_compact(s, isrc, cap, CompactOut::inliers(F), post(2), F);
    }

    // 4. final solve on the inliers (+ RANSAC's own trace record)
    KParams fk = kp;
    fk.correspond_number = 0;                       // the count gate ran before RANSAC
    switch (rp.final_method) {
        case IMLS_FINAL_LS:
            fk.solve_method = IMLS_SOLVE_LS;
            fk.ls_threshold = rp.ls_threshold;
            launch_solve_chain(s, cap, 0, fk, nullptr, nullptr, nullptr, inl, nullptr, st, L.tr, L.update_pose, 1, F.cnt_in, nullptr);
            if (L.tr) k_ransac_trace<<<1, 64, 0, s>>>(F.cnt_all, R, L.tr);
            break;
        case IMLS_FINAL_WEIGHTED_LS:
            fk.solve_method = IMLS_SOLVE_WEIGHTED_LS;
            launch_solve_chain(s, cap, 0, fk, nullptr, nullptr, nullptr, inl, inl + 9 * c, st, L.tr, L.update_pose, 1, F.cnt_in, F.wsum);
            if (L.tr) k_ransac_trace<<<1, 64, 0, s>>>(F.cnt_all, R, L.tr);
            break;
        default:   // DRPM (the head has run pass 1 and the eigendecomposition of a small frame)
            launch_drpm(s, rows, cap, L.st, F.Dv, L.tr, fk, rp, F.cnt_all, F.cnt_in, L.update_pose, R, L.tr, fold_select);
    }
}

int launch_ransac_batch(hipStream_t s, const PairDev* tab, const int* n_host, int npairs, const KParams& kp,
                        const RansacParams& rp, int it) {
    if (npairs <= 0) return 0;
    if (npairs > kMaxRansacBatch) return -1;   // the hypothesis kernels keep one slot per frame in LDS
    std::vector<int> caps((size_t)npairs);
    int maxc = 1;
    for (int k = 0; k < npairs; ++k) {
        caps[k] = std::max(n_host[k], 1);
        maxc = std::max(maxc, caps[k]);
    }
    const dim3 g1(1, npairs);
    // 1. every frame's valid correspondences, compacted (order kept) to fp64
    launch_compact_batch(s, tab, npairs, maxc, 0, 0.0, 0.0, kp.correspond_number, it);
    // 2. hypotheses: each chunk's items of the still-running frames spread over one grid
    for (const int cn : ransac_chunks(rp.max_iterations)) {
        const int grid = std::min(cn * npairs, kHypGrid);
        if (hyp_block_of(maxc) == 64)
            k_ransac_hyp_b<64><<<grid, 64, 0, s>>>(tab, npairs, cn, rp.distance_threshold);
        else
            k_ransac_hyp_b<256><<<grid, 256, 0, s>>>(tab, npairs, cn, rp.distance_threshold);
        k_ransac_select_b<<<g1, 64, 0, s>>>(tab, cn, rp.max_iterations, rp.min_inliers_percentage);
    }
    // 3. inliers of each frame's best Δ with their weights
    launch_compact_batch(s, tab, npairs, maxc, 1, rp.distance_threshold, rp.huber_threshold * rp.distance_threshold,
                         kp.correspond_number, it);
    // 4. final solve (+ RANSAC's trace record: the DRPM final writes it itself)
    KParams fk = kp;
    fk.correspond_number = 0;
    switch (rp.final_method) {
        case IMLS_FINAL_LS:
            fk.ls_threshold = rp.ls_threshold;
            [[fallthrough]];
        case IMLS_FINAL_WEIGHTED_LS:
            fk.solve_method = rp.final_method == IMLS_FINAL_LS ? IMLS_SOLVE_LS : IMLS_SOLVE_WEIGHTED_LS;
            launch_solve_batch(s, tab, caps.data(), npairs, fk, it, 1);
            k_ransac_trace_b<<<g1, 64, 0, s>>>(tab, it);
            break;
        default:
            launch_drpm_batch(s, tab, caps.data(), npairs, maxc, fk, rp, it);
    }
    return 0;
}

int ransac_init_tables(int device) {
    // C[k][j] over k < kHypMax: C[m − 31] = e_m (m < 31), C[k] = C[k − 31] + C[k − 3] (mod 2^32)
    static std::mutex mu;
    static std::vector<int> ready;
    std::lock_guard<std::mutex> lock(mu);
    if (device < 0) return -1;
    if ((int)ready.size() <= device) ready.resize(device + 1, 0);
    if (ready[device]) return 0;
    std::vector<uint32_t> T((size_t)(kHypMax + 31) * 31, 0u);
    for (int j = 0; j < 31; ++j) T[(size_t)j * 31 + j] = 1u;
    for (int k = 0; k < kHypMax; ++k)
        for (int j = 0; j < 31; ++j)
            T[(size_t)(k + 31) * 31 + j] = T[(size_t)k * 31 + j] + T[(size_t)(k + 28) * 31 + j];
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_rand_jump), T.data() + 31 * 31, (size_t)kHypMax * 31 * 4) != hipSuccess) return -1;
    ready[device] = 1;
    return 0;
}

void ransac_seed_host(uint32_t seed, int st[34]) {
    int32_t r[34];
    r[0] = (int32_t)(seed == 0 ? 1 : seed);
    for (int i = 1; i < 31; ++i) {
        const int64_t hi = r[i - 1] / 127773, lo = r[i - 1] % 127773;
        int64_t word = 16807 * lo - 2836 * hi;
        if (word < 0) word += 2147483647;
        r[i] = (int32_t)word;
    }
    uint32_t ring[31];
    for (int i = 0; i < 31; ++i) ring[i] = (uint32_t)r[i];
    int f = 3, rr = 0;
    for (int k = 0; k < 310; ++k) {   // srandom_r discards 10·31 outputs
        ring[f] += ring[rr];
        f = (f + 1) % 31;
        rr = (rr + 1) % 31;
    }
    for (int i = 0; i < 31; ++i) st[i] = (int)ring[i];
    st[31] = f;
    st[32] = rr;
    st[33] = 0;
}

}  // namespace imlsgpu
