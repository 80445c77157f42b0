// knn_wave.hip — k_knn_wave / k_knn_wave_b: the wave-coherent ("packet") traversal (project.hip's
// header describes the whole matching step).
#include "project_common.h"

namespace imlsgpu {
namespace {

// =============================================================================================
// Packet traversal (hot kernel 1): per-query top-KL list positions + worst key
// =============================================================================================
// The per-wave trace of the diagnostic build (make debug, tools/wave_dump.py): counters and clocks
// behind the hooks knn_wave_body calls; in the product build every hook is empty.
#ifdef IMLS_DEBUG_WAVE_TRACE
__device__ unsigned g_dbg_wave[kDbgWaves][16];
struct WaveTrace {
    long long t0 = 0, t1 = 0;
    unsigned ev = 0, ins = 0;
    unsigned sparse = 0, bcast = 0, sparse_lanes = 0, listed_lv = 0;   // … sparse visits where a wanting lane has a listed point in the leaf
    unsigned mask_lv = 0;   // sparse visits that built the listed mask (some lane had a new candidate)
    unsigned seed_steps = 0, seed_pts = 0;   // seed points where any lane inserted / seed points scanned
    __device__ __forceinline__ void begin() { t0 = wall_clock64(); }
    __device__ __forceinline__ void walk() { t1 = wall_clock64(); }
    __device__ __forceinline__ void leaf(unsigned long long want) {
        if (__popcll(want) <= kSparseLanes) { ++sparse; sparse_lanes += __popcll(want); } else { ++bcast; }
    }
    __device__ __forceinline__ void listed(int nin, unsigned long long want) { listed_lv += (__ballot(nin > 0) & want) ? 1 : 0; }
    __device__ __forceinline__ void mask() { ++mask_lv; }
    __device__ __forceinline__ void insert() { ++ins; }
    __device__ __forceinline__ void event() { ++ev; }
    __device__ __forceinline__ void seed(bool inserts) {
        seed_steps += __ballot(inserts) ? 1 : 0;
        ++seed_pts;
    }
    // the launch counters and the wave's record (16 u32, the layout tools/wave_dump.py reads); w: the
    // wave's index in the launch; w_inf / w_gt1 / wmax: the lane's list is not full / its bound
    // is above 1 / its bound
    __device__ __forceinline__ void end(unsigned long long* nbr_stats, int lane, int w, unsigned n_leaf, unsigned n_inner,
                                        bool greedy, bool w_inf, bool w_gt1, float wmax) {
        if (nbr_stats && lane == 0) {
            atomicAdd(&nbr_stats[6], (unsigned long long)ev);
            atomicAdd(&nbr_stats[7], (unsigned long long)ins);
        }
        if (nbr_stats && lane == 0) {
            const long long t2 = wall_clock64();
            atomicAdd(&nbr_stats[8], (unsigned long long)(t1 - t0));
            atomicMax(&nbr_stats[9], (unsigned long long)(t1 - t0));
            atomicAdd(&nbr_stats[10], (unsigned long long)(t2 - t1));
            atomicMax(&nbr_stats[11], (unsigned long long)(t2 - t1));
            atomicAdd(&nbr_stats[12], (unsigned long long)n_leaf);
            atomicMax(&nbr_stats[13], (unsigned long long)n_leaf);
            atomicMax(&nbr_stats[14], (unsigned long long)ev);
            atomicAdd(&nbr_stats[15], (unsigned long long)__popcll(__ballot(greedy)));
        }
        const unsigned long long gl = __ballot(greedy), wi = __ballot(w_inf), w1 = __ballot(w_gt1);
        for (int o = 1; o < 64; o <<= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, o));
        if (lane == 0 && w < kDbgWaves) {
            unsigned* r = g_dbg_wave[w];
            r[0] = (unsigned)(t1 - t0); r[1] = (unsigned)(wall_clock64() - t1);
            r[2] = n_leaf; r[3] = n_inner; r[4] = ev; r[5] = sparse; r[6] = bcast;
            r[7] = __popcll(gl); r[8] = __popcll(wi); r[9] = __popcll(w1); r[10] = __float_as_uint(wmax);
            r[11] = sparse_lanes; r[12] = listed_lv | (mask_lv << 16); r[13] = ins;
            r[14] = seed_steps; r[15] = __builtin_amdgcn_readfirstlane(seed_pts);
        }
    }
};
#else
struct WaveTrace {
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void walk() {}
    __device__ __forceinline__ void leaf(unsigned long long) {}
    __device__ __forceinline__ void listed(int, unsigned long long) {}
    __device__ __forceinline__ void mask() {}
    __device__ __forceinline__ void insert() {}
    __device__ __forceinline__ void event() {}
    __device__ __forceinline__ void seed(bool) {}
    __device__ __forceinline__ void end(unsigned long long*, int, int, unsigned, unsigned, bool, bool, bool, float) {}
};
#endif

// Slot-id keys in registers, positions in LDS: ~96 VGPRs and ~29 KB of LDS per 4-wave block — 5
// waves/SIMD (round 4: the register list needed 160 VGPRs, 3 waves/SIMD; config B 331 → 406 pairs/s)
#ifndef IMLS_KNN_WAVES
#define IMLS_KNN_WAVES 5
#endif
#define IMLS_KNN_ATTR __attribute__((amdgpu_waves_per_eu(KL <= 26 ? IMLS_KNN_WAVES : 2)))
// One pass: every lane decides reuse, and the packet walks for the lanes that cannot reuse.  (Round 6
// tried a compacted second launch for the later iterations and a breadth-first top for the first
// ones; both measured slower — profiles/r06_compact_rejected/, profiles/r06_bfs_rejected/ — and
// were removed in round 7.)
template <int KL>
__device__ __forceinline__ void knn_wave_body(TreeView t, const float4* __restrict__ spt,
                                                         const unsigned* __restrict__ qperm, int N,
                                                         const double* __restrict__ pose,
                                                         const int* __restrict__ done, KParams kp,
                                                         const double* __restrict__ delta,
                                                         int* __restrict__ lists, float* __restrict__ wlist,
                                                         float4* __restrict__ xref, float* __restrict__ nref,
                                                         int use_prev, unsigned long long* __restrict__ nbr_stats,
                                                         int bx) {
    if (done && ld_const(done)) return;
    __shared__ int snode[kWaveBlock / 64][kWaveStack];
    __shared__ float4 sboxa[kWaveBlock / 64][kWaveStack];   // stacked node boxes: lo.xyz, hi.x
    __shared__ float2 sboxb[kWaveBlock / 64][kWaveStack];   //                     hi.yz
    // the list's positions, slot s of thread tid at spos[s][tid] (slot-id keys, IdKeys)
    __shared__ int spos[KL][kWaveBlock];
    const int tid = threadIdx.x, lane = tid & 63;
    int* const mypos = &spos[0][tid];
    using IK = IdKeys<KL>;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // a wave owns kp.packet Morton-consecutive queries (64; 32 or 16 in the first iterations, where
    // most lanes seed: a smaller packet's union of neighbourhoods is smaller, and the launch lasts
    // as long as its slowest wave); lanes past the packet idle
    const int qp = kp.packet;
    const int slot = (bx * (kWaveBlock / 64) + wv) * qp + lane;
    const bool active = lane < qp && slot < N;
    float xf[3] = {0.f, 0.f, 0.f};
    // the stored list's bound and reference (slot-indexed) load beside the query's point: one round
    // trip after the query index, not one more after the transform
    float w_prev = 0.f, n_prev = 0.f;
    float4 x_prev = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) {
        double ns[3];
        const int i = (int)qperm[slot];
        const float4 sp4 = spt[i];
        if (use_prev) {
            w_prev = wlist[slot];
            x_prev = xref[slot];
            n_prev = nref[slot];
        }
        transform_query(pose, sp4, make_float4(0.f, 0.f, 0.f, 0.f), 0, xf, ns);
    }
    float lk[KL];
#pragma unroll
    for (int j = 0; j < KL; ++j) lk[j] = IK::empty(j);
    // the slots are cleared here when no seed table is staged; in the first ICP iteration the table
    // aliases spos and they are cleared after the seed search, below
    if (use_prev) {
#pragma unroll
        for (int j = 0; j < KL; ++j) mypos[j * kWaveBlock] = -1;
    }
    // the list behind one interface: thr_ = the strict insertion threshold (a point with key d joins
    // iff d < thr_()), ins_ = sorted insertion (precondition d < thr_()), pos_ = position of slot s
    // (any order), full_ = KL real entries, need_ = need_key (upper-rounded for slot-id keys)
    auto thr_ = [&]() -> float { return IK::lo(lk[KL - 1]); };
    auto full_ = [&]() -> bool { return IK::real(lk[KL - 1]); };
    auto pos_ = [&](int s) -> int { return mypos[s * kWaveBlock]; };
    auto need_ = [&]() -> float { return need_key_ids<KL>(lk, (float)kp.r2, kp.K); };
    auto ins_ = [&](float d, int pos) {
        const unsigned s = IK::id(lk[KL - 1]);
        insert_key<KL>(lk, IK::make(d, s));
        mypos[s * kWaveBlock] = pos;
    };
    const float r2s = (float)(kp.r2 * kSearchR2) * kBoxSlack + 1e-30f;   // the search bound (radius (1 + skin)·r)
    float bnd = active ? r2s : -1.0f;
    // (pinned: scalars of their own — as members of the view's 8-dword kernel-argument tuple, every
    // use inside the walk loop reloaded the whole spilled tuple, 8 v_readlane each)
    int P = t.P, B = t.B, M = t.M;
    asm volatile("" : "+s"(P), "+s"(B), "+s"(M));
    WaveTrace trace;
    trace.begin();
    bool greedy = active && !use_prev;
    bool skip = false;               // list certified without a traversal (Verlet-list reuse)
    float wskip = kInfF;
    if (active && use_prev) {
        // temporal seed only while the query moved little against its neighbourhood: the last
        // pose increment Δ moves it by at most ‖t‖ + ‖R − I‖_F·‖x‖
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
        greedy = disp * disp > kReseed * w_prev;
    }
    float wlow = -1.0f;              // W' of the stored list at xf (prefill certificate below)
    if (active && !greedy && kp.reuse) skip = verlet_skip(x_prev, n_prev, xf, r2s, wskip, wlow);
    if (active && !greedy && !skip) {
        // prefill from the previous iteration's list re-measured at the new pose: all positions,
        // then all points are loaded before any is consumed (two memory round trips, not 2·KL),
        // and the nearly sorted keys are ordered by an early-exit odd-even transposition sort
        // (the list is full and the bound tight before the traversal starts; a later leaf insert
        // must then skip points already listed).  Slot j keeps entry j's position; its key carries
        // id j (the keys alone get sorted)
        // The points in two chunks, each chunk's loads issued (pinned) before any of its slot writes:
        // in the batched kernel the table's pointers are generic, so a point load after a slot write
        // (an LDS store it might alias) waited for it — one round trip per entry
        int pj[KL];
#pragma unroll
        for (int j = 0; j < KL; ++j) pj[j] = lists[(size_t)j * N + slot];
        constexpr int kPCh = (KL + 1) / 2;
#pragma unroll
        for (int j0 = 0; j0 < KL; j0 += kPCh) {
            float4 q[kPCh];
#pragma unroll
            for (int u = 0; u < kPCh; ++u)
                if (j0 + u < KL) q[u] = t.mpt[max(pj[j0 + u], 0)];
#pragma unroll
            for (int u = 0; u < kPCh; ++u)
                if (j0 + u < KL) pin_loaded(q[u]);
#pragma unroll
            for (int u = 0; u < kPCh; ++u) {
                const int j = j0 + u;
                if (j >= KL) break;
                const float ex = q[u].x - xf[0], ey = q[u].y - xf[1], ez = q[u].z - xf[2];
                const float d32 = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
                const bool keep = pj[j] >= 0 && d32 <= r2s;
                lk[j] = keep ? IK::make(d32, j) : IK::empty(j);
                mypos[j * kWaveBlock] = keep ? pj[j] : -1;
            }
        }
        bool swapped = true;
        while (swapped) {
            swapped = false;
#pragma unroll
            for (int par = 0; par < 2; ++par) {
#pragma unroll
                for (int j = par; j + 1 < KL; j += 2) {
                    const bool sw = lk[j + 1] < lk[j];
                    const float tk = lk[j];
                    lk[j] = sw ? lk[j + 1] : lk[j];
                    lk[j + 1] = sw ? tk : lk[j + 1];
                    swapped |= sw;
                }
            }
        }
        bnd = fmin_nn(r2s, thr_());
        // prefill certificate: the stored list re-measured at xf holds its answer when the key that
        // answer relies on (max(K-th key within r, NN-1 key), need_key) is below W' — every point
        // outside the list is at least √W' away (verlet_skip) — so the traversal is skipped exactly
        // as for a Verlet reuse; the stale bound √nr + D there is the worst case of this re-measured
        // key.  (fp32 slack as in verlet_skip; k_finish re-certifies the list in fp64 against W'.)
        if (kp.reuse && wlow > 0.f) {
            const float nk = need_();
            if (nk < kInfF && nk * (1.0f + 1e-5f) < wlow) { skip = true; wskip = wlow; }
        }
    }
    // leaf scan of the traversal (its one call site): the lanes in `want` test every point of
    // leaf `leaf` against their bound; `listed`: the leaf may hold points already in a lane's
    // list (prefilled or seeded), which must not be inserted twice
    // mine: lane k's point k of the leaf (loaded by the caller; zero past the leaf's count)
    auto scan_leaf = [&](int leaf, unsigned long long want, bool listed, float4 mine) {
        const int base = leaf * B;
        const int cnt = min(B, M - base);
        // points of this leaf already in the lane's list, as a bit mask: one lockstep pass over
        // the list instead of a divergent membership test per point
        unsigned long long inl = 0ull;
        auto listed_mask = [&]() {
#pragma unroll
            for (int k = 0; k < KL; ++k) {
                const unsigned rel = (unsigned)(pos_(k) - base);
                inl |= rel < 64u ? (1ull << rel) : 0ull;
            }
        };
        const bool sparse = __popcll(want) <= kSparseLanes;
        // the two scans are two ifs, the second's flag opaque (an empty pin), not an if/else: the
        // structuriser's if/else gives the keys written in its first arm a register set of their own
        // (see the walk loop's header)
        int bcast = __builtin_amdgcn_readfirstlane(!sparse);
        asm volatile("" : "+s"(bcast));
        trace.leaf(want);
        if (sparse) {
            // few lanes want this leaf (spread-out queries in a dense region): per wanting lane,
            // all leaf points are measured at once (one per lane) and the ones under that lane's
            // bound and not yet listed become its candidate mask; then the lanes insert their own
            // candidates in lockstep, each its lowest pending point per step (index order) fetched
            // by ds_bpermute — max(per-lane candidates) insertion steps instead of one per
            // candidate of every lane.  Per lane, the insertions are exactly the sequential scan's
            // (same order, re-tested at the current bound; a non-candidate was above the
            // leaf-start bound already).
            // Listed points: only their NUMBER in the leaf per lane up front (3 ops per list slot
            // instead of 7).  Every listed point of the leaf is a candidate of its lane (its key,
            // recomputed here bit for bit, is ≤ the lane's candidate bound cb), so a lane with
            // exactly that many candidates has no new one; the mask itself is built only when some
            // lane has more (a leaf with new points).  cb must admit every listed point: slot-id
            // keys truncate, so a listed point can lie up to hi(max key) (the insertion loop
            // re-tests d32 < thr_())
            int nin = 0;
            if (listed) {
#pragma unroll
                for (int k = 0; k < KL; ++k) nin += (unsigned)(pos_(k) - base) < (unsigned)cnt ? 1 : 0;
                trace.listed(nin, want);
            }
            const float cb = fmin_nn(r2s, IK::hi(lk[KL - 1]));
            // lane q's candidate mask is written into lane q by v_writelane (two per trip: the mask is
            // wave-uniform, in SGPRs) instead of a compare and two selects over all lanes; the
            // in-leaf mask is one scalar AND on the compare's own mask (no trip through a VGPR)
            int cm_lo = 0, cm_hi = 0;
            // (cnt ≥ 1 for every leaf the walk admits — a padded leaf past M has an inverted box — as the
            // broadcast scan's lp[cnt − 1] assumes too; clamped all the same: no undefined shift)
            const unsigned long long inleaf = cnt >= 64 ? ~0ull : (1ull << max(cnt, 0)) - 1ull;
            // The trip knows nothing of listed points (round 8: no branch in it, and the visited bit
            // goes by a shift and one and-not): lane q gets its raw candidate mask, and the listed
            // points are taken out after the loop in vector form, below
            unsigned long long m = want;
            while (m) {
                const int q = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
                m &= ~(1ull << q);
                const float qx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xf[0]), q));
                const float qy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xf[1]), q));
                const float qz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xf[2]), q));
                const float qb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cb), q));
                const float ex = mine.x - qx, ey = mine.y - qy, ez = mine.z - qz;
                const float d32 = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
                const unsigned long long pm = __ballot(d32 <= qb) & inleaf;
                cm_lo = imls_amdgcn_writelane((int)(unsigned)pm, q, cm_lo);
                cm_hi = imls_amdgcn_writelane((int)(unsigned)(pm >> 32), q, cm_hi);
            }
            unsigned long long cm = ((unsigned long long)(unsigned)cm_hi << 32) | (unsigned)cm_lo;
            // Each lane now owns its mask and its listed count.  A lane with exactly nin candidates
            // holds only listed points (above), so cm & ~inl is zero there as well: when no lane has
            // more, every mask is cleared without building inl; else inl is built once, in lockstep,
            // and taken out of every lane's mask.  (Lanes outside `want` have cm = 0 ≤ nin.)
            if (listed) {
                if (__ballot(__popcll(cm) > nin)) {
                    trace.mask();
                    listed_mask();
                    cm &= ~inl;
                } else {
                    cm = 0ull;
                }
            }
            while (__ballot(cm != 0ull)) {
                // every lane takes part in the permutes and measures its point (lanes without a
                // candidate read lane 0's and drop it): one predicate, one divergent region
                const bool has = cm != 0ull;
                const int jj = has ? (int)__builtin_ctzll(cm) : 0;
                const float px = __shfl(mine.x, jj), py = __shfl(mine.y, jj), pz = __shfl(mine.z, jj);
                cm &= cm - 1ull;   // (0 stays 0)
                const float ex = px - xf[0], ey = py - xf[1], ez = pz - xf[2];
                const float d32 = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
                if (has & (d32 <= bnd) & (d32 < thr_())) {
                    trace.insert();
                    ins_(d32, base + jj);
                    bnd = fmin_nn(r2s, thr_());
                }
                trace.event();
            }
        }
        if (bcast) {
            if (listed) listed_mask();
            const bool wants = (want >> lane) & 1ull;
            // broadcast, round 6: the leaf's points come by scalar loads (wave-uniform addresses, a
            // group of kBcGroup points per s_load burst, the next group in flight while this one is
            // measured) and feed the distance VALUs as SGPR operands — no v_readlane per coordinate;
            // a group none of whose points is under any wanting lane's bound (the common case once
            // the bounds are tight) costs one compare and one branch instead of one per point.  The
            // insertion order and the keys are the per-point scan's, bit for bit.
            const kconst_f4* lp = (const kconst_f4*)t.mpt + base;
            kf4v g[kBcGroup];
#pragma unroll
            for (int u = 0; u < kBcGroup; ++u) g[u] = lp[min(u, cnt - 1)];
            for (int j0 = 0; j0 < cnt; j0 += kBcGroup) {
                kf4v nx[kBcGroup];
                const int jn = j0 + kBcGroup;
                if (jn + kBcGroup <= cnt) {   // a whole group: one base address, immediate offsets
                    const kconst_f4* q = lp + jn;
#pragma unroll
                    for (int u = 0; u < kBcGroup; ++u) nx[u] = q[u];
                } else {
#pragma unroll
                    for (int u = 0; u < kBcGroup; ++u) nx[u] = lp[min(jn + u, cnt - 1)];
                }
                float d[kBcGroup];
                float dmin = kInfF;
#pragma unroll
                for (int u = 0; u < kBcGroup; ++u) {
                    const float ex = g[u].x - xf[0], ey = g[u].y - xf[1], ez = g[u].z - xf[2];
                    d[u] = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
                    dmin = fminf(dmin, d[u]);   // past cnt: a copy of the last point (never inserted)
                }
                if (__ballot(wants && dmin <= bnd)) {
#pragma unroll
                    for (int u = 0; u < kBcGroup; ++u) {
                        const int j = j0 + u;
                        const bool ins = j < cnt && wants && d[u] <= bnd && d[u] < thr_() && !((inl >> j) & 1ull);
                        if (ins) {
                            ins_(d[u], base + j);
                            bnd = fmin_nn(r2s, thr_());
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < kBcGroup; ++u) g[u] = nx[u];
            }
        }
    };
    // seed (first ICP iteration, or a lane that moved far): the leaf holding the lane's own Morton
    // key (binary search over the leaves' first keys) ± kSeedHalf, scanned per lane — Morton-near
    // points are mostly space-near, while a greedy box-distance descent goes astray in the heavily
    // overlapping upper-level boxes.  The traversal re-scans these leaves harmlessly (listed points
    // are masked, the rest are not under the bound).
    const unsigned long long gmask = __ballot(greedy);
    // the seed search's leaf: its first ~10 bisection steps run in a coarse table of every S-th
    // leaf key staged in LDS (one coalesced block load), the last ⌈log2 S⌉ in HBM/L2 — instead of
    // ~15 dependent global loads per lane (first ICP iteration only, where every lane seeds: later
    // iterations reseed a few lanes, which would not repay the block barrier).  The table lives in
    // spos, whose slots are not in use yet (cleared after the search)
    static_assert(KL * kWaveBlock * 4 >= kSeedTab * 8, "seed table fits the slot array");
    unsigned long long* const skey = reinterpret_cast<unsigned long long*>(&spos[0][0]);
    const int S = use_prev ? t.L : (t.L + kSeedTab - 1) / kSeedTab;
    const int ntab = S > 0 ? (t.L + S - 1) / S : 0;
    if (!use_prev) {
        for (int k = threadIdx.x; k < ntab; k += kWaveBlock) skey[k] = t.lkeys[(size_t)k * S];
        __syncthreads();
    }
    int seed_leaf = 0;
    if (greedy) {
        const unsigned long long qk = morton48(xf[0], xf[1], xf[2], t.qparams);
        int j = 0, jh = ntab - 1;
        while (j < jh) {
            const int mid = (j + jh + 1) >> 1;
            if (skey[mid] <= qk) j = mid;
            else jh = mid - 1;
        }
        int l = j * S, h = min(t.L, (j + 1) * S) - 1;   // the largest leaf l with lkeys[l] ≤ qk (else 0)
        while (l < h) {
            const int mid = (l + h + 1) >> 1;
            if (t.lkeys[mid] <= qk) l = mid;
            else h = mid - 1;
        }
        seed_leaf = l;
    }
    if (!use_prev) {
        __syncthreads();             // every wave is done with the seed table (it aliases spos)
#pragma unroll
        for (int j = 0; j < KL; ++j) mypos[j * kWaveBlock] = -1;
    }
    if (greedy) {
        const int l = seed_leaf;
        const int p0s = max(0, l - kSeedHalf) * B;
        const int pend = min(M, (min(t.L - 1, l + kSeedHalf) + 1) * B);
        float4 qs[kSeedChunk];
#pragma unroll
        for (int k = 0; k < kSeedChunk; ++k) qs[k] = t.mpt[min(p0s + k, pend - 1)];
        for (int p0 = p0s; p0 < pend; p0 += kSeedChunk) {
            float4 nx[kSeedChunk];   // software pipelined: the next chunk is in flight while this one is consumed
#pragma unroll
            for (int k = 0; k < kSeedChunk; ++k) nx[k] = t.mpt[min(p0 + kSeedChunk + k, pend - 1)];
#pragma unroll
            for (int k = 0; k < kSeedChunk; ++k) {
                const float ex = qs[k].x - xf[0], ey = qs[k].y - xf[1], ez = qs[k].z - xf[2];
                const float d32 = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
                trace.seed(p0 + k < pend && d32 <= bnd && d32 < thr_());
                if (p0 + k < pend && d32 <= bnd && d32 < thr_()) {
                    ins_(d32, p0 + k);
                    bnd = fmin_nn(r2s, thr_());
                }
            }
#pragma unroll
            for (int k = 0; k < kSeedChunk; ++k) qs[k] = nx[k];
        }
    }
    unsigned n_inner = 0, n_leaf = 0;
    trace.walk();
    if (skip) bnd = -1.0f;           // a certified lane takes no part in the traversal
    int node = 1, sp = 0;
    int pf_leaf = -1;                 // the leaf whose points `pf` holds (wave-uniform)
    float4 pf = make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned long long em = __ballot(active && !skip);   // lanes whose bound admits the current node's box
    const unsigned long long skipped = __ballot(skip);
    if (nbr_stats && lane == 0 && skipped) atomicAdd(&nbr_stats[kStatSkipped], (unsigned long long)__popcll(skipped));
    // The loop body is three plain ifs in a row — if (node < P) the node step, if (at_leaf) the leaf
    // scan, if (pop) the pop — with no else, no continue, no break, and one exit at the header, so
    // that the keys and bnd are one loop-carried value each.  The loop holds divergent branches (the
    // insertions), so the backend's control-flow structuriser rewrites all of it, and it turns
    // `if (c) A else B` into `if (c) A; Flow; if (!c) B`: every value A writes gets a register of
    // its own, undefined on the path around A.  The leaf scan's keys then could not share registers
    // with the loop's, and all KL + 1 were copied at the leaf's entry and again at the back edge
    // (profiles/r07_knn_issue/).  Around a plain if the bypass carries the loop's own value.
    // at_leaf and pop (and bcast in scan_leaf) pass through empty asm pins: the optimiser would
    // otherwise see that they are complementary / constant on each path and thread the three ifs
    // back into the if/else + continue + break shape.
    while (em) {
        int pop = 1;
        int at_leaf = __builtin_amdgcn_readfirstlane(node >= P);
        asm volatile("" : "+s"(at_leaf));
        if (node < P) {
            // one step descends `sw` binary levels at once: the 2^sw descendants' boxes sit in
            // the 2^(sw−1) consecutive records of the intermediate level (one scalar burst of
            // ≤ 192 B), so a root-to-leaf walk costs ⌈levels/3⌉ dependent loads instead of levels
            ++n_inner;
            const int lev = 31 - __builtin_clz(node);
            const int sw = min(kWide, t.levels - lev);
            const int nk = 1 << sw, nrec = nk >> 1;
            // the records are read-only for the whole kernel and the address is wave-uniform: read
            // them through the constant address space so they come by scalar loads into SGPRs (a
            // generic pointer is may-clobbered by the fences / atomics of this kernel and would be
            // fetched by vector loads into 48 VGPRs)
            const int unode = __builtin_amdgcn_readfirstlane(node);
            const kconst_f4* rec = (const kconst_f4*)t.nodes + 3 * ((size_t)unode << (sw - 1));
            // lane k < 2^sw also fetches child k's own box (6 consecutive floats of the records) by a
            // vector load: the push below then is ONE masked section — lane k writes child k's stack
            // entry — instead of eight unrolled lane-0 pushes fed from the scalar records, and the 48
            // record SGPRs die after the box tests (they were live to the last push, the cause of
            // most scalar spills).  Issued before the scalar burst, consumed after the vote
            float2 cb0 = make_float2(0.f, 0.f), cb1 = cb0, cb2 = cb0;
            if (lane < nk) {
                const float2* cp = reinterpret_cast<const float2*>(t.nodes + 3 * ((size_t)unode << (sw - 1))) + 3 * lane;
                cb0 = cp[0]; cb1 = cp[1]; cb2 = cp[2];
            }
            // (a record past the step's last is the last one again, its child masked below; the clamp
            // is on the 32-bit byte offset — one s_min and a register-offset s_load per record, not
            // a 64-bit address each)
            float4 R[3 * (kWideMax / 2)];
            const unsigned lastb = (unsigned)(3 * nrec - 1) * 16u;
#pragma unroll
            for (int k = 0; k < 3 * (kWideMax / 2); ++k) {
                const kf4v v = *(const kconst_f4*)((const __attribute__((address_space(4))) char*)rec + min((unsigned)k * 16u, lastb));
                R[k] = make_float4(v.x, v.y, v.z, v.w);
            }
            const float bs = bnd * kBoxSlack;
            // round 8: the lanes keep what they want as one bit per child (no ballot per child), and
            // the wave's view of it — the wanted children wm, the votes per child — comes from three
            // DPP reductions on the vector side instead of 8 ballots, 8 popcounts and their selects
            unsigned wbits = 0u;
            int best = -1;
            float bd = kInfF;
#pragma unroll
            for (int k = 0; k < kWideMax; ++k) {
                const float4 a = R[3 * (k >> 1)], b = R[3 * (k >> 1) + 1], c = R[3 * (k >> 1) + 2];
                const float d = (k & 1) ? box_d2(xf, b.z, b.w, c.x, c.y, c.z, c.w) : box_d2(xf, a.x, a.y, a.z, a.w, b.x, b.y);
                const bool w = k < nk && d <= bs;
                wbits |= w ? (1u << k) : 0u;
                if (w && d < bd) { bd = d; best = k; }
            }
            // descend into the child most lanes find nearest; stack the other wanted ones so that
            // they pop in Morton (index) order.  A lane's vote is a one in byte `best` of a 64-bit
            // word (two halves; a count is ≤ 64, so the bytes never carry); child k's key is
            // (votes << 3) | (7 − k) in lane k, and the largest key among the wanted children names
            // the first child with the most votes — the strict `>` of a scan k = 0 … 7 that starts
            // at the first wanted child
            const unsigned hot = best < 0 ? 0u : 1u << ((best & 3) * 8);
            const unsigned wm = (unsigned)wave_last(wave_reduce<RedOr>((int)wbits));
            const unsigned vlo = (unsigned)wave_last(wave_reduce<RedAdd>((int)(best < 4 ? hot : 0u)));
            const unsigned vhi = (unsigned)wave_last(wave_reduce<RedAdd>((int)(best < 4 ? 0u : hot)));
            const unsigned cnt = (unsigned)((((unsigned long long)vhi << 32) | vlo) >> ((lane & 7) * 8)) & 0xffu;
            // (+ 1: zero, the reductions' identity, stands for "not wanted")
            unsigned key = (wm >> (lane & 7)) & 1u ? ((cnt << 3) | (unsigned)(7 - (lane & 7))) + 1u : 0u;
            key = max(key, (unsigned)dpp_i<kDppShr1>(0, (int)key));
            key = max(key, (unsigned)dpp_i<kDppShr2>(0, (int)key));
            key = max(key, (unsigned)dpp_i<kDppShr4>(0, (int)key));
            const unsigned kmax = (unsigned)__builtin_amdgcn_readlane((int)key, 7);   // lanes 0 … 7 hold children 0 … 7
            const int cstar = kmax == 0u ? -1 : 7 - (int)((kmax - 1u) & 7u);
            // the wanted children but cstar, pushed as the unrolled loop k = 7 … 0 did (child k above
            // every wanted child > k, so they pop in Morton order): child k's slot is sp + the number
            // of pushed children above k.  The divergent section stands alone, before the uniform
            // updates: merged into their if, its join made sp, em, node and pop look divergent
            const unsigned pm = cstar >= 0 ? wm & ~(1u << cstar) : 0u;
            if (lane < kWideMax && ((pm >> lane) & 1u)) {
                const int pos = sp + __popc(pm >> (lane + 1));
                snode[wv][pos] = (node << sw) + lane;
                sboxa[wv][pos] = make_float4(cb0.x, cb0.y, cb1.x, cb1.y);
                sboxb[wv][pos] = cb2;
            }
            if (cstar >= 0) {
                sp += __popc(pm);
                em = __ballot((wbits >> cstar) & 1u);
                node = (node << sw) + cstar;
                pop = 0;
            }
        }
        if (at_leaf) {
            ++n_leaf;
            const int leaf = node - P;
            float4 mine = make_float4(0.f, 0.f, 0.f, 0.f);
            // the leaf's points were prefetched when it was the stack's top during the previous leaf
            // scan; else loaded now.  Then the stack's top, when it is a leaf (most often the next node
            // visited: a sibling at the bottom level), has its points in flight during this scan
            if (leaf == pf_leaf) mine = pf;
            else if (lane < min(B, M - leaf * B)) mine = t.mpt[leaf * B + lane];
            pf_leaf = -1;
            if (sp > 0) {
                const int nn = __builtin_amdgcn_readfirstlane(snode[wv][sp - 1]);
                if (nn >= P) {
                    pf_leaf = nn - P;
                    pf = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (lane < min(B, M - pf_leaf * B)) pf = t.mpt[pf_leaf * B + lane];
                }
            }
            scan_leaf(leaf, em, use_prev || gmask, mine);
        }
        // pop: the stacked node's box is in LDS — re-check it against the shrunken lane bounds.  The
        // flag is opaque to the optimiser (an empty pin), which would otherwise thread the leaf path
        // straight into the pop and the descent straight to the back edge: see the loop's header
        asm volatile("" : "+s"(pop));
        if (pop) {
            em = 0ull;
            while (sp > 0 && !em) {
                --sp;
                const float4 b0 = sboxa[wv][sp];
                const float2 b1 = sboxb[wv][sp];
                const float d = box_d2(xf, b0.x, b0.y, b0.z, b0.w, b1.x, b1.y);
                em = __ballot(d <= bnd * kBoxSlack);
            }
            if (em) node = snode[wv][sp];
        }
    }
    if (active && skip) wlist[slot] = wskip;   // a reused list stays in place
    if (active && !skip) {
#pragma unroll
        for (int j = 0; j < KL; ++j) lists[(size_t)j * N + slot] = pos_(IK::id(lk[j]));   // ascending keys
        const bool full = full_();
        const float wk = full ? thr_() : kInfF;
        wlist[slot] = wk;
        // reference position + guarantee of a fresh list: every map point outside it has fp32
        // key ≥ the KL-th key's truncation thr_ (full list) or > the search bound (all points
        // within r listed)
        xref[slot] = make_float4(xf[0], xf[1], xf[2], full ? wk : r2s);
        nref[slot] = need_();
    }
    trace.end(nbr_stats, lane, bx * (kWaveBlock / 64) + wv, n_leaf, n_inner, greedy, active && !full_(),
              active && full_() && thr_() > 1.0f, active && full_() ? thr_() : 0.f);
    if (nbr_stats && lane == 0) {
        atomicAdd(&nbr_stats[2], (unsigned long long)n_leaf);
        atomicAdd(&nbr_stats[3], (unsigned long long)n_inner);
        atomicAdd(&nbr_stats[4], 1ull);
    }
}

template <int KL>
__global__ __launch_bounds__(kWaveBlock) IMLS_KNN_ATTR void k_knn_wave(
        TreeView t, const float4* __restrict__ spt, const unsigned* __restrict__ qperm, int N,
        const double* __restrict__ pose, const int* __restrict__ done, KParams kp, const double* __restrict__ delta,
        int* __restrict__ lists, float* __restrict__ wlist, float4* __restrict__ xref, float* __restrict__ nref,
        int use_prev, unsigned long long* __restrict__ nbr_stats) {
    knn_wave_body<KL>(t, spt, qperm, N, pose, done, kp, delta, lists, wlist, xref, nref, use_prev, nbr_stats,
                      (int)blockIdx.x);
}

template <int KL>
__global__ __launch_bounds__(kWaveBlock) IMLS_KNN_ATTR void k_knn_wave_b(const PairDev* __restrict__ tab, KParams kp,
                                                                          int use_prev, int npairs) {
    int f, bx;
    batch_block(kp.xcd, f, bx);
    if (f >= npairs) return;
    const PairDev A = device_view(tab + f);
    if (use_qwave(kp, A.N) || bx >= knn_blocks_of(A.N, kp.packet)) return;
    const ListBlock lb = list_block(A.lists, A.N, KL);
    knn_wave_body<KL>(A.t, A.spt, A.qperm, A.N, A.st.pose, A.st.done, kp, A.st.delta, lb.pos, lb.wlist, lb.xref, lb.nref,
                      use_prev, A.stats, bx);
}

}  // namespace

void launch_knn_wave(hipStream_t s, const ProjectLaunch& L) {
    with_list_sizes(L.kp.K, [&](auto z) {
        constexpr int KL = decltype(z)::KL;
        const ListBlock lb = list_block(L.lists, L.N, KL);
        k_knn_wave<KL><<<knn_blocks_of(L.N, L.kp.packet), kWaveBlock, 0, s>>>(L.t, L.spt, L.qperm, L.N, L.pose, L.done, L.kp,
                                                                              L.delta, lb.pos, lb.wlist, lb.xref, lb.nref,
                                                                              L.use_prev, L.stats);
    });
}

void launch_knn_wave_batch(hipStream_t s, dim3 grid, const PairDev* tab, const KParams& kp, int use_prev, int npairs) {
    with_list_sizes(kp.K, [&](auto z) {
        k_knn_wave_b<decltype(z)::KL><<<grid, kWaveBlock, 0, s>>>(tab, kp, use_prev, npairs);
    });
}

}  // namespace imlsgpu

#ifdef IMLS_DEBUG_WAVE_TRACE
// debug build only: per-wave records of the last k_knn_wave launch (16 u32 per wave)
extern "C" int imls_debug_waves(unsigned* out, int nwaves) {
    const int n = nwaves < imlsgpu::kDbgWaves ? nwaves : imlsgpu::kDbgWaves;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(imlsgpu::g_dbg_wave), (size_t)n * 64) == hipSuccess ? n : -1;
}
#endif
