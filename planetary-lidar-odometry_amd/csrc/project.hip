// project.hip — fused transform + matching: the GPU form of one ICP iteration's Matching
// step (laser_odometry.cpp:527-549 → IMLSICPMatcher::ProjSourcePtToSurface, imls_icp.cpp:496-745
// → ImplicitMLSFunction, imls_icp.cpp:301-483).  This unit is the host side (which kernels a frame
// or a batch takes, in what order); the kernels: knn_wave.hip (k_knn_wave), knn_qwave.hip (the
// wave-per-query traversal, alone or fused with its exact stage), finish.hip (k_finish,
// k_project_lane), knn_export.hip (the public kNN query); shared code: project_common.h, exact_stage.h.
//
// k_knn_wave (hot kernel 1) — wave-coherent ("packet") traversal of the target tree:
//   * a wave owns 64 queries taken in Morton order of the source scan, so they are neighbours;
//   * ONE traversal per wave: the node index and the LDS stack (node + its box, so a pop needs no
//     memory round trip) are wave-uniform, node records come through the scalar cache; a child is
//     entered when any lane's box distance is within that lane's bound (ballot), near-first by
//     lane majority;
//   * a leaf (B ≤ 64 Morton-consecutive map points) is ONE coalesced float4 load, each point is
//     broadcast to all lanes by v_readlane and tested against each lane's register top-(K+4)
//     list keyed by the fp32 distance;
//   * bounds: iteration 0 seeds each lane from its nearest leaf (greedy descent); later ICP
//     iterations prefill the list with the previous iteration's neighbours re-measured at the
//     new pose (temporal coherence: the pose changes little), so few leaf points insert;
//   * output: the list positions (Morton order) and the worst key W per query, to HBM.
// k_finish (hot kernel 2) — one lane per query: the exact stage — fp64 distances
//   ((dx²+dy²)+dz², the libnabo metric, no FMA) of the list, sorted by (d², index), the radius
//   filter (d² ≤ r², inclusive), NN-1 = first entry with d² > DBL_EPSILON (no self match,
//   imls_icp.cpp:605-607), L = first K (ALLOW_SELF_MATCH, imls_icp.cpp:372-375);
//   CERTIFICATION — every map point outside the list has d²₆₄ ≥ W/(1+3.1e-7)
//   (|d²₃₂ − d²₆₄| ≤ 5·2⁻²⁴·d²), so the result is exact iff the largest exact distance it relies
//   on is < W/(1+4e-7); uncertified queries (near-ties at the list edge, > K+4 duplicates) are
//   appended to a list that k_project_lane re-runs exactly.  Then the gates
//   (imls_icp.cpp:612-717 in order), IMLS height with the h_max quirk (Q3) and the 1e-5 bias (Q4),
//   y = float(x − height·n_NN), and the pass-1 normal-equation partials of the LS solve
//   (solver.cpp:89-107): 21 JᵀJ + 6 Jᵀb + count per block, fp64.
// k_project_lane — one lane per query, exact fp64 list during the traversal (the fallback, and
// the IMLS_TRAVERSAL_LANE reference mode, imls_set_option).
// Compiled with -ffp-contract=off: every fp64 expression evaluates as written.
#include "project_common.h"

namespace imlsgpu {

void launch_project_batch(hipStream_t s, const PairDev* tab, const int* n_host, int npairs, const KParams& kp0, int it,
                          int use_prev) {
    // auto traversal choice for a batch: the wave-per-query kernel wins on one small frame (latency:
    // few waves), packets win once the batch's queries fill the GPU (measured on the config-C-like
    // stream, 32 frames of ~1900 queries per launch: 546 → 320 µs).  Either gives the exact answer.
    KParams kp = kp_at(kp0, kp0.pk_batch ? it : -1);
    long long total = 0;
    for (int k = 0; k < npairs; ++k) total += n_host[k];
    if (kp.qwave < 0 && total > kQwaveAutoN) kp.qwave = 0;
    // XCD-grouped frames for batches of many frames (their maps together outgrow the L2s)
    if (kp.xcd < 0) kp.xcd = npairs >= 16 ? 1 : 0;
    // tensor voting: every frame's voted normals at its current pose first (imls_icp.cpp:514-546)
    if (kp.tv) launch_tv_vote_batch(s, tab, n_host, npairs, kp, use_prev);
    int maxN = 0;
    bool any_small = false, any_large = false;
    for (int k = 0; k < npairs; ++k) {
        maxN = std::max(maxN, n_host[k]);
        (use_qwave(kp, n_host[k]) ? any_small : any_large) = true;
    }
    if (npairs <= 0 || maxN <= 0) return;
    const int gy = kp.xcd ? (npairs + 7) / 8 * 8 : npairs;
    if (any_small) {
        const int n = kp.qwave > 0 ? maxN : std::min(maxN, kQwaveAutoN);
        launch_knn_qwave_batch(s, dim3((n + kWaveBlock / 64 - 1) / (kWaveBlock / 64), gy), tab, kp, use_prev, npairs);
    }
    if (any_large) launch_knn_wave_batch(s, dim3(knn_blocks_of(maxN, kp.packet), gy), tab, kp, use_prev, npairs);
    launch_finish_batch(s, dim3(finish_blocks_of(maxN), gy), tab, kp, it, npairs);
    // exact fallback for uncertified queries: every frame's kFallbackBlocks slabs are written, by
    // fewer physical blocks per frame when many frames share the launch (uncertified queries are
    // rare; a grid of 64 mostly idle blocks per frame cost ~130 µs at 512 frames)
    launch_lane_batch(s, dim3(npairs >= 16 ? kFallbackBlocksBatched : kFallbackBlocks, npairs), tab, kp, it);
}

int project_blocks(int N) { return finish_blocks_of(N) + kFallbackBlocks; }

void launch_project(hipStream_t s, const ProjectLaunch& L) {
    const int wblocks = finish_blocks_of(L.N);
    // tensor voting: every source point's voted normal at this pose first (imls_icp.cpp:514-546)
    if (L.kp.tv) launch_tv_vote(s, L.t, L.spt, L.N, L.pose, L.done, L.kp, const_cast<double4*>(L.t.tvn), L.use_prev);
    if (L.lane_mode || L.kp.proj) {
        // reference mode: every query through the exact per-lane kernel (grid-stride over the
        // fallback slabs); the wave slabs are zeroed
        (void)hipMemsetAsync(L.partial1, 0, (size_t)wblocks * kNormEq * sizeof(double), s);
        launch_lane(s, L, false);
        return;
    }
    if (L.marks) (void)hipEventRecord(L.marks[0], s);
    // sparse query sets (≤ kQwaveAutoN queries, e.g. FPS-sampled frames): one wave per query, with the
    // exact stage in the same kernel for ≤ kSmallRows; dense scans: packets of 64 Morton-coherent
    // queries, then k_finish
    const bool fused = fused_stage(L.kp, L.N);
    if (use_qwave(L.kp, L.N)) launch_knn_qwave(s, L, fused);
    else launch_knn_wave(s, L);
    if (L.marks) (void)hipEventRecord(L.marks[1], s);
    if (!fused) launch_finish(s, L);
    if (L.marks) (void)hipEventRecord(L.marks[2], s);
    // exact fallback for uncertified queries (usually none; the launch exits at once then); the
    // fused small-frame kernel resolves them in place
    if (!fused) launch_lane(s, L, true);
}

}  // namespace imlsgpu
