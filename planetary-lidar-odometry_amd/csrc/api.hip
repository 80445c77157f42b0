// api.hip — the C ABI of include/imls_gpu.h: context, uploads, and the fused per-frame loop.  The
// rest of the ABI: api_map.hip (map FIFO), api_frames.hip (batched registration), api_producer.hip
// (front end … kNN query), api_support.hip (buffer retirement, timing, upload packing); context.h
// is what the units share.
//
// imls_register_frame is the device-resident form of laser_odometry.cpp:478-660: all
// `iterations` × {k_project, solve chain} launches are enqueued back to back on the context
// stream; convergence / too-few-correspondence exits are taken on the device (a `done` flag
// every later launch checks first), so the host synchronises once per frame.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "context.h"
#include "index.h"
#include "solve.h"

using namespace imlsgpu;

// Helpers: the ones context.h declares are called from the other api units too.  All of them are
// hidden, so the library's dynamic symbol table holds the C ABI and nothing of this file besides.
namespace imlsgpu {
#pragma GCC visibility push(hidden)

int fail(imls_ctx* c, int code, const std::string& m) {
    if (c) c->err = m;
    return code;
}

// Grow-only device buffers with 25 % headroom: per-frame sizes vary by a few percent.  A replaced
// buffer is retired, not freed (devbuf_grow below): no reallocation waits for the device.
bool grow(DevBuf& b, size_t bytes) { return devbuf_grow(b, bytes, bytes + bytes / 4 + 256); }

// grow keeping the first `keep` bytes (copied on stream s, a registered stream: the old buffer is
// retired behind the copy)
bool grow_keep(DevBuf& b, size_t bytes, size_t keep, hipStream_t s) {
    if (b.bytes >= bytes) return true;
    if (!b.p || keep == 0) return grow(b, bytes);
    DevBuf nb;
    if (!grow(nb, bytes)) return false;
    if (hipMemcpyAsync(nb.p, b.p, std::min(keep, b.bytes), hipMemcpyDeviceToDevice, s) != hipSuccess) {
        devbuf_retire(nb);
        return false;
    }
    devbuf_retire(b);
    b = nb;
    return true;
}

KParams make_kparams(const imls_params& p, const Options& o) {
    KParams k{};
    k.h2 = p.h * p.h;
    k.r2 = p.r * p.r;
    k.angle_thr_deg = p.angle_diff_threshold;
    k.K = p.search_number;
    k.angle_on = p.normal_angle_constraint ? 1 : 0;
    k.get_normals = p.get_normals ? 1 : 0;
    k.transform_normal = p.transform_normal ? 1 : 0;
    k.correspond_number = p.correspond_number;
    k.solve_method = p.solve_method;
    k.ls_threshold = p.ls_threshold;
    k.delta_dist = p.delta_dist_threshold;
    k.delta_angle = p.delta_angle_threshold;
    // get_normals=false in count mode reads normals recomputed from the map (normals.hip); in the
    // reference's own (dead, Q1) mode every candidate normal is ∞
    if (!p.get_normals && p.recompute_normal_count_mode) k.get_normals = 1;
    k.matcher = p.matching_method;
    // projected-distance gates: IMLS ‖p−x‖ < r_proj, proj < r (imls_icp.cpp:576); plane_ICP keeps the
    // reference's swapped gate ‖p−x‖ < r·r, proj < r_proj (laser_odometry.cpp:322)
    k.proj = p.use_projected_distance ? 1 : 0;
    k.gate_dist = p.r_proj;
    k.gate_proj = p.r;
    if (p.matching_method == IMLS_MATCH_PLANE_ICP) {
        k.proj = p.picp_use_projected_distance ? 1 : 0;
        k.gate_dist = p.picp_r * p.picp_r;
        k.gate_proj = p.picp_r_proj;
        // plane_ICP_proj (laser_odometry.cpp:295-299, 346-350): NN-1 within its own r and angle gate
        k.r2 = p.picp_r * p.picp_r;
        k.K = 1;
        k.angle_on = p.picp_normal_angle_constraint ? 1 : 0;
        k.angle_thr_deg = p.picp_angle_diff_threshold;
    }
    // traversal (imls_set_option, include/imls_gpu.h): −1 auto = one wave per query up to
    // kQwaveAutoN queries (the exact stage fused in for ≤ kSmallRows), packets above
    k.qwave = o.traversal == IMLS_TRAVERSAL_PACKETS ? 0 : o.traversal == IMLS_TRAVERSAL_WAVE_PER_QUERY ? 1 : -1;
    // one frame alone on the GPU (imls_register_frame): its first ICP iteration, where every lane
    // seeds, traverses in 32-query packets (the launch lasts as long as its slowest wave; measured
    // on config B, one pair: k_knn_wave 240 -> 229 us per launch, 8.35 -> 8.14 ms per pair).
    // Batched launches keep 64 (with 4 pairs in flight 32 measured 295 vs 305 pairs/s: the GPU is
    // then throughput-bound and the idle half-waves cost more than the shorter tail saves).
    k.packet = 64;
    k.pk_small = o.first_packet;
    k.pk_iters = o.first_packet_iters;
    k.pk_batch = o.first_packet_batched;
    // Verlet-list reuse (and the prefill certificate), both traversals (round 4: a lone 1949-query
    // frame 1.95 -> 1.84 ms with it on the wave-per-query traversal)
    k.reuse = o.list_reuse;
    k.force_fb = o.force_fallback;
    k.xcd = -1;   // auto: XCD-grouped frames for batches of ≥ 16 frames
    // tensor voting replaces the NN-1 normal only on the IMLS matcher's get_normals=false branch
    // (imls_icp.cpp:514, 630-644); the IMLS neighbours keep the recompute branch (404-434)
    k.tv = (p.use_tensor_voting && !p.get_normals && p.matching_method == IMLS_MATCH_IMLS) ? 1 : 0;
    k.tv_k = p.tensor_k;
    k.tv_sigma = p.tensor_sigma;
    k.tv_thr = p.tensor_distance_threshold;
    k.tv_skin = (float)o.tv_skin;
    k.robust_loss = p.robust_loss;
    k.robust_iters = p.robust_iterations;
    k.robust_scale = p.robust_scale;
    // angle_reject reads "cosine above cos_thr" as "angle below the threshold", which holds for
    // thresholds in [0°, 180°] only.  The reference compares the angle itself (acos(ca)·180/π > thr,
    // any double): outside that range the cosine of the nearer end stands in, and the exact branch
    // of angle_reject, which the cosines within 1e-9 of it and the NaN / out-of-range ones reach,
    // still compares with the threshold as given.  thr < 0: cos_thr = 1 — every cosine below
    // 1 − 1e-9 is rejected, the rest by acos (a number in [−1, 1] gives an angle ≥ 0 > thr; NaN and
    // |ca| > 1 pass).  thr ≥ 180: cos_thr = −1 — every cosine above −1 + 1e-9 passes, the rest by
    // acos (≤ 180 ≤ thr passes, as do NaNs).  A NaN threshold stays NaN: nothing is rejected.
    const double thr = k.angle_thr_deg;
    k.cos_thr = thr < 0.0 ? 1.0 : thr >= 180.0 ? -1.0 : std::cos(thr * M_PI / 180.0);
    return k;
}

int check_params(imls_ctx* c, const imls_params* p) {
    if (!p) return fail(c, IMLS_ERR_ARG, "null params");
    if (p->search_number < 1 || p->search_number > 32) return fail(c, IMLS_ERR_UNSUPPORTED, "search_number must be in [1, 32]");
    if (p->matching_method != IMLS_MATCH_IMLS && p->matching_method != IMLS_MATCH_PLANE_ICP)
        return fail(c, IMLS_ERR_ARG, "matching_method must be IMLS or plane_ICP");
    if (p->use_tensor_voting && !p->get_normals) {
        if (p->tensor_k < 1 || p->tensor_k > kTvMaxK) return fail(c, IMLS_ERR_UNSUPPORTED, "tensor_voting.k must be in [1, 64]");
        if (!(p->tensor_sigma > 0)) return fail(c, IMLS_ERR_ARG, "tensor_voting.sigma must be > 0");
    }
    if (!p->get_normals && p->recompute_normal_count_mode && (p->search_number_normal < 1 || p->search_number_normal > 32))
        return fail(c, IMLS_ERR_ARG, "search_number_normal must be in [1, 32]");
    if (p->solve_method != IMLS_SOLVE_LS && p->solve_method != IMLS_SOLVE_WEIGHTED_LS && p->solve_method != IMLS_SOLVE_RANSAC &&
        p->solve_method != IMLS_SOLVE_ROBUST)
        return fail(c, IMLS_ERR_UNSUPPORTED, "solve_method must be LS, Weighted LS, RANSAC or Robust (Ceres/ICP/Teaser stay on the CPU path)");
    if (p->solve_method == IMLS_SOLVE_ROBUST) {   // (the robust fields are read for this method only)
        if (p->robust_loss != IMLS_ROBUST_HUBER && p->robust_loss != IMLS_ROBUST_CAUCHY && p->robust_loss != IMLS_ROBUST_GEMAN_MCCLURE)
            return fail(c, IMLS_ERR_ARG, "robust_loss must be Huber, Cauchy or Geman-McClure");
        if (p->robust_iterations < 1 || p->robust_iterations > 32) return fail(c, IMLS_ERR_ARG, "robust_iterations must be in [1, 32]");
        if (!std::isfinite(p->robust_scale) || !(p->robust_scale > 0)) return fail(c, IMLS_ERR_ARG, "robust_scale must be finite and > 0");
    }
    if (p->solve_method == IMLS_SOLVE_RANSAC) {
        if (p->ransac_final_method != IMLS_FINAL_LS && p->ransac_final_method != IMLS_FINAL_WEIGHTED_LS &&
            p->ransac_final_method != IMLS_FINAL_DRPM)
            return fail(c, IMLS_ERR_ARG, "RANSAC final_solve_method must be LS, Weighted LS or DRPM");
        if (p->ransac_max_iterations < 1) return fail(c, IMLS_ERR_ARG, "RANSAC max_iterations < 1");
        if (!(p->ransac_ls_threshold >= 0 && p->ransac_ls_threshold < 0.5))
            return fail(c, IMLS_ERR_ARG, "RANSAC LS threshold must be in [0, 0.5)");
    }
    if (p->iterations < 0) return fail(c, IMLS_ERR_ARG, "iterations < 0");
    if (!(p->ls_threshold >= 0 && p->ls_threshold < 0.5)) return fail(c, IMLS_ERR_ARG, "LS threshold must be in [0, 0.5)");
    return IMLS_OK;
}

// Per-N solver / correspondence buffers.
int ensure_solve(imls_ctx* c, int N) {
    if (c->st_N >= N && c->st.trace) return IMLS_OK;
    size_t n = (size_t)std::max(N, 1);
    n += n / 4 + 64;                      // headroom (see grow): the next frames' N differ a little
    // deferred (uncertified) queries: k_finish's wave w writes its count to word w and its queries,
    // in slot order, to the region fb_off + w·64 (finish.hip finish_body, k_project_lane)
    const size_t nfb = (n + 63) / 64;
    c->fb_off = (nfb + 63) / 64 * 64;
    if (!grow(c->cs, n * 16) || !grow(c->cd, n * 16) || !grow(c->cn, n * 16) || !grow(c->fb, (c->fb_off + nfb * 64) * 4))
        return fail(c, IMLS_ERR_DEVICE, "hipMalloc (correspondences)");
    if (!grow(c->prevnn, prevnn_bytes((int)n))) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (prevnn)");
    if (!grow(c->tvn, n * kTvBytesPerQuery)) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (tvn)");
    const int pb = std::max(project_blocks((int)n), solve_blocks((int)n)) + 1;
    size_t bytes = 0;
    auto add = [&](size_t b) { size_t o = bytes; bytes += (b + 255) / 256 * 256; return o; };
    size_t o_pose = add(16 * 8), o_delta = add(16 * 8), o_x0 = add(8 * 8), o_done = add(16), o_status = add(16),
           o_iters = add(16), o_hist = add(kHistBins * 4), o_coarse = add(kHistBins / 256 * 4), o_cc = add(16), o_cl = add((size_t)kCandCap * 8),
           o_clr = add((size_t)kCandCap * 4), o_ch = add((size_t)kCandCap * 8), o_chr = add((size_t)kCandCap * 4),
           o_sel = add(16 * 4), o_p1 = add((size_t)pb * kNormEq * 8), o_p2 = add((size_t)pb * kNormEq * 8),
           o_keys = add(n * 8), o_trace1 = add(sizeof(imls_iter_trace));
    if (!grow(c->solve_mem, bytes)) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (solver)");
    char* b = (char*)c->solve_mem.p;
    SolveState& s = c->st;
    s.pose = (double*)(b + o_pose);
    s.delta = (double*)(b + o_delta);
    s.x0 = (double*)(b + o_x0);
    s.done = (int*)(b + o_done);
    s.status = (int*)(b + o_status);
    s.iters = (int*)(b + o_iters);
    s.hist = (unsigned*)(b + o_hist);
    s.coarse = (unsigned*)(b + o_coarse);
    s.cand_count = (unsigned*)(b + o_cc);
    s.cand_lo = (unsigned long long*)(b + o_cl);
    s.cand_lo_row = (unsigned*)(b + o_clr);
    s.cand_hi = (unsigned long long*)(b + o_ch);
    s.cand_hi_row = (unsigned*)(b + o_chr);
    s.sel = (int*)(b + o_sel);
    s.partial1 = (double*)(b + o_p1);
    s.partial2 = (double*)(b + o_p2);
    s.keys = (double*)(b + o_keys);
    s.trace = (imls_iter_trace*)(b + o_trace1);
    s.partial_cap = pb;
    // the residual histogram is re-zeroed after each use (k_collect); it starts zero
    if (hipMemsetAsync(s.hist, 0, kHistBins * 4, c->stream) != hipSuccess ||
        hipMemsetAsync(s.coarse, 0, kHistBins / 256 * 4, c->stream) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "hipMemset (solver)");
    c->st_N = (int)n;
    return IMLS_OK;
}

RansacParams ransac_params(const imls_params& p) {
    RansacParams r;
    r.max_iterations = p.ransac_max_iterations;
    r.distance_threshold = p.ransac_distance_threshold;
    r.min_inliers_percentage = p.ransac_min_inliers_percentage;
    r.huber_threshold = p.ransac_huber_threshold;
    r.final_method = p.ransac_final_method;
    r.ls_threshold = p.ransac_ls_threshold;
    r.drpm_threshold = p.drpm_threshold;
    r.drpm_stdev_points = p.drpm_stdev_points;
    r.drpm_stdev_normals = p.drpm_stdev_normals;
    return r;
}

// The context's glibc rand() state lives on the device and runs on across every RANSAC solve and
// every frame, like the reference's one process-wide rand() stream (solver.cpp / common.cpp:49 never
// call srand).  It is seeded from params.ransac_seed at context creation, when imls_set_params
// changes ransac_seed, and by imls_seed_rng; imls_set_rng_state hands a stream from one context to
// the next.  Async on the context stream.
int sync_rng(imls_ctx* c) {
    if (!grow(c->rng, 34 * 4)) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (rand state)");
    if (!c->rng_dirty) return IMLS_OK;
    // pinned source, rewritten only after its previous copy ran (ev_rng): no host wait on the stream
    // (a caller that reseeds before every frame keeps its frames in flight)
    if (!c->h_rng && hipHostMalloc((void**)&c->h_rng, 34 * 4) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "hipHostMalloc (rand state)");
    if (!c->ev_rng && hipEventCreateWithFlags(&c->ev_rng, hipEventDisableTiming) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "hipEventCreate (rand state)");
    if (hipEventSynchronize(c->ev_rng) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "rand state upload");
    std::memcpy(c->h_rng, c->rng_seed_state, 34 * 4);
    if (hipMemcpyAsync(c->rng.p, c->h_rng, 34 * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipEventRecord(c->ev_rng, c->stream) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "rand state upload");
    c->rng_dirty = false;
    return IMLS_OK;
}

// RANSAC scratch for `rows` rows and the (persistent) rand() state.
int prepare_ransac(imls_ctx* c, int rows) {
    if (c->P.solve_method != IMLS_SOLVE_RANSAC) return IMLS_OK;
    if (!grow(c->ransac_mem, ransac_bytes(rows))) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (RANSAC)");
    if (ransac_init_tables(c->device)) return fail(c, IMLS_ERR_DEVICE, "RANSAC rand() table upload");
    return sync_rng(c);
}

// count mode: (re)compute the map normals once per (map, search_number_normal, r_normal)
int ensure_map_normals(imls_ctx* c) {
    if (c->P.get_normals || !c->P.recompute_normal_count_mode) return IMLS_OK;
    if (c->rnr_valid && c->rnr_k == c->P.search_number_normal && c->rnr_r == c->P.r_normal) return IMLS_OK;
    if (!grow(c->rnr, (size_t)std::max(c->M, 1) * 16)) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (normals)");
    TreeView t = tree_view(c);
    if (launch_map_normals(c->stream, t, c->P.search_number_normal, c->P.r_normal, (float4*)c->rnr.p))
        return fail(c, IMLS_ERR_DEVICE, "map normal launch failed");
    c->rnr_valid = true;
    c->rnr_k = c->P.search_number_normal;
    c->rnr_r = c->P.r_normal;
    return IMLS_OK;
}

// the context's frame as a projection launch: at `pose` / `done`, trace slot tr, list reuse
// (use_prev) against the last increment `delta`
ProjectLaunch project_launch(imls_ctx* c, const TreeView& t, const KParams& kp, const double* pose, const int* done,
                             imls_iter_trace* tr, const double* delta, int use_prev, hipEvent_t* marks) {
    ProjectLaunch L{};
    L.t = t;
    L.spt = (const float4*)c->spt.p;
    L.snr = (const float4*)c->snr.p;
    L.qperm = (const unsigned*)c->qperm.p;
    L.N = c->N;
    L.pose = pose;
    L.done = done;
    L.delta = delta;
    L.kp = kp;
    L.cs = (float4*)c->cs.p;
    L.cd = (float4*)c->cd.p;
    L.cn = (float4*)c->cn.p;
    L.partial1 = c->st.partial1;
    L.tr = tr;
    L.stats = stats_ptr(c);
    L.fb_list = fb_list(c);
    L.fb_count = fb_count(c);
    L.lists = (int*)c->prevnn.p;
    L.lane_mode = c->lane_mode;
    L.use_prev = use_prev;
    L.marks = marks;
    return L;
}

SolveLaunch solve_launch(imls_ctx* c, imls_iter_trace* tr, int update_pose) {
    SolveLaunch L{};
    L.N = c->N;
    L.blocks1 = project_blocks(c->N);
    L.kp = c->kp;
    L.cs = (const float4*)c->cs.p;
    L.cd = (const float4*)c->cd.p;
    L.cn = (const float4*)c->cn.p;
    L.st = c->st;
    L.tr = tr;
    L.update_pose = update_pose;
    L.scratch = c->ransac_mem.p;
    L.rng = (int*)c->rng.p;
    L.ransac = ransac_params(c->P);
    return L;
}

// Pose-info capture (imls_capture_pose_info).  info_begin, ahead of a solve sequence of up to `rows`
// rows: with capture off it clears SolveState::info (no solve exports, nothing else runs); with it on
// it sizes the buffers, points the solves at the export block and clears that block on stream s.
// Call it before the SolveState is copied into a launch (solve_launch, pair_dev).
constexpr size_t kInfoOutOff = 256, kInfoSlabOff = 256 + (sizeof(struct imls_pose_info) + 255) / 256 * 256;
static_assert(sizeof(InfoExport) <= kInfoOutOff, "export block");
int info_begin(imls_ctx* c, int rows, hipStream_t s) {
    c->info_state = 0;
    c->st.info = nullptr;
    if (!c->info_capture) return IMLS_OK;
    if (!grow(c->info_mem, kInfoSlabOff + (size_t)info_blocks(rows) * kInfoTerms * 8))
        return fail(c, IMLS_ERR_DEVICE, "hipMalloc (pose info)");
    if (!c->h_info && hipHostMalloc((void**)&c->h_info, sizeof(struct imls_pose_info)) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "hipHostMalloc (pose info)");
    c->st.info = (InfoExport*)c->info_mem.p;
    if (hipMemsetAsync(c->info_mem.p, 0, kInfoOutOff, s) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "hipMemset (pose info)");
    return IMLS_OK;
}

// The pass itself, behind the solve sequence on stream s (timed as kind 13 on `timer`, the context
// whose stream s is), and the report's copy into pinned memory.  method: the solve method of the
// sequence; rows_d / weights: the fp64 rows of a host-API solve (null: the projection's float rows);
// N: their count.  RANSAC reads its inlier rows where launch_ransac left them.
int info_enqueue(imls_ctx* c, imls_ctx* timer, hipStream_t s, int method, const double* rows_d, const double* weights, int N,
                 int in_loop) {
    if (!c->st.info) return IMLS_OK;
    char* base = (char*)c->info_mem.p;
    InfoLaunch L{};
    L.N = N;
    L.ex = c->st.info;
    L.status = c->st.status;
    L.iters = c->st.iters;
    L.in_loop = in_loop;
    L.solve_method = method;
    L.robust_loss = c->kp.robust_loss;
    L.robust_scale = c->kp.robust_scale;
    L.slabs = (double*)(base + kInfoSlabOff);
    L.out = (struct imls_pose_info*)(base + kInfoOutOff);
    if (method == IMLS_SOLVE_RANSAC) {
        const int cap = std::max(N, 1);
        const RansacFrame F = ransac_frame(c->ransac_mem.p, cap, (int*)c->rng.p);
        const bool unit = c->P.ransac_final_method == IMLS_FINAL_LS;
        L.final_method = c->P.ransac_final_method;
        L.N = cap;
        L.rows_d = F.inl;
        L.count = F.cnt_in;
        L.weights = unit ? nullptr : F.inl + 9 * (size_t)cap;
        L.wsum = unit ? nullptr : F.wsum;
    } else if (rows_d) {
        L.rows_d = rows_d;
        L.weights = weights;
    } else {
        L.cs = (const float4*)c->cs.p;
        L.cd = (const float4*)c->cd.p;
        L.cn = (const float4*)c->cn.p;
    }
    int slot = -1;
    if (timer->timing == 1) {             // (the light mode 2 keeps to the projection and solve events)
        slot = ev_pair(timer);
        if (slot >= 0) hipEventRecord(timer->ev[slot], s);
    }
    launch_pose_info(s, L);
    if (slot >= 0) {
        hipEventRecord(timer->ev[slot + 1], s);
        timer->ev_pairs[kTimePoseInfo].push_back({slot, slot + 1});
    }
    if (hipMemcpyAsync(c->h_info, L.out, sizeof(struct imls_pose_info), hipMemcpyDeviceToHost, s) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "pose info download");
    c->info_state = 1;
    return IMLS_OK;
}

int ensure_trace(imls_ctx* c, int iters) {
    if (c->trace_cap >= iters && c->h_trace) return IMLS_OK;
    if (!grow(c->trace_mem, (size_t)std::max(iters, 1) * sizeof(imls_iter_trace))) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (trace)");
    if (c->h_trace) (void)hipHostFree(c->h_trace);
    if (hipHostMalloc((void**)&c->h_trace, (size_t)std::max(iters, 1) * sizeof(imls_iter_trace)) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "hipHostMalloc (trace)");
    c->trace_cap = std::max(iters, 1);
    return IMLS_OK;
}

unsigned* fb_count(imls_ctx* c) { return (unsigned*)c->fb.p; }
unsigned long long* stats_ptr(imls_ctx* c) { return c->collect_stats ? (unsigned long long*)c->stats.p : nullptr; }
unsigned* fb_list(imls_ctx* c) { return (unsigned*)c->fb.p + c->fb_off; }

TreeView tree_view(imls_ctx* c) {
    TreeView t;
    t.mpt = (const float4*)c->mpt.p;
    t.mnr = t.mpt ? t.mpt + c->M : nullptr;
    if (!c->P.get_normals && c->P.recompute_normal_count_mode && c->rnr.p) t.mnr = (const float4*)c->rnr.p;
    t.ipos = t.mpt ? (const unsigned*)(t.mpt + 2 * (size_t)c->M) : nullptr;
    t.nodes = (const float4*)c->nodes.p;
    t.tpt = (const float4*)c->tpt.p;
    t.tnr = (const float4*)c->tnr.p;
    t.M = c->M;
    t.B = c->B;
    t.P = c->Pl;
    t.levels = c->levels;
    t.L = c->B > 0 ? (c->M + c->B - 1) / c->B : 0;
    t.lkeys = (const unsigned long long*)c->lkeys.p;
    t.qparams = c->lkeys.p ? (const float*)((const unsigned long long*)c->lkeys.p + t.L) : nullptr;
    t.mten = c->has_tensors ? (const float4*)c->mten.p : nullptr;
    t.tvn = (const double4*)c->tvn.p;
    return t;
}

// Phase B of a pending target build (waits for its filter's kept count).
int finish_target(imls_ctx* c) {
    if (!c->tgt_pending) return IMLS_OK;
    c->tgt_pending = false;
    if (c->fifo_inc) return fifo_build(c);
    if (c->tgt_filter_deferred) {
        c->tgt_filter_deferred = false;
        if (int rc = filter_async(c->stream, c->tf_soa, c->tf_n, c->tpt, c->tnr, c->tscratch, (unsigned*)c->tkept.p,
                                  &c->h_cnt[0], c->err))
            return rc;
        if (hipEventRecord(c->ev_tgt, c->stream) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "event record");
    }
    if (hipEventSynchronize(c->ev_tgt) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "target filter failed");
    c->stage_pending[0] = false;
    c->M = c->h_cnt[0];
    int rc = build_target_tree(c->stream, c->M, c->B, c->lkeys, c->tpt, c->tnr, c->mpt, c->nodes, c->tscratch,
                               c->treescratch, c->permbuf, &c->Pl, &c->levels, c->err);
    timed_end(c, kTimeIndex, c->tgt_slot);
    c->tgt_slot = -1;
    c->has_target = rc == IMLS_OK && c->M > 0;
    if (rc == IMLS_OK && c->ten_pending) {
        c->ten_pending = false;
        if (c->has_target) rc = gather_tensors(c, c->stream, c->ten_src, c->ten_n);
        else c->has_tensors = false;
    }
    return rc;
}

// Phase B of a pending source load.
int finish_source(imls_ctx* c) {
    if (!c->src_pending) return IMLS_OK;
    c->src_pending = false;
    if (c->src_filter_deferred) {
        c->src_filter_deferred = false;
        if (int rc = filter_async(c->stream, c->sf_soa, c->sf_n, c->spt, c->snr, c->sscratch, nullptr, &c->h_cnt[1], c->err))
            return rc;
        if (hipEventRecord(c->ev_src, c->stream) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "event record");
    }
    if (hipEventSynchronize(c->ev_src) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "source filter failed");
    c->stage_pending[1] = false;
    c->N = c->h_cnt[1];
    c->has_source = false;
    if (int rc = source_order(c->stream, c->N, c->spt, c->sscratch, c->qperm, c->err)) return rc;
    if (c->src_kept_out && c->N > 0 &&
        (hipMemcpyAsync(c->src_kept_out, c->skept.p, (size_t)c->N * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
         hipStreamSynchronize(c->stream) != hipSuccess))
        return fail(c, IMLS_ERR_DEVICE, "kept index download failed");
    c->src_kept_out = nullptr;
    c->has_source = c->N > 0;
    return ensure_solve(c, c->N);
}

int ensure_built(imls_ctx* c) {
    if (int rc = finish_target(c)) return rc;
    return finish_source(c);
}

// A count-less load defers its NaN filter to the first use only when the caller asked for deferred
// reads (imls_set_defer: a batch then filters all its members in three launches); otherwise the
// filter is enqueued at once, behind the context's running work, so it overlaps it.  Either way
// the rule the caller sees depends on that switch alone, never on the context's history.
bool defer_filter(const imls_ctx* c) { return c->defer; }

int do_set_target(imls_ctx* c, const float* d_soa6, size_t n, size_t* n_kept) {
    if (n == 0 || n > (size_t)0x7fffffff) return fail(c, IMLS_ERR_ARG, "target size out of range");
    c->fifo_inc = false;
    if (!grow(c->tkept, n * 4 + 16)) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (kept)");
    if (!c->ev_tgt && hipEventCreateWithFlags(&c->ev_tgt, hipEventDisableTiming) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "hipEventCreate");
    c->has_tensors = false;
    c->ten_pending = false;
    c->tgt_pending = false;
    c->tgt_filter_deferred = false;
    timed_begin(c, kTimeIndex, c->tgt_slot);
    if (n_kept || !defer_filter(c)) {
        int rc = filter_async(c->stream, d_soa6, n, c->tpt, c->tnr, c->tscratch, (unsigned*)c->tkept.p, &c->h_cnt[0], c->err);
        if (rc) return rc;
    } else {
        c->tf_soa = d_soa6;                // filtered at first use (alone, or with a whole batch)
        c->tf_n = n;
        c->tgt_filter_deferred = true;
    }
    if (hipEventRecord(c->ev_tgt, c->stream) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "event record");
    c->n_target_in = n;
    c->tgt_pending = true;
    c->has_target = true;                 // provisional: the build decides (an all-NaN map has none)
    c->rnr_valid = false;
    c->has_corr = false;
    if (n_kept) {
        if (int rc2 = finish_target(c)) return rc2;
        *n_kept = (size_t)c->M;
    }
    return IMLS_OK;
}

int do_set_source(imls_ctx* c, const float* d_soa6, size_t n, size_t* n_kept, uint32_t* kept_index) {
    c->cap_iters = 0;                     // a new source drops the captured frame
    if (n == 0 || n > (size_t)0x7fffffff) return fail(c, IMLS_ERR_ARG, "source size out of range");
    if (kept_index && !grow(c->skept, n * 4)) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (kept)");
    if (!c->ev_src && hipEventCreateWithFlags(&c->ev_src, hipEventDisableTiming) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "hipEventCreate");
    c->src_pending = false;
    c->src_filter_deferred = false;
    if (n_kept || kept_index || !defer_filter(c)) {
        int rc = filter_async(c->stream, d_soa6, n, c->spt, c->snr, c->sscratch, kept_index ? (unsigned*)c->skept.p : nullptr,
                              &c->h_cnt[1], c->err);
        if (rc) return rc;
    } else {
        c->sf_soa = d_soa6;
        c->sf_n = n;
        c->src_filter_deferred = true;
    }
    if (hipEventRecord(c->ev_src, c->stream) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "event record");
    c->src_pending = true;
    c->src_kept_out = kept_index;
    c->has_source = true;                 // provisional, as for the target
    c->has_corr = false;
    if (n_kept || kept_index) {
        if (int rc2 = finish_source(c)) return rc2;
        if (n_kept) *n_kept = (size_t)c->N;
    }
    return IMLS_OK;
}

// The target's tensors gathered to Morton order (needs the built target: its kept index and order).
int gather_tensors(imls_ctx* c, hipStream_t s, const float* d_ten6, size_t n) {
    if (!grow(c->mten, (size_t)std::max(c->M, 1) * 32)) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (tensors)");
    launch_tensor_gather(s, d_ten6, n, (const unsigned*)c->tkept.p, (const float4*)c->mpt.p, c->M, (float4*)c->mten.p);
    if (hipGetLastError() != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "tensor gather launch failed");
    return IMLS_OK;
}

// With the target build still pending (a count-less load) the gather waits for it too: it runs
// right after the build (alone, or with a batch's builds), reading d_ten6 then.
int do_set_tensors(imls_ctx* c, const float* d_ten6, size_t n) {
    if (!c->has_target) return fail(c, IMLS_ERR_STATE, "set_target first");
    // (the incremental FIFO index keeps no filtered → input index of the concatenation)
    if (c->fifo_inc) return fail(c, IMLS_ERR_UNSUPPORTED, "tensor inputs need a set_target map, not the FIFO index");
    if (n != c->n_target_in) return fail(c, IMLS_ERR_ARG, "tensor count must equal the last set_target's point count");
    if (c->tgt_pending) {
        c->ten_src = d_ten6;
        c->ten_n = n;
        c->ten_pending = true;
        c->has_tensors = true;
        return IMLS_OK;
    }
    if (!c->has_target) return fail(c, IMLS_ERR_STATE, "set_target first");
    if (int rc = gather_tensors(c, c->stream, d_ten6, n)) return rc;
    c->ten_pending = false;
    c->has_tensors = true;
    return IMLS_OK;
}

// tensor voting needs the target's tensors
int check_tv_ready(imls_ctx* c) {
    if (c->kp.tv && !c->has_tensors) return fail(c, IMLS_ERR_STATE, "use_tensor_voting: imls_set_target_tensors first");
    return IMLS_OK;
}

int check_device(imls_ctx* c) {
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return fail(c, IMLS_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    return IMLS_OK;
}

#pragma GCC visibility pop
}  // namespace imlsgpu

namespace {

// One frame's prologue / epilogue as one launch each (round 4: the lone-frame latency paid ~11 µs
// for an H2D pose copy, five fills and four D2H copies around the 20 iterations).
// (rPose starts at the context's initial pose — imls_set_initial_pose, identity by default — a
// launch argument)
struct Pose16 { double T[16]; };
Pose16 init_pose_of(const imls_ctx* c) {
    Pose16 p;
    std::memcpy(p.T, c->init_pose, sizeof(p.T));
    return p;
}
__global__ void k_frame_init(double* __restrict__ pose, int* __restrict__ done, int* __restrict__ status,
                             int* __restrict__ iters, unsigned long long* __restrict__ trace, int trace_words,
                             unsigned long long* __restrict__ stats, const Pose16 init) {
    const int t = threadIdx.x;
    if (t < 16) pose[t] = init.T[t];
    if (t < 4) { done[t] = 0; status[t] = 0; iters[t] = 0; }
    if (t < 16) stats[t] = 0ull;
    for (int k = t; k < trace_words; k += blockDim.x) trace[k] = 0ull;
}
// pose, iterations, status and the trace records written straight into the pinned host buffers
// (device-visible host memory; read by the host after the stream synchronisation)
__global__ void k_frame_results(const double* __restrict__ pose, const int* __restrict__ iters,
                                const int* __restrict__ status, const unsigned long long* __restrict__ trace,
                                int trace_words, double* __restrict__ h_misc, unsigned long long* __restrict__ h_trace) {
    const int t = threadIdx.x;
    if (t < 16) h_misc[t] = pose[t];
    if (t == 16) reinterpret_cast<int*>(h_misc + 16)[0] = *iters;
    if (t == 17) reinterpret_cast<int*>(h_misc + 18)[0] = *status;
    for (int k = t; k < trace_words; k += blockDim.x) h_trace[k] = trace[k];
}

}  // namespace

extern "C" {

int imls_abi_version(void) { return IMLS_GPU_ABI_VERSION; }

void imls_default_params(imls_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    // config.json shipped values (laser_odometry section)
    p->matching_method = IMLS_MATCH_IMLS;
    p->correspond_number = 6;
    p->h = 1.0;
    p->r = 3.0;
    p->get_normals = 1;
    p->search_number_normal = 10;
    p->r_normal = 1.0;
    p->use_projected_distance = 0;
    p->r_proj = 0.8;
    p->normal_angle_constraint = 1;
    p->angle_diff_threshold = 30.0;
    p->search_number = 20;
    p->use_tensor_voting = 0;
    p->tensor_k = 50;
    p->tensor_sigma = 0.2;
    p->tensor_distance_threshold = 0.6;
    p->picp_r = 1.5;
    p->picp_r_proj = 0.8;
    p->picp_angle_diff_threshold = 30.0;
    p->picp_use_projected_distance = 0;
    p->picp_normal_angle_constraint = 1;
    p->solve_method = IMLS_SOLVE_RANSAC;
    p->iterations = 30;
    p->delta_dist_threshold = 0.001;
    p->delta_angle_threshold = 0.0001745353;
    p->ls_threshold = 0.02;
    p->ransac_max_iterations = 5000;
    p->ransac_final_method = IMLS_FINAL_DRPM;
    p->ransac_distance_threshold = 0.8;
    p->ransac_min_inliers_percentage = 0.95;
    p->ransac_huber_threshold = 0.648;
    p->ransac_ls_threshold = 0.02;
    p->drpm_threshold = 0.05;
    p->drpm_stdev_points = 0.02;
    p->drpm_stdev_normals = 0.05;
    p->ransac_seed = 1;
    p->transform_normal = 0;
    p->max_queue_size = 1;
    p->robust_loss = IMLS_ROBUST_HUBER;
    p->robust_iterations = 5;
    p->robust_scale = 0.1;
}

imls_ctx* imls_create(int device, const imls_params* p) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return nullptr;
    imls_ctx* c = new imls_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return nullptr;
    }
    c->stream = c->own;
    register_stream(c->own, device);
    if (hipHostMalloc((void**)&c->h_misc, 32 * sizeof(double)) != hipSuccess ||
        // coherent: the NaN filter's compaction kernel writes the kept counts here directly
        hipHostMalloc((void**)&c->h_cnt, 4 * sizeof(int), hipHostMallocCoherent) != hipSuccess) {
        delete c;
        return nullptr;
    }
    imls_params d;
    imls_default_params(&d);
    d.solve_method = IMLS_SOLVE_LS;
    if (imls_set_params(c, p ? p : &d) != IMLS_OK) {
        imls_destroy(c);
        return nullptr;
    }
    return c;
}

void imls_destroy(imls_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->ustream) (void)hipStreamSynchronize(c->ustream);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    DevBuf* bufs[] = {&c->knn_q, &c->knn_perm, &c->knn_scratch, &c->knn_lists, &c->knn_fb, &c->knn_pose, &c->knn_up, &c->knn_out,
                      &c->cap_mem, &c->deskew_mem, &c->front_mem, &c->curv_mem, &c->ta_mem, &c->sample_mem, &c->pca_mem, &c->tkept, &c->mten, &c->upload_ten, &c->tvn, &c->rnr, &c->ransac_mem, &c->rng, &c->lkeys, &c->tpt, &c->tnr, &c->mpt, &c->nodes, &c->tscratch, &c->treescratch, &c->permbuf, &c->qperm, &c->fb, &c->prevnn,
                      &c->upload_t, &c->spt, &c->snr, &c->sscratch,
                      &c->upload_s, &c->cs, &c->cd, &c->cn, &c->solve_mem, &c->trace_mem, &c->stats, &c->rows_d, &c->pose_tmp};
    for (DevBuf* b : bufs)
        if (b->p) (void)hipFree(b->p);
    for (DevBuf* b : sweep_buffers(c->sweep))
        if (b->p) (void)hipFree(b->p);
    for (auto* v : {&c->fifo}) for (auto& sl : *v) for (DevBuf* b : {&sl.buf, &sl.fpt, &sl.fnr, &sl.run}) if (b->p) (void)hipFree(b->p);
    for (auto& sl : c->slot_pool) for (DevBuf* b : {&sl.buf, &sl.fpt, &sl.fnr, &sl.run}) if (b->p) (void)hipFree(b->p);
    for (DevBuf* b : {&c->fifo_dev, &c->mkey[0], &c->mkey[1], &c->mval[0], &c->mval[1], &c->fscr}) if (b->p) (void)hipFree(b->p);
    if (c->h_fifo_cnt) (void)hipHostFree(c->h_fifo_cnt);
    if (c->h_fifo_clamp) (void)hipHostFree(c->h_fifo_clamp);
    if (c->ev_fifo) (void)hipEventDestroy(c->ev_fifo);
    for (DevBuf* b : {&c->vox.buf[0], &c->vox.buf[1], &c->vox.scan, &c->vox.scratch}) if (b->p) (void)hipFree(b->p);
    if (c->vox.h_rec) (void)hipHostFree(c->vox.h_rec);
    if (c->vox.ev) (void)hipEventDestroy(c->vox.ev);
    if (c->macc.p) (void)hipFree(c->macc.p);
    if (c->skept.p) (void)hipFree(c->skept.p);
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    if (c->h_trace) (void)hipHostFree(c->h_trace);
    if (c->h_misc) (void)hipHostFree(c->h_misc);
    if (c->h_info) (void)hipHostFree(c->h_info);
    if (c->info_mem.p) (void)hipFree(c->info_mem.p);
    if (c->h_rng) (void)hipHostFree(c->h_rng);
    if (c->ev_rng) (void)hipEventDestroy(c->ev_rng);
    if (c->tab_h) (void)hipHostFree(c->tab_h);
    if (c->h_cnt) (void)hipHostFree(c->h_cnt);
    for (int k = 0; k < 2; ++k) {
        if (c->h_stage[k]) (void)hipHostFree(c->h_stage[k]);
        if (c->ev_stage[k]) (void)hipEventDestroy(c->ev_stage[k]);
    }
    if (c->ev_tgt) (void)hipEventDestroy(c->ev_tgt);
    if (c->ev_src) (void)hipEventDestroy(c->ev_src);
    if (c->res_h) (void)hipHostFree(c->res_h);
    if (c->tab_d.p) (void)hipFree(c->tab_d.p);
    if (c->res_d.p) (void)hipFree(c->res_d.p);
    if (c->ev_batch) (void)hipEventDestroy(c->ev_batch);
    if (c->bscratch.p) (void)hipFree(c->bscratch.p);
    if (c->btable.p) (void)hipFree(c->btable.p);
    if (c->h_btable) (void)hipHostFree(c->h_btable);
    if (c->fscratch.p) (void)hipFree(c->fscratch.p);
    if (c->ftable.p) (void)hipFree(c->ftable.p);
    if (c->h_ftable) (void)hipHostFree(c->h_ftable);
    if (c->ev_build) (void)hipEventDestroy(c->ev_build);
    if (c->stream && c->stream != c->own) unregister_stream(c->stream);
    if (c->ustream) {
        unregister_stream(c->ustream);
        (void)hipStreamDestroy(c->ustream);
    }
    if (c->own) {
        unregister_stream(c->own);
        (void)hipStreamDestroy(c->own);
    }
    release_retired(c->device);
    delete c;
}

int imls_set_params(imls_ctx* c, const imls_params* p) {
    if (!c) return IMLS_ERR_ARG;
    int rc = check_params(c, p);
    if (rc) return rc;
    // the map FIFO's entries are held in the form of the mode they were pushed under (incremental
    // index: filtered points + sorted runs, device scans not copied; concatenation: raw SoA6 copies):
    // the mode may change only while the FIFO is empty
    auto inc_mode = [](int q) { return q >= 2 && q < kMaxFifoRuns; };
    if (c->rng_init && !c->fifo.empty() && inc_mode(c->P.max_queue_size) != inc_mode(p->max_queue_size))
        return fail(c, IMLS_ERR_STATE, "max_queue_size " + std::to_string(c->P.max_queue_size) + " -> " +
                                           std::to_string(p->max_queue_size) +
                                           " changes the map FIFO's index mode while it holds scans: imls_map_clear first");
    if (!c->rng_init || p->ransac_seed != c->P.ransac_seed) {   // creation, or a new seed: restart the stream
        c->rng_init = true;
        ransac_seed_host(p->ransac_seed, c->rng_seed_state);
        c->rng_dirty = true;
    }
    c->P = *p;
    c->kp = make_kparams(*p, c->opt);
    return IMLS_OK;
}

int imls_set_option(imls_ctx* c, int32_t option, double value) {
    if (!c) return IMLS_ERR_ARG;
    if (!std::isfinite(value)) return fail(c, IMLS_ERR_ARG, "option value must be finite");
    const int v = (int)value;
    const bool integral = (double)v == value;
    Options& o = c->opt;
    switch (option) {
    case IMLS_OPT_TRAVERSAL:
        if (!integral || v < IMLS_TRAVERSAL_AUTO || v > IMLS_TRAVERSAL_LANE) return fail(c, IMLS_ERR_ARG, "traversal: 0..3");
        o.traversal = v;
        break;
    case IMLS_OPT_LIST_REUSE:
        if (!integral || (v != 0 && v != 1)) return fail(c, IMLS_ERR_ARG, "list_reuse: 0 or 1");
        o.list_reuse = v;
        break;
    case IMLS_OPT_TEMPORAL_SEED:
        if (!integral || (v != 0 && v != 1)) return fail(c, IMLS_ERR_ARG, "temporal_seed: 0 or 1");
        o.temporal_seed = v;
        break;
    case IMLS_OPT_LEAF_SIZE:   // a leaf is one wave-wide load
        if (!integral || v < 4 || v > 64 || (v & (v - 1))) return fail(c, IMLS_ERR_ARG, "leaf_size: a power of two in [4, 64]");
        o.leaf_size = v;
        break;
    case IMLS_OPT_FIRST_PACKET:
        if (!integral || (v != 16 && v != 32 && v != 64)) return fail(c, IMLS_ERR_ARG, "first_packet: 16, 32 or 64");
        o.first_packet = v;
        break;
    case IMLS_OPT_FIRST_PACKET_ITERS:
        if (!integral || v < 0) return fail(c, IMLS_ERR_ARG, "first_packet_iters: >= 0");
        o.first_packet_iters = v;
        break;
    case IMLS_OPT_FIRST_PACKET_BATCHED:
        if (!integral || (v != 0 && v != 1)) return fail(c, IMLS_ERR_ARG, "first_packet_batched: 0 or 1");
        o.first_packet_batched = v;
        break;
    case IMLS_OPT_TV_SKIN:
        if (value < 0.0 || value > 1.0) return fail(c, IMLS_ERR_ARG, "tv_skin: [0, 1] m");
        o.tv_skin = value;
        break;
    case IMLS_OPT_FORCE_FALLBACK:
        if (!integral || v < 0) return fail(c, IMLS_ERR_ARG, "force_fallback: >= 0");
        o.force_fallback = v;
        break;
    default:
        return fail(c, IMLS_ERR_ARG, "unknown option");
    }
    c->B = o.leaf_size;                          // the next index build
    c->lane_mode = o.traversal == IMLS_TRAVERSAL_LANE;
    c->temporal_seed = o.temporal_seed;
    c->kp = make_kparams(c->P, o);
    return IMLS_OK;
}

int imls_get_option(imls_ctx* c, int32_t option, double* value) {
    if (!c || !value) return IMLS_ERR_ARG;
    const Options& o = c->opt;
    switch (option) {
    case IMLS_OPT_TRAVERSAL: *value = o.traversal; break;
    case IMLS_OPT_LIST_REUSE: *value = o.list_reuse; break;
    case IMLS_OPT_TEMPORAL_SEED: *value = o.temporal_seed; break;
    case IMLS_OPT_LEAF_SIZE: *value = o.leaf_size; break;
    case IMLS_OPT_FIRST_PACKET: *value = o.first_packet; break;
    case IMLS_OPT_FIRST_PACKET_ITERS: *value = o.first_packet_iters; break;
    case IMLS_OPT_FIRST_PACKET_BATCHED: *value = o.first_packet_batched; break;
    case IMLS_OPT_TV_SKIN: *value = o.tv_skin; break;
    case IMLS_OPT_FORCE_FALLBACK: *value = o.force_fallback; break;
    default: return fail(c, IMLS_ERR_ARG, "unknown option");
    }
    return IMLS_OK;
}

const char* imls_last_error(const imls_ctx* c) { return c ? c->err.c_str() : "null context"; }

int imls_seed_rng(imls_ctx* c, uint32_t seed) {
    if (!c) return IMLS_ERR_ARG;
    // the stream restarts; params.ransac_seed is left as set (contexts seeded differently still
    // batch together: frames_async compares the params without it)
    ransac_seed_host(seed, c->rng_seed_state);
    c->rng_dirty = true;
    return IMLS_OK;
}

int imls_get_rng_state(imls_ctx* c, int32_t state[34]) {
    if (!c || !state) return IMLS_ERR_ARG;
    if (c->rng_dirty || !c->rng.p) {                  // not on the device yet: the pending seed is the state
        std::memcpy(state, c->rng_seed_state, 34 * 4);
        return IMLS_OK;
    }
    if (int rc = check_device(c)) return rc;
    if (hipMemcpyAsync(state, c->rng.p, 34 * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "rand state download");
    return IMLS_OK;
}

int imls_set_rng_state(imls_ctx* c, const int32_t state[34]) {
    if (!c || !state) return IMLS_ERR_ARG;
    const int f = state[31], r = state[32];
    if (f < 0 || f > 30 || r < 0 || r > 30 || (f - r + 31) % 31 != 3) return fail(c, IMLS_ERR_ARG, "not a glibc TYPE_3 rand() state");
    std::memcpy(c->rng_seed_state, state, 34 * 4);
    c->rng_dirty = true;
    return IMLS_OK;
}

int imls_set_stream(imls_ctx* c, void* s) {
    if (!c) return IMLS_ERR_ARG;
    hipStream_t ns = s ? (hipStream_t)s : c->own;
    if (ns != c->stream) {
        // a caller's stream joins the registry (its pending work may read this context's buffers)
        if (ns != c->own) register_stream(ns, c->device);
        if (c->stream != c->own) unregister_stream(c->stream);
    }
    c->stream = ns;
    return IMLS_OK;
}

int imls_synchronize(imls_ctx* c) {
    if (!c) return IMLS_ERR_ARG;
    return hipStreamSynchronize(c->stream) == hipSuccess ? IMLS_OK : fail(c, IMLS_ERR_DEVICE, "stream sync failed");
}

int imls_set_target(imls_ctx* c, const float* xyz, const float* nrm, size_t n, size_t stride, size_t* n_kept) {
    if (!c) return IMLS_ERR_ARG;
    if (int rc = check_device(c)) return rc;
    if (int rc = upload_soa6(c, c->upload_t, xyz, nrm, n, stride, 0)) return rc;
    return do_set_target(c, (const float*)c->upload_t.p, n, n_kept);
}

int imls_set_target_device(imls_ctx* c, const float* d_soa6, size_t n, size_t* n_kept) {
    if (!c || !d_soa6) return IMLS_ERR_ARG;
    if (int rc = check_device(c)) return rc;
    return do_set_target(c, d_soa6, n, n_kept);
}

int imls_set_target_tensors(imls_ctx* c, const float* tens, size_t n, size_t stride) {
    if (!c || !tens || n == 0 || stride < 6) return fail(c, IMLS_ERR_ARG, "bad tensor pointer/size/stride");
    if (int rc = check_device(c)) return rc;
    std::vector<float> h(6 * n);
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 6; ++k) h[(size_t)k * n + i] = tens[i * stride + k];
    if (!grow(c->upload_ten, h.size() * 4)) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (upload)");
    if (hipMemcpyAsync(c->upload_ten.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "tensor upload failed");
    int rc = do_set_tensors(c, (const float*)c->upload_ten.p, n);
    if (rc) return rc;
    return hipStreamSynchronize(c->stream) == hipSuccess ? IMLS_OK : fail(c, IMLS_ERR_DEVICE, "tensor upload failed");
}

int imls_set_target_tensors_device(imls_ctx* c, const float* d_ten6, size_t n) {
    if (!c || !d_ten6) return IMLS_ERR_ARG;
    if (int rc = check_device(c)) return rc;
    return do_set_tensors(c, d_ten6, n);
}

void imls_tv_encode_pca(const float* evals, const float* evecs, size_t n, int32_t k, float* out) {
    // CustomTensorVoting::myCustomFunctionWithEigen (scan_registration.cpp:358-381), float arithmetic
    const float kf = (float)k;
    for (size_t i = 0; i < n; ++i) {
        const float a0 = std::fabs(evals[3 * i]), a1 = std::fabs(evals[3 * i + 1]), a2 = std::fabs(evals[3 * i + 2]);
        const float l1 = std::max(a0, std::max(a1, a2));
        const float l3 = std::min(a0, std::min(a1, a2));
        const float l2 = ((a0 + a1) + a2) - (l1 + l3);
        const float* e = evecs + 9 * i;           // columns: e1 = e[0..2] (stick tail), e2 = e[3..5] (plate tail)
        float T[6];
        if (l1 >= l2 && l2 >= l3) {
            const float s1 = (l1 - l2) / kf, s3 = l3 / kf;
            const int rr[6] = {0, 0, 0, 1, 1, 2}, cc[6] = {0, 1, 2, 1, 2, 2};
            for (int m = 0; m < 6; ++m) {
                const float S = e[rr[m]] * e[cc[m]];
                const float Pm = S + e[3 + rr[m]] * e[3 + cc[m]];
                T[m] = s1 * S + s3 * Pm;
            }
        } else {
            T[0] = 1.f; T[1] = 0.f; T[2] = 0.f; T[3] = 1.f; T[4] = 0.f; T[5] = 1.f;   // unit ball (377-380)
        }
        for (int m = 0; m < 6; ++m) out[6 * i + m] = T[m];
    }
}

int imls_set_source(imls_ctx* c, const float* xyz, const float* nrm, size_t n, size_t stride, size_t* n_kept,
                    uint32_t* kept_index) {
    if (!c) return IMLS_ERR_ARG;
    if (int rc = check_device(c)) return rc;
    if (int rc = upload_soa6(c, c->upload_s, xyz, nrm, n, stride, 1)) return rc;
    return do_set_source(c, (const float*)c->upload_s.p, n, n_kept, kept_index);
}

int imls_set_source_device(imls_ctx* c, const float* d_soa6, size_t n, size_t* n_kept) {
    if (!c || !d_soa6) return IMLS_ERR_ARG;
    if (int rc = check_device(c)) return rc;
    return do_set_source(c, d_soa6, n, n_kept, nullptr);
}

int imls_project(imls_ctx* c, const double pose[16], float* x_out, float* y_out, float* n_out, uint32_t* src_index_out,
                 size_t* n_valid, uint64_t reject[IMLS_NUM_REJ]) {
    if (!c || !pose) return IMLS_ERR_ARG;
    if (int rc = check_device(c)) return rc;
    if (int rc = ensure_built(c)) return rc;
    if (!c->has_target || !c->has_source) return fail(c, IMLS_ERR_STATE, "set_target and set_source first");
    if (int rc = ensure_solve(c, c->N)) return rc;
    if (int rc = check_tv_ready(c)) return rc;
    if (int rc = ensure_map_normals(c)) return rc;
    if (!grow(c->pose_tmp, 32 * 8) || !grow(c->stats, 128)) return fail(c, IMLS_ERR_DEVICE, "hipMalloc");
    double* dpose = (double*)c->pose_tmp.p;
    int* dzero = (int*)(dpose + 16);
    hipMemcpyAsync(dpose, pose, 16 * 8, hipMemcpyHostToDevice, c->stream);
    hipMemsetAsync(dzero, 0, 16, c->stream);
    hipMemsetAsync(c->st.trace, 0, sizeof(imls_iter_trace), c->stream);
    hipMemsetAsync(c->stats.p, 0, 128, c->stream);
    int slot;
    hipEvent_t marks[3];
    timed_begin(c, kTimeProject, slot);
    launch_project(c->stream,
                   project_launch(c, tree_view(c), c->kp, dpose, dzero, c->st.trace, nullptr, 0, project_marks(c, marks)));
    timed_end(c, kTimeProject, slot);
    std::vector<float> hs((size_t)c->N * 4), hd((size_t)c->N * 4), hn((size_t)c->N * 4);
    imls_iter_trace tr;
    hipMemcpyAsync(hs.data(), c->cs.p, hs.size() * 4, hipMemcpyDeviceToHost, c->stream);
    hipMemcpyAsync(hd.data(), c->cd.p, hd.size() * 4, hipMemcpyDeviceToHost, c->stream);
    hipMemcpyAsync(hn.data(), c->cn.p, hn.size() * 4, hipMemcpyDeviceToHost, c->stream);
    hipMemcpyAsync(&tr, c->st.trace, sizeof(tr), hipMemcpyDeviceToHost, c->stream);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, std::string("project: ") + hipGetErrorString(hipGetLastError()));
    harvest_timing(c);
    size_t k = 0;
    for (int i = 0; i < c->N; ++i) {
        if (hs[4 * i + 3] == 0.f) continue;
        for (int d = 0; d < 3; ++d) {
            if (x_out) x_out[3 * k + d] = hs[4 * i + d];
            if (y_out) y_out[3 * k + d] = hd[4 * i + d];
            if (n_out) n_out[3 * k + d] = hn[4 * i + d];
        }
        if (src_index_out) src_index_out[k] = (uint32_t)i;
        ++k;
    }
    if (n_valid) *n_valid = k;
    if (reject) std::memcpy(reject, tr.reject, sizeof(tr.reject));
    c->has_corr = true;
    return IMLS_OK;
}

int imls_solve(imls_ctx* c, double delta_out[16], int* ok) {
    if (!c || !delta_out) return IMLS_ERR_ARG;
    c->info_state = 0;
    if (!c->has_corr) return fail(c, IMLS_ERR_STATE, "imls_project first");
    if (int rc = check_device(c)) return rc;
    hipMemsetAsync(c->st.done, 0, 16, c->stream);
    hipMemsetAsync(c->st.status, 0, 16, c->stream);
    if (int rc = prepare_ransac(c, c->N)) return rc;
    if (int rc = info_begin(c, c->N, c->stream)) return rc;
    int slot;
    timed_begin(c, kTimeSolve, slot);
    launch_solve(c->stream, solve_launch(c, nullptr, 0));
    timed_end(c, kTimeSolve, slot);
    if (int rc = info_enqueue(c, c, c->stream, c->P.solve_method, nullptr, nullptr, c->N, 0)) return rc;
    int status = 0;
    hipMemcpyAsync(delta_out, c->st.delta, 16 * 8, hipMemcpyDeviceToHost, c->stream);
    hipMemcpyAsync(&status, c->st.status, sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "solve failed");
    harvest_timing(c);
    if (c->info_state == 1) c->info_state = 2;
    if (ok) *ok = status == IMLS_FRAME_SOLVE_FAILED ? 0 : 1;
    return IMLS_OK;
}

int imls_solve_correspondences(imls_ctx* c, int32_t method, const double* s, const double* d, const double* n,
                               const double* w, size_t N, double delta_out[16], int* ok) {
    if (!c || !s || !d || !n || !delta_out) return IMLS_ERR_ARG;
    c->info_state = 0;
    if (method != IMLS_SOLVE_LS && method != IMLS_SOLVE_WEIGHTED_LS && method != IMLS_SOLVE_RANSAC &&
        method != IMLS_SOLVE_DRPM && method != IMLS_SOLVE_ROBUST)
        return fail(c, IMLS_ERR_UNSUPPORTED, "method");
    if (N > (size_t)0x3fffffff) return fail(c, IMLS_ERR_ARG, "N too large");
    if (method == IMLS_SOLVE_ROBUST && c->P.solve_method != IMLS_SOLVE_ROBUST) {
        // the robust fields of the params in force were not checked under another method
        imls_params q = c->P;
        q.solve_method = IMLS_SOLVE_ROBUST;
        if (int rc = check_params(c, &q)) return rc;
    }
    if (int rc = check_device(c)) return rc;
    if (int rc = ensure_solve(c, (int)std::max<size_t>(N, 1))) return rc;
    size_t bytes = (9 * N + N) * 8 + 64;
    if (!grow(c->rows_d, bytes)) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (rows)");
    double* r = (double*)c->rows_d.p;
    hipMemcpyAsync(r, s, 3 * N * 8, hipMemcpyHostToDevice, c->stream);
    hipMemcpyAsync(r + 3 * N, d, 3 * N * 8, hipMemcpyHostToDevice, c->stream);
    hipMemcpyAsync(r + 6 * N, n, 3 * N * 8, hipMemcpyHostToDevice, c->stream);
    const double* dw = nullptr;
    if (w) {
        hipMemcpyAsync(r + 9 * N, w, N * 8, hipMemcpyHostToDevice, c->stream);
        dw = r + 9 * N;
    }
    hipMemsetAsync(c->st.done, 0, 16, c->stream);
    hipMemsetAsync(c->st.status, 0, 16, c->stream);
    const int saved = c->P.solve_method;
    c->P.solve_method = method;
    const int rc0 = prepare_ransac(c, (int)std::max<size_t>(N, 1));
    c->P.solve_method = saved;
    if (rc0) return rc0;
    if (method == IMLS_SOLVE_DRPM && !grow(c->ransac_mem, ransac_bytes((int)std::max<size_t>(N, 1))))
        return fail(c, IMLS_ERR_DEVICE, "hipMalloc (DRPM)");
    if (int rc = info_begin(c, (int)std::max<size_t>(N, 1), c->stream)) return rc;
    SolveLaunch L = solve_launch(c, nullptr, 0);
    L.N = (int)N;
    L.blocks1 = 0;
    L.kp.solve_method = method;
    L.cs = L.cd = L.cn = nullptr;
    L.rows_d = r;
    L.weights = dw;
    L.rows_are_double = 1;
    launch_solve(c->stream, L);
    if (int rc = info_enqueue(c, c, c->stream, method, r, dw, (int)N, 0)) return rc;
    int status = 0;
    hipMemcpyAsync(delta_out, c->st.delta, 16 * 8, hipMemcpyDeviceToHost, c->stream);
    hipMemcpyAsync(&status, c->st.status, sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "solve failed");
    if (c->info_state == 1) {
        harvest_timing(c);
        c->info_state = 2;
    }
    if (ok) *ok = status == IMLS_FRAME_SOLVE_FAILED ? 0 : 1;
    return IMLS_OK;
}

int imls_register_frame_async(imls_ctx* c) {
    if (!c) return IMLS_ERR_ARG;
    c->info_state = 0;                    // whatever happens below, the previous frame's report is gone
    if (c->batch_member) return fail(c, IMLS_ERR_STATE, "the context is part of a pending batch");
    if (int rc = check_device(c)) return rc;
    if (int rc = ensure_built(c)) return rc;
    if (!c->has_target || !c->has_source) return fail(c, IMLS_ERR_STATE, "set_target and set_source first");
    if (int rc = ensure_solve(c, c->N)) return rc;
    if (int rc = check_tv_ready(c)) return rc;
    const int iters = c->P.iterations;
    if (int rc = ensure_trace(c, iters)) return rc;
    if (!grow(c->stats, 128)) return fail(c, IMLS_ERR_DEVICE, "hipMalloc");
    const int trace_words = std::max(iters, 1) * (int)(sizeof(imls_iter_trace) / 8);
    k_frame_init<<<1, 256, 0, c->stream>>>(c->st.pose, c->st.done, c->st.status, c->st.iters,
                                           (unsigned long long*)c->trace_mem.p, trace_words,
                                           (unsigned long long*)c->stats.p, init_pose_of(c));
    imls_iter_trace* tr = (imls_iter_trace*)c->trace_mem.p;
    if (int rc = ensure_map_normals(c)) return rc;
    const TreeView tv = tree_view(c);
    if (int rc = prepare_ransac(c, c->N)) return rc;
    if (int rc = info_begin(c, c->N, c->stream)) return rc;
    c->cap_iters = 0;
    c->cap_run = -1;
    if (c->capture && iters > 0) {
        if (!grow(c->cap_mem, (size_t)iters * c->N * 48)) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (capture)");
        c->cap_iters = iters;
        c->cap_N = c->N;
    }
    for (int it = 0; it < iters; ++it) {
        int slot;
        hipEvent_t marks[3];
        timed_begin(c, kTimeProject, slot);
        launch_project(c->stream, project_launch(c, tv, kp_at(c->kp, it), c->st.pose, c->st.done, tr + it, c->st.delta,
                                                 it > 0 && c->temporal_seed, project_marks(c, marks)));
        timed_end(c, kTimeProject, slot);
        if (c->cap_iters) {   // this iteration's correspondences (stale, and never read, once the frame stopped)
            char* dst = (char*)c->cap_mem.p + (size_t)it * c->N * 48;
            const size_t nb = (size_t)c->N * 16;
            if (hipMemcpyAsync(dst, c->cs.p, nb, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
                hipMemcpyAsync(dst + nb, c->cd.p, nb, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
                hipMemcpyAsync(dst + 2 * nb, c->cn.p, nb, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) {
                c->cap_iters = 0;
                return fail(c, IMLS_ERR_DEVICE, "capture copy");
            }
        }
        timed_begin(c, kTimeSolve, slot);
        launch_solve(c->stream, solve_launch(c, tr + it, 1));
        timed_end(c, kTimeSolve, slot);
    }
    if (int rc = info_enqueue(c, c, c->stream, c->P.solve_method, nullptr, nullptr, c->N, 1)) return rc;
    k_frame_results<<<1, 256, 0, c->stream>>>(c->st.pose, c->st.iters, c->st.status, (const unsigned long long*)tr,
                                              iters * (int)(sizeof(imls_iter_trace) / 8), c->h_misc,
                                              (unsigned long long*)c->h_trace);
    if (hipGetLastError() != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "launch failed");
    c->pending = true;
    c->pending_iters = iters;
    c->has_corr = true;
    return IMLS_OK;
}

int imls_register_frame_result(imls_ctx* c, double pose_out[16], int* iters_run, int* status, imls_iter_trace* trace) {
    if (!c) return IMLS_ERR_ARG;
    if (!c->pending) return fail(c, IMLS_ERR_STATE, "no frame pending");
    c->pending = false;
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, IMLS_ERR_DEVICE, std::string("frame failed: ") + hipGetErrorString(e));
    harvest_timing(c);
    if (c->info_state == 1) c->info_state = 2;
    const int* misc = (const int*)(c->h_misc + 16);     // iters (pinned, copied by register_frame_async)
    const int st = *(const int*)(c->h_misc + 18);       // status
    if (pose_out) std::memcpy(pose_out, c->h_misc, 16 * 8);
    if (iters_run) *iters_run = misc[0];
    if (status) *status = st;
    if (c->cap_iters) c->cap_run = misc[0];
    if (trace && c->pending_iters > 0) std::memcpy(trace, c->h_trace, (size_t)c->pending_iters * sizeof(imls_iter_trace));
    return IMLS_OK;
}

int imls_register_frame(imls_ctx* c, double pose_out[16], int* iters_run, int* status, imls_iter_trace* trace) {
    int rc = imls_register_frame_async(c);
    if (rc) return rc;
    return imls_register_frame_result(c, pose_out, iters_run, status, trace);
}

int imls_capture_correspondences(imls_ctx* c, int on) {
    if (!c) return IMLS_ERR_ARG;
    c->capture = on != 0;
    return IMLS_OK;
}

int imls_captured_correspondences(imls_ctx* c, int iter, size_t cap, float* x_out, float* y_out, float* n_out,
                                  uint32_t* src_index_out, size_t* n_valid) {
    if (!c || !n_valid) return IMLS_ERR_ARG;
    if (c->pending) return fail(c, IMLS_ERR_STATE, "collect the frame first (imls_register_frame_result)");
    // the captured frame's iterations only: a later set_source or batch drops the capture (its rows
    // index the old source), and iterations at or past the frame's iters_run hold stale rows
    if (c->cap_iters == 0 || c->cap_run < 0) return fail(c, IMLS_ERR_STATE, "no captured frame");
    if (iter < 0 || iter >= std::min(c->cap_iters, c->cap_run))
        return fail(c, IMLS_ERR_STATE, "no captured iteration " + std::to_string(iter));
    if (int rc = check_device(c)) return rc;
    const size_t N = (size_t)c->cap_N;
    std::vector<float> h(N * 12);
    if (hipMemcpy(h.data(), (const char*)c->cap_mem.p + (size_t)iter * N * 48, N * 48, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "capture download");
    const float *hs = h.data(), *hd = hs + 4 * N, *hn = hs + 8 * N;
    size_t nv = 0;
    for (size_t i = 0; i < N; ++i) nv += hs[4 * i + 3] != 0.f ? 1 : 0;
    *n_valid = nv;
    const bool want = x_out || y_out || n_out || src_index_out;
    if (!want) return IMLS_OK;            // size query
    if (nv > cap) return fail(c, IMLS_ERR_ARG, "capacity " + std::to_string(cap) + " < " + std::to_string(nv) + " rows");
    size_t k = 0;
    for (size_t i = 0; i < N; ++i) {
        if (hs[4 * i + 3] == 0.f) continue;   // rejected (erased from in_cloud by the reference)
        for (int d = 0; d < 3; ++d) {
            if (x_out) x_out[3 * k + d] = hs[4 * i + d];
            if (y_out) y_out[3 * k + d] = hd[4 * i + d];
            if (n_out) n_out[3 * k + d] = hn[4 * i + d];
        }
        if (src_index_out) src_index_out[k] = (uint32_t)i;
        ++k;
    }
    return IMLS_OK;
}

int imls_capture_pose_info(imls_ctx* c, int on) {
    if (!c) return IMLS_ERR_ARG;
    c->info_capture = on != 0;
    return IMLS_OK;
}

int imls_pose_info(imls_ctx* c, struct imls_pose_info* out) {
    if (!c || !out) return IMLS_ERR_ARG;
    if (c->info_state == 1) return fail(c, IMLS_ERR_STATE, "collect the result first");
    if (c->info_state != 2) return fail(c, IMLS_ERR_STATE, "pose-info capture was off for the last solve (imls_capture_pose_info)");
    std::memcpy(out, c->h_info, sizeof(*out));
    return IMLS_OK;
}

int imls_set_defer(imls_ctx* c, int on) {
    if (!c) return IMLS_ERR_ARG;
    c->defer = on != 0;
    return IMLS_OK;
}

}  // extern "C"
