// api_producer.hip — the producer side of the C ABI: scan front end, ring PCA, samplers, curvature
// presample, three_axis, random, sweep, deskew, and the public kNN query.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "context.h"
#include "index.h"

using namespace imlsgpu;

extern "C" {

void imls_default_front_params(imls_front_params* p) {
    if (!p) return;
    p->n_scans = 64;            // planetary_slam_VLP_32.launch: scan_line 64, minimum_range 2, maximum_range 150
    p->minimum_range = 2.0f;
    p->maximum_range = 150.0f;
    p->scan_period = 0.1f;      // scan_registration.cpp:55
    p->is_dense = 0;
}

int imls_scan_front_end(imls_ctx* c, const imls_front_params* p, const float* xyz, size_t stride_floats, size_t n,
                        float* out_xyzi, uint32_t* out_index, int32_t* ring_sizes, size_t* n_out) {
    if (!c || !p || !out_xyzi || !ring_sizes || !n_out || (n > 0 && !xyz)) return IMLS_ERR_ARG;
    if (int rc = check_device(c)) return rc;
    int slot;
    timed_begin(c, kTimeFrontEnd, slot);
    const int rc = front_end_run(c->stream, *p, xyz, stride_floats, n, c->front_mem, out_xyzi, out_index, ring_sizes,
                                 n_out, c->err);
    timed_end(c, kTimeFrontEnd, slot);
    harvest_timing(c);
    return rc;
}

void imls_default_pca_params(imls_pca_params* p) {
    // scan_registration section of the shipped config.json (read at scan_registration.cpp:1140-1145, 1451, 1133)
    if (!p) return;
    p->window_size = 3;
    p->iter_step = 1;
    p->knn_distance_threshold = 10.f;
    p->neighbor_scan = 0;
    p->distance_threshold = 0.02f;
    p->valid_points_threshold = 0.8f;
    p->use_all_points = 1;
    p->planarity_threshold = 0.05f;
}

int imls_ring_normals_pca(imls_ctx* c, const imls_pca_params* p, const float* xyz, size_t stride,
                          const int32_t* ring_sizes, int32_t n_rings, uint32_t* index_out, float* normal_out,
                          float* evals_out, float* evecs_out, float* features_out, uint8_t* flags_out, size_t* n_out,
                          uint64_t counters[2]) {
    if (!c) return IMLS_ERR_ARG;
    if (!p || !ring_sizes || n_rings <= 0 || n_rings > 4096 || stride < 3)
        return fail(c, IMLS_ERR_ARG, "bad pca params / ring sizes / stride");
    if (p->window_size < 0 || p->iter_step <= 0 || p->neighbor_scan < 0 || p->neighbor_scan > 1)
        return fail(c, IMLS_ERR_ARG, "bad pca window_size / iter_step / neighbor_scan");
    long long total = 0;
    for (int i = 0; i < n_rings; ++i) total += ring_sizes[i];
    if (total > 0 && !xyz) return fail(c, IMLS_ERR_ARG, "null xyz");
    if (total >= (1ll << 31)) return fail(c, IMLS_ERR_CAPACITY, "cloud too large");
    if (int rc = check_device(c)) return rc;
    int slot;
    hipEvent_t marks[2];
    hipEvent_t* mk = pair_marks(c, marks, slot);
    if (mk) c->ev_pairs[kTimeRingPca].push_back({slot, slot + 1});
    int rc = ring_pca_run(c->stream, *p, xyz, stride, ring_sizes, n_rings, c->pca_mem, mk, index_out, normal_out,
                          evals_out, evecs_out, features_out, flags_out, n_out, counters, c->err);
    if (c->timing) harvest_timing(c);
    return rc;
}

void imls_default_sample_params(imls_sample_params* p, int32_t method) {
    // scan_registration.sample_method.{normal, major_axis} of the shipped config.json (784-799)
    if (!p) return;
    p->method = method;
    p->r = 0.5f;
    p->r_proj = 1.5f;
    p->max_total_points = 2000;
    p->azimuth_bins = 8;
    p->elevation_bins = 8;
    p->min_points_per_bin = 20;
    p->max_points_per_bin = method == IMLS_SAMPLE_NORMAL ? 100 : 200;
    p->sampling_strategy = method == IMLS_SAMPLE_NORMAL ? 1 : 0;   // normal: "random", major_axis: "FPS"
    p->shuffle_seed = 0;
    p->rand_seed = 1;
}

int imls_sample_point_cloud(imls_ctx* c, const imls_sample_params* p, const float* xyz, const float* nrm,
                            size_t stride, size_t n, const int32_t* candidates, size_t n_cand, const float* last_xyz,
                            size_t last_stride, size_t m, int32_t* sampled_out, size_t* n_sampled,
                            float* bin_weights_out) {
    if (!c) return IMLS_ERR_ARG;
    if (!p || stride < 3 || (n_cand > 0 && (!xyz || !nrm || !candidates || !sampled_out)))
        return fail(c, IMLS_ERR_ARG, "bad sample params / pointers / stride");
    if (p->method < 0 || p->method > 1 || p->azimuth_bins <= 0 || p->elevation_bins <= 0 || p->azimuth_bins > 1024 ||
        p->elevation_bins > 1024 || p->sampling_strategy < 0 || p->sampling_strategy > 1)
        return fail(c, IMLS_ERR_ARG, "bad sample method / bins / strategy");
    if (p->method == IMLS_SAMPLE_MAJOR_AXIS && m > 0 && (!last_xyz || last_stride < 3))
        return fail(c, IMLS_ERR_ARG, "major_axis needs last_pcl_cloud");
    if (n >= (1ull << 31) || m >= (1ull << 31)) return fail(c, IMLS_ERR_CAPACITY, "cloud too large");
    if (int rc = check_device(c)) return rc;
    int slot;
    hipEvent_t marks[2];
    hipEvent_t* mk = pair_marks(c, marks, slot);
    if (mk) c->ev_pairs[kTimeMajorAvg].push_back({slot, slot + 1});
    int rc = sample_run(c->stream, *p, xyz, nrm, stride, n, candidates, n_cand, last_xyz, last_stride, m,
                        c->sample_mem, mk, sampled_out, n_sampled, bin_weights_out, c->err);
    if (mk && rc == IMLS_OK && p->method != IMLS_SAMPLE_MAJOR_AXIS) c->ev_pairs[kTimeMajorAvg].pop_back();   // no kernel recorded
    if (c->timing) harvest_timing(c);
    return rc;
}

void imls_default_curvature_params(imls_curvature_params* p) {
    // scan_registration.presample_method.curvature of the shipped config.json (read at 1073, 1464)
    if (!p) return;
    p->window_size = 5;
    p->curvature_threshold = 0.02f;
}

int imls_presample_curvature(imls_ctx* c, const imls_curvature_params* p, const float* xyz, size_t stride,
                             const int32_t* ring_sizes, int32_t n_rings, const uint32_t* row_index,
                             const uint8_t* row_flags, size_t n_rows, float* curvature_out, int32_t* candidates_out,
                             size_t* n_cand) {
    if (!c) return IMLS_ERR_ARG;
    if (!p || !ring_sizes || n_rings <= 0 || n_rings > 4096 || stride < 3)
        return fail(c, IMLS_ERR_ARG, "bad curvature params / ring sizes / stride");
    if (p->window_size < 0) return fail(c, IMLS_ERR_ARG, "bad curvature window_size");
    if (n_rows > 0 && (!row_index || !row_flags || !candidates_out || !n_cand))
        return fail(c, IMLS_ERR_ARG, "null row arrays / candidate outputs");
    long long total = 0;
    for (int i = 0; i < n_rings; ++i) total += ring_sizes[i];
    if (total > 0 && !xyz) return fail(c, IMLS_ERR_ARG, "null xyz");
    if (total >= (1ll << 31) || n_rows >= ((size_t)1 << 31)) return fail(c, IMLS_ERR_CAPACITY, "cloud too large");
    if (int rc = check_device(c)) return rc;
    int slot;
    hipEvent_t marks[2];
    hipEvent_t* mk = pair_marks(c, marks, slot);
    int rc = presample_curvature_run(c->stream, *p, xyz, stride, ring_sizes, n_rings, row_index, row_flags, n_rows,
                                     c->curv_mem, mk, curvature_out, candidates_out, n_cand, c->err);
    if (mk && rc == IMLS_OK && total > 0) c->ev_pairs[kTimeCurvature].push_back({slot, slot + 1});   // (an empty cloud records nothing)
    if (c->timing) harvest_timing(c);
    return rc;
}

int imls_sample_three_axis(imls_ctx* c, int32_t points_per_list, const float* xyz, const float* nrm, size_t stride,
                           size_t n, const float* evals, const int32_t* candidates, size_t n_cand, int32_t* sampled_out,
                           size_t* n_sampled, uint64_t* nan_keys) {
    if (!c) return IMLS_ERR_ARG;
    if (points_per_list < 1 || points_per_list > 4096)
        return fail(c, IMLS_ERR_UNSUPPORTED,
                    "three_axis: points_per_list must be in [1, 4096] (points_per_list = " + std::to_string(points_per_list) + ")");
    if (stride < 3 || !n_sampled || (n_cand > 0 && (!xyz || !nrm || !evals || !candidates || !sampled_out)))
        return fail(c, IMLS_ERR_ARG, "three_axis: null array or stride < 3");
    if (n >= (1ull << 31) || n_cand >= (1ull << 31) / 9) return fail(c, IMLS_ERR_CAPACITY, "cloud too large");
    if (int rc = check_device(c)) return rc;
    int slot = -1;
    hipEvent_t marks[2];
    hipEvent_t* mk = n_cand > 0 ? pair_marks(c, marks, slot) : nullptr;
    int rc = three_axis_run(c->stream, points_per_list, xyz, nrm, stride, n, evals, candidates, n_cand, c->ta_mem, mk,
                            sampled_out, n_sampled, nan_keys, c->err);
    if (mk && rc == IMLS_OK) c->ev_pairs[kTimeThreeAxis].push_back({slot, slot + 1});
    if (c->timing) harvest_timing(c);
    return rc;
}

int imls_sample_random(imls_ctx* c, const int32_t* candidates, size_t n_cand, int32_t max_points, uint32_t shuffle_seed,
                       int32_t* sampled_out, size_t* n_sampled) {
    if (!c) return IMLS_ERR_ARG;
    if (max_points < 0 || !n_sampled || (n_cand > 0 && (!candidates || (max_points > 0 && !sampled_out))))
        return fail(c, IMLS_ERR_ARG, "random: null array or max_points < 0");
    if (n_cand >= (1ull << 31)) return fail(c, IMLS_ERR_CAPACITY, "too many candidates");
    sample_random_host(candidates, n_cand, max_points, shuffle_seed, sampled_out, n_sampled);
    return IMLS_OK;
}

// ---------------------------------------------------------------------------------------------
// A raw sweep to the two clouds on the device (sweep.hip)
// ---------------------------------------------------------------------------------------------
void imls_default_sweep_params(imls_sweep_params* p) {
    if (!p) return;
    imls_default_front_params(&p->front);
    imls_default_pca_params(&p->pca);
    imls_default_curvature_params(&p->curvature);
    imls_default_sample_params(&p->normal, IMLS_SAMPLE_NORMAL);
    imls_default_sample_params(&p->major_axis, IMLS_SAMPLE_MAJOR_AXIS);
    p->presample_method = IMLS_PRESAMPLE_GEOMETRIC_FEATURES;
    p->sample_method = IMLS_SWEEP_MAJOR_AXIS;
    p->points_per_list = 200;
    p->max_points = 2000;
    p->shuffle_seed = 0;
    p->rand_seed = 1;
}

}  // extern "C"
namespace {

// SweepMark: an event pair harvested as `kind` (timing level 1 only)
bool sweep_mark(void* owner, int kind, hipEvent_t ev[2]) {
    imls_ctx* c = (imls_ctx*)owner;
    if (c->timing != 1) return false;
    const int slot = ev_pair(c);
    if (slot < 0) return false;
    ev[0] = c->ev[slot];
    ev[1] = c->ev[slot + 1];
    c->ev_pairs[kind].push_back({slot, slot + 1});
    return true;
}
SweepEnv sweep_env(imls_ctx* c) { return SweepEnv{c->stream, &c->front_mem, &c->pca_mem, sweep_mark, c, &c->err}; }

int sweep_process(imls_ctx* c, const imls_sweep_params* p, const float* h_xyz, const float* d_xyz, size_t stride, size_t n,
                  imls_sweep_info* info) {
    if (!c) return IMLS_ERR_ARG;
    if (!p || (n > 0 && ((!h_xyz && !d_xyz) || stride < 3))) return fail(c, IMLS_ERR_ARG, "sweep: null params / sweep or stride < 3");
    if (p->presample_method < 0 || p->presample_method > 1 || p->sample_method < 0 || p->sample_method > 3)
        return fail(c, IMLS_ERR_ARG, "sweep: unknown presample / sample method");
    if (p->pca.window_size < 0 || p->pca.iter_step <= 0 || p->pca.neighbor_scan < 0 || p->pca.neighbor_scan > 1)
        return fail(c, IMLS_ERR_ARG, "bad pca window_size / iter_step / neighbor_scan");
    if (p->presample_method == IMLS_PRESAMPLE_CURVATURE && p->curvature.window_size < 0)
        return fail(c, IMLS_ERR_ARG, "bad curvature window_size");
    if (p->sample_method == IMLS_SWEEP_THREE_AXIS && (p->points_per_list < 1 || p->points_per_list > 4096))
        return fail(c, IMLS_ERR_UNSUPPORTED, "three_axis: points_per_list must be in [1, 4096]");
    if (p->sample_method == IMLS_SWEEP_RANDOM && p->max_points < 0) return fail(c, IMLS_ERR_ARG, "random: max_points < 0");
    if (c->sweep.deskew_on && !(std::isfinite(p->front.scan_period) && p->front.scan_period > 0.f))
        return fail(c, IMLS_ERR_ARG, "sweep: a motion is set and front.scan_period is not positive");
    if (int rc = check_device(c)) return rc;
    SweepEnv e = sweep_env(c);
    const int rc = sweep_run(e, c->sweep, *p, h_xyz, d_xyz, stride, n, info);
    if (c->timing) {
        if (rc != IMLS_OK) (void)hipStreamSynchronize(c->stream);
        harvest_timing(c);
    }
    return rc;
}

}  // namespace
extern "C" {

int imls_sweep_process(imls_ctx* c, const imls_sweep_params* p, const float* xyz, size_t stride_floats, size_t n,
                       imls_sweep_info* info) {
    return sweep_process(c, p, xyz, nullptr, stride_floats, n, info);
}

int imls_sweep_process_device(imls_ctx* c, const imls_sweep_params* p, const float* d_xyz, size_t stride_floats, size_t n,
                              imls_sweep_info* info) {
    return sweep_process(c, p, nullptr, d_xyz, stride_floats, n, info);
}

int imls_sweep_reset(imls_ctx* c) {
    if (!c) return IMLS_ERR_ARG;
    c->sweep.counter = 1;
    c->sweep.has = false;
    c->sweep.cur = 0;
    c->sweep.deskew_on = false;
    for (auto& S : c->sweep.set) S.n_filtered = S.n_flat = S.cap_filtered = 0;
    return IMLS_OK;
}

// ---------------------------------------------------------------------------------------------
// Deskew (deskew.hip): TransformToStart / TransformToEnd from relTime
// ---------------------------------------------------------------------------------------------
int imls_sweep_set_motion(imls_ctx* c, const double motion[16], int32_t to_frame) {
    if (!c) return IMLS_ERR_ARG;
    if (!motion) {
        c->sweep.deskew_on = false;
        return IMLS_OK;
    }
    DeskewArg A;
    bool identity = false;
    if (int rc = deskew_prepare(motion, to_frame, &A, &identity, c->err)) return rc;
    c->sweep.deskew_on = !identity;
    c->sweep.deskew = A;
    return IMLS_OK;
}

int imls_deskew_device(imls_ctx* c, const double motion[16], int32_t to_frame, float scan_period, float* d_xyzi4, size_t n,
                       float* d_normals4) {
    if (!c) return IMLS_ERR_ARG;
    if (!motion || (n > 0 && !d_xyzi4)) return fail(c, IMLS_ERR_ARG, "deskew: null motion / records");
    if (!(std::isfinite(scan_period) && scan_period > 0.f)) return fail(c, IMLS_ERR_ARG, "deskew: scan_period must be positive");
    if (n > (size_t)0x3fffffff) return fail(c, IMLS_ERR_CAPACITY, "cloud too large");
    DeskewArg A;
    bool identity = false;
    if (int rc = deskew_prepare(motion, to_frame, &A, &identity, c->err)) return rc;
    if (identity || n == 0) return IMLS_OK;
    if (int rc = check_device(c)) return rc;
    int slot;
    timed_begin(c, kTimeDeskew, slot);
    deskew_enqueue(c->stream, A, scan_period, (float4*)d_xyzi4, (float4*)d_normals4, n);
    const bool ok = hipGetLastError() == hipSuccess;
    timed_end(c, kTimeDeskew, slot);
    return ok ? IMLS_OK : fail(c, IMLS_ERR_DEVICE, "deskew launch failed");
}

int imls_deskew(imls_ctx* c, const double motion[16], int32_t to_frame, float scan_period, float* xyzi, size_t stride_floats,
                size_t n, float* normals, size_t normal_stride_floats) {
    if (!c) return IMLS_ERR_ARG;
    if (!motion || (n > 0 && (!xyzi || stride_floats < 4 || (normals && normal_stride_floats < 3))))
        return fail(c, IMLS_ERR_ARG, "deskew: null motion / records, or stride below 4 (points) / 3 (normals)");
    if (!(std::isfinite(scan_period) && scan_period > 0.f)) return fail(c, IMLS_ERR_ARG, "deskew: scan_period must be positive");
    if (n > (size_t)0x3fffffff) return fail(c, IMLS_ERR_CAPACITY, "cloud too large");
    DeskewArg A;
    bool identity = false;
    if (int rc = deskew_prepare(motion, to_frame, &A, &identity, c->err)) return rc;
    if (identity || n == 0) return IMLS_OK;
    if (int rc = check_device(c)) return rc;
    int slot;
    hipEvent_t marks[2];
    hipEvent_t* mk = pair_marks(c, marks, slot);
    const int rc = deskew_host(c->stream, A, scan_period, xyzi, stride_floats, n, normals, normal_stride_floats, c->deskew_mem,
                               mk, c->err);
    if (mk && rc == IMLS_OK) c->ev_pairs[kTimeDeskew].push_back({slot, slot + 1});
    if (c->timing) harvest_timing(c);
    return rc;
}

int imls_sweep_clouds_device(imls_ctx* c, const float** d_filtered_soa6, size_t* n_filtered, const float** d_flat_soa6,
                             size_t* n_flat, const float** d_intensity, const float** d_curvature) {
    if (!c) return IMLS_ERR_ARG;
    if (!c->sweep.has) return fail(c, IMLS_ERR_STATE, "no sweep processed yet");
    const SweepSet& S = c->sweep.set[c->sweep.cur];
    const float* side = S.n_filtered ? (const float*)S.side.p : nullptr;
    if (d_filtered_soa6) *d_filtered_soa6 = S.n_filtered ? (const float*)S.soa6.p : nullptr;
    if (n_filtered) *n_filtered = S.n_filtered;
    if (d_flat_soa6) *d_flat_soa6 = S.n_flat ? (const float*)S.flat.p : nullptr;
    if (n_flat) *n_flat = S.n_flat;
    if (d_intensity) *d_intensity = side;
    if (d_curvature) *d_curvature = side ? side + S.cap_filtered : nullptr;
    return IMLS_OK;
}

int imls_sweep_download(imls_ctx* c, int32_t which, void* records, size_t cap, size_t* n, int32_t* sampled_index) {
    if (!c) return IMLS_ERR_ARG;
    if (which < 0 || which > 1) return fail(c, IMLS_ERR_ARG, "sweep_download: which must be 0 or 1");
    if (!c->sweep.has) return fail(c, IMLS_ERR_STATE, "no sweep processed yet");
    if (int rc = check_device(c)) return rc;
    SweepEnv e = sweep_env(c);
    return sweep_download(e, c->sweep, which, records, cap, n, sampled_index);
}

int imls_sample_point_cloud_device(imls_ctx* c, const imls_sample_params* p, const float* d_soa6, size_t n,
                                   const int32_t* d_candidates, size_t n_cand, const float* d_last_soa6, size_t m,
                                   int32_t* d_sampled_out, size_t* n_sampled, float* d_bin_weights_out,
                                   uint64_t* nan_normals) {
    if (!c) return IMLS_ERR_ARG;
    if (!p || (n_cand > 0 && (!d_soa6 || !d_candidates || !d_sampled_out)))
        return fail(c, IMLS_ERR_ARG, "bad sample params / pointers");
    if (p->method == IMLS_SAMPLE_MAJOR_AXIS && m > 0 && !d_last_soa6) return fail(c, IMLS_ERR_ARG, "major_axis needs last_pcl_cloud");
    if (n >= (1ull << 31) || m >= (1ull << 31) || n_cand >= (1ull << 30)) return fail(c, IMLS_ERR_CAPACITY, "cloud too large");
    if (int rc = check_device(c)) return rc;
    SweepEnv e = sweep_env(c);
    const int rc = sampler_run(e, c->sweep, *p, d_soa6, n, d_candidates, n_cand, d_last_soa6, m, d_sampled_out, n_sampled,
                               d_bin_weights_out, nan_normals);
    if (c->timing) {
        if (rc != IMLS_OK) (void)hipStreamSynchronize(c->stream);
        harvest_timing(c);
    }
    return rc;
}

void imls_shuffle_positions(uint32_t seed, int32_t size, int32_t k, int32_t* out, size_t* n_out) {
    std::vector<int> v;
    shuffle_positions(seed, size, k, v);
    if (out) std::copy(v.begin(), v.end(), out);
    if (n_out) *n_out = v.size();
}

// ---------------------------------------------------------------------------------------------
// Nearest-neighbour queries on the current index (Nabo::NNSearchD::knn, epsilon 0, SORT_RESULTS)
// ---------------------------------------------------------------------------------------------
}  // extern "C"
namespace {

// argument and state checks shared by both forms; completes a pending target build
int knn_check(imls_ctx* c, size_t nq, int32_t k, double max_radius, uint32_t flags) {
    if (k < 1 || k > 32) return fail(c, IMLS_ERR_UNSUPPORTED, "knn: k must be in [1, 32] (k = " + std::to_string(k) + ")");
    if (!(max_radius > 0.0)) return fail(c, IMLS_ERR_ARG, "knn: max_radius must be > 0 (+inf: unbounded)");
    if (flags & ~(uint32_t)IMLS_KNN_ALLOW_SELF_MATCH) return fail(c, IMLS_ERR_ARG, "knn: unknown flag bits");
    if (nq >= ((size_t)1 << 31)) return fail(c, IMLS_ERR_ARG, "knn: nq must be < 2^31");
    if (c->pending || c->batch_member) return fail(c, IMLS_ERR_STATE, "collect the frame first (imls_register_frame_result)");
    if (int rc = finish_target(c)) return rc;
    if (!c->has_target) return fail(c, IMLS_ERR_STATE, "knn: set_target or map_push first");
    return IMLS_OK;
}

// One chunk of n ≤ kKnnChunk queries (component d of query i at d_src[i·pstride + d·cstride], device)
// → device rows; everything is enqueued on the context stream, nothing waits.
int knn_chunk(imls_ctx* c, const float* d_src, size_t pstride, size_t cstride, int n, int32_t k, double max_radius,
              uint32_t flags, int32_t* d_idx, double* d_d2, int32_t* d_found) {
    const size_t nreg = ((size_t)n + 63) / 64, fb_off = (nreg + 63) / 64 * 64;
    if (!grow(c->knn_q, (size_t)n * 16) || !grow(c->knn_lists, knn_list_bytes(n)) ||
        !grow(c->knn_fb, (fb_off + nreg * 64) * 4) || !grow(c->knn_pose, 256))
        return fail(c, IMLS_ERR_DEVICE, "hipMalloc (knn)");
    const TreeView t = tree_view(c);
    knn_prepare(c->stream, t, d_src, pstride, cstride, n, (float4*)c->knn_q.p, (double*)c->knn_pose.p);
    if (int rc = query_order(c->stream, (const float4*)c->knn_q.p, n, t.qparams, c->knn_scratch, c->knn_perm, c->err)) return rc;
    KnnArgs a{};
    a.K = k;
    a.r2 = max_radius * max_radius;
    a.allow_self = (flags & IMLS_KNN_ALLOW_SELF_MATCH) ? 1 : 0;
    a.qwave = c->kp.qwave;
    a.force_fb = c->kp.force_fb;
    int slot;
    timed_begin(c, kTimeKnnQuery, slot);
    launch_knn(c->stream, t, (const float4*)c->knn_q.p, (const unsigned*)c->knn_perm.p, n, (const double*)c->knn_pose.p, a,
               c->lane_mode, (int*)c->knn_lists.p, (unsigned*)c->knn_fb.p + fb_off, (unsigned*)c->knn_fb.p, d_idx, d_d2,
               d_found);
    timed_end(c, kTimeKnnQuery, slot);
    if (hipGetLastError() != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "knn launch failed");
    return IMLS_OK;
}

}  // namespace
extern "C" {

int imls_knn(imls_ctx* c, const float* q_xyz, size_t stride_floats, size_t nq, int32_t k, double max_radius, uint32_t flags,
             int32_t* idx_out, double* d2_out, int32_t* found_out) {
    if (!c) return IMLS_ERR_ARG;
    if (int rc = check_device(c)) return rc;
    if (int rc = knn_check(c, nq, k, max_radius, flags)) return rc;
    if (nq == 0) return IMLS_OK;
    if (!q_xyz || !idx_out || !d2_out || stride_floats < 3) return fail(c, IMLS_ERR_ARG, "knn: null array or stride < 3");
    std::vector<float> pack;
    for (size_t c0 = 0; c0 < nq; c0 += kKnnChunk) {
        const int n = (int)std::min(nq - c0, (size_t)kKnnChunk);
        const float* src = q_xyz + c0 * stride_floats;
        if (stride_floats != 3) {
            pack.resize((size_t)n * 3);
            for (int i = 0; i < n; ++i)
                for (int d = 0; d < 3; ++d) pack[(size_t)i * 3 + d] = src[(size_t)i * stride_floats + d];
            src = pack.data();
        }
        const size_t bi = ((size_t)n * k * 4 + 255) / 256 * 256, bd = ((size_t)n * k * 8 + 255) / 256 * 256;
        if (!grow(c->knn_up, (size_t)n * 12) || !grow(c->knn_out, bi + bd + (size_t)n * 4))
            return fail(c, IMLS_ERR_DEVICE, "hipMalloc (knn staging)");
        int32_t* d_idx = (int32_t*)c->knn_out.p;
        double* d_d2 = (double*)((char*)c->knn_out.p + bi);
        int32_t* d_found = (int32_t*)((char*)c->knn_out.p + bi + bd);
        if (hipMemcpyAsync(c->knn_up.p, src, (size_t)n * 12, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return fail(c, IMLS_ERR_DEVICE, "knn: query upload failed");
        if (int rc = knn_chunk(c, (const float*)c->knn_up.p, 3, 1, n, k, max_radius, flags, d_idx, d_d2, d_found)) return rc;
        hipMemcpyAsync(idx_out + c0 * k, d_idx, (size_t)n * k * 4, hipMemcpyDeviceToHost, c->stream);
        hipMemcpyAsync(d2_out + c0 * k, d_d2, (size_t)n * k * 8, hipMemcpyDeviceToHost, c->stream);
        if (found_out) hipMemcpyAsync(found_out + c0, d_found, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream);
        // (per chunk: the staging buffers and `pack` are reused by the next one)
        if (hipStreamSynchronize(c->stream) != hipSuccess)
            return fail(c, IMLS_ERR_DEVICE, std::string("knn: ") + hipGetErrorString(hipGetLastError()));
    }
    harvest_timing(c);
    return IMLS_OK;
}

int imls_knn_device(imls_ctx* c, const float* d_q3, size_t nq, int32_t k, double max_radius, uint32_t flags,
                    int32_t* d_idx_out, double* d_d2_out, int32_t* d_found_out) {
    if (!c) return IMLS_ERR_ARG;
    if (int rc = check_device(c)) return rc;
    if (int rc = knn_check(c, nq, k, max_radius, flags)) return rc;
    if (nq == 0) return IMLS_OK;
    if (!d_q3 || !d_idx_out || !d_d2_out) return fail(c, IMLS_ERR_ARG, "knn: null array");
    for (size_t c0 = 0; c0 < nq; c0 += kKnnChunk) {
        const int n = (int)std::min(nq - c0, (size_t)kKnnChunk);
        if (int rc = knn_chunk(c, d_q3 + c0, 1, nq, n, k, max_radius, flags, d_idx_out + c0 * k, d_d2_out + c0 * k,
                               d_found_out ? d_found_out + c0 : nullptr))
            return rc;
    }
    return IMLS_OK;
}

}  // extern "C"
