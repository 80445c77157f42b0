// context.h — what the api*.hip units share: the context behind include/imls_gpu.h's opaque imls_ctx,
// its runtime options, and the helpers that more than one unit
// calls.  Not installed; nothing outside csrc/api*.hip includes it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <deque>
#include <string>
#include <utility>
#include <vector>

#include "internal.h"

using imlsgpu::DevBuf;
using imlsgpu::KParams;
using imlsgpu::PairDev;
using imlsgpu::SolveState;
using imlsgpu::SweepState;

// Runtime options of a context (imls_set_option; include/imls_gpu.h documents each): the validated
// tuning parameters and test hooks.  Nothing is read from the environment.
struct Options {
    int traversal = IMLS_TRAVERSAL_AUTO;
    int list_reuse = 1;
    int temporal_seed = 1;
    int leaf_size = 64;
    int first_packet = 32;
    int first_packet_iters = 1;
    int first_packet_batched = 0;
    double tv_skin = 0.03;
    int force_fallback = 0;
};

inline bool same_options(const Options& a, const Options& b) {
    return a.traversal == b.traversal && a.list_reuse == b.list_reuse && a.temporal_seed == b.temporal_seed &&
           a.leaf_size == b.leaf_size && a.first_packet == b.first_packet && a.first_packet_iters == b.first_packet_iters &&
           a.first_packet_batched == b.first_packet_batched && a.tv_skin == b.tv_skin && a.force_fallback == b.force_fallback;
}

struct imls_ctx {
    int device = 0;
    hipStream_t own = nullptr, stream = nullptr;
    imls_params P{};
    KParams kp{};
    std::string err;
    int B = 64;
    // target
    DevBuf tpt, tnr, mpt, nodes, tscratch, treescratch, permbuf, upload_t;
    int M = 0, Pl = 0, levels = 0;
    bool has_target = false;
    // source
    DevBuf spt, snr, sscratch, qperm, upload_s, skept;
    // map FIFO (accumulateTargetCloud, laser_odometry.cpp:116-136): the last max_queue_size filtered
    // scans, each SoA6 in its own slot, and their concatenation (oldest first) the index is built from
    // a FIFO entry: its raw SoA6 scan (the concatenation path), and for the incremental index its
    // filtered points (fpt / fnr, NaN filter at the push) and its sorted run (fifo_index.hip)
    struct MapSlot {
        DevBuf buf, fpt, fnr, run;
        size_t n = 0;
        bool ghost = false;
        int id = -1;                      // run id (incremental index)
        int nk = -1;                      // kept count after the NaN filter (−1: not read yet)
        bool sorted = false;              // run built under the current quantisation frame
    };
    std::deque<MapSlot> fifo;
    std::vector<MapSlot> slot_pool;       // freed slots, their buffers reused (no allocation per frame)
    // incremental FIFO index (max_queue_size 2..kMaxFifoRuns−1): each scan sorted once at its first
    // build under a quantisation frame fixed for the FIFO, the previous merged order kept across
    // registrations (finish_target → fifo_build)
    bool fifo_inc = false;                // the current / pending target is the FIFO's incremental index
    unsigned fifo_seq = 0;                // run ids: pushes mod kMaxFifoRuns
    int* h_fifo_cnt = nullptr;            // pinned [kMaxFifoRuns]: kept count of each run's filter
    unsigned* h_fifo_clamp = nullptr;     // pinned: points outside the frame at the last build
    DevBuf fifo_dev;                      // fq[4] | clamp counter
    bool fq_valid = false;
    // imls_set_initial_pose: rPose at the start of every later registration (identity by default)
    double init_pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::vector<int> merged_ids;          // runs in the merged order, oldest first
    DevBuf mkey[2], mval[2];
    int mcur = 0, m_n = 0;
    DevBuf fscr;                          // FIFO build scratch
    hipEvent_t ev_fifo = nullptr;         // after the last incremental build (batch joins)
    DevBuf macc;
    size_t map_points = 0;                // Σ n over the FIFO (before the NaN filter)
    // voxel map (imls_voxel_map_update, voxel_map.hip): the map as SoA6 [6][n] in buf[cur], the other
    // buffer the next update's output; the scan's map-frame copy; the update's scratch; the pinned
    // record the one wait of an update reads.  A context holds this map or the FIFO, never both.
    struct VoxelMap {
        DevBuf buf[2], scan, scratch;
        int cur = 0;
        size_t n = 0;
        imls_voxel_map_params P{0.5f, 20, 100.0f};
        imls_voxel_map_info info{};
        unsigned* h_rec = nullptr;
        hipEvent_t ev = nullptr;
    } vox;
    DevBuf fb;                            // deferred-query counts per k_finish block + their lists
    size_t fb_off = 64;                   // words: start of the lists in fb
    DevBuf lkeys;                         // leaf first Morton keys + quantisation (seed search)
    DevBuf rnr;                           // recomputed map normals (count mode), Morton order
    bool rnr_valid = false;
    int rnr_k = -1;
    double rnr_r = -1.0;
    DevBuf prevnn;                        // per-query neighbour lists carried between ICP iterations
    DevBuf tkept;                         // target: filtered index → input index (tensor upload)
    DevBuf mten, upload_ten;              // tensor voting: input tensors (Morton order) + upload staging
    DevBuf tvn;                           // tensor voting: per-source voted normal + found flag (double4)
    DevBuf pca_mem;                       // imls_ring_normals_pca scratch (upstream producer)
    DevBuf sample_mem;                    // imls_sample_point_cloud scratch
    DevBuf front_mem;                     // imls_scan_front_end scratch
    DevBuf curv_mem;                      // imls_presample_curvature scratch
    DevBuf ta_mem;                        // imls_sample_three_axis scratch
    DevBuf deskew_mem;                    // imls_deskew staging (records | normals)
    SweepState sweep;                     // imls_sweep_process: the rotating cloud sets, counter, scratch
    // imls_knn / imls_knn_device: buffers of their own (one chunk of ≤ kKnnChunk queries), so a query
    // leaves the loaded source, its order, the correspondences and the neighbour lists alone —
    // queries (xyz, non-finite flag), their Morton order + the sort's scratch, the list block,
    // the deferred-query counts + lists, the identity pose, and the host form's staging (upload, rows)
    DevBuf knn_q, knn_perm, knn_scratch, knn_lists, knn_fb, knn_pose, knn_up, knn_out;
    size_t n_target_in = 0;               // input size of the last set_target (tensor arrays match it)
    bool has_tensors = false;
    Options opt;                          // imls_set_option
    int lane_mode = 0;                    // opt.traversal == IMLS_TRAVERSAL_LANE
    int temporal_seed = 1;                // opt.temporal_seed
    int N = 0;
    bool has_source = false;
    // deferred index builds: set_target / map_push / set_source without a requested count only
    // enqueue the upload and the NaN filter; the rest of the build (which needs the kept count on
    // the host) runs at the first use (ensure_built), so many frames' filters overlap one wait
    int* h_cnt = nullptr;                 // pinned [4]: kept counts of the pending target / source
    hipEvent_t ev_tgt = nullptr, ev_src = nullptr;
    bool tgt_pending = false, src_pending = false;
    // deferred filters (no count requested): the NaN filter itself waits for the first use, reading
    // its input (an owned upload / FIFO buffer, or the caller's device scan) then — a batch runs all
    // its members' filters in one launch sequence (filter_batch)
    const float* tf_soa = nullptr;
    const float* sf_soa = nullptr;
    size_t tf_n = 0, sf_n = 0;
    bool tgt_filter_deferred = false, src_filter_deferred = false;
    bool defer = false;                   // imls_set_defer: count-less loads read their input at first use
    const float* ten_src = nullptr;       // tensors set while the target build was pending
    size_t ten_n = 0;
    bool ten_pending = false;
    int tgt_slot = -1;                    // timing event slot of the pending target build
    uint32_t* src_kept_out = nullptr;
    // pinned staging of host uploads (0: target / map scans, 1: source), reused once its copy ran
    float* h_stage[2] = {nullptr, nullptr};
    size_t stage_cap[2] = {0, 0};
    hipEvent_t ev_stage[2] = {nullptr, nullptr};
    // an upload of that kind whose NaN filter has not been consumed by a build yet (it may still be
    // reading its device buffer): the next upload's copy is then ordered behind it
    bool stage_pending[2] = {false, false};
    hipStream_t ustream = nullptr;        // host → device copies of uploads (upload_soa6)
    // correspondences + solver state
    DevBuf cs, cd, cn, solve_mem, trace_mem, stats, rows_d, pose_tmp;
    DevBuf ransac_mem, rng;               // RANSAC scratch + the glibc rand() state (34 words)
    int rng_seed_state[34] = {};          // host copy of the seeded state
    bool rng_dirty = true;                // upload rng_seed_state to the device before its next use
    int* h_rng = nullptr;                 // pinned source of that upload (rewritten after ev_rng)
    hipEvent_t ev_rng = nullptr;
    bool rng_init = false;                // seeded from params.ransac_seed (first imls_set_params)
    SolveState st{};
    int st_N = -1, trace_cap = 0;
    bool has_corr = false;
    // per-iteration correspondences of imls_register_frame (imls_capture_correspondences): slot it =
    // cs / cd / cn (float4 [N] each) after iteration it's projection
    bool capture = false;
    DevBuf cap_mem;
    int cap_iters = 0, cap_N = 0;
    int cap_run = -1;                     // iterations the captured frame ran (-1: result not collected yet)
    // pose covariance / degeneracy report (imls_capture_pose_info): info_mem = the solves' export block,
    // the report and the row pass's slabs; h_info = the pinned copy the result call reads
    bool info_capture = false;
    DevBuf info_mem;
    struct imls_pose_info* h_info = nullptr;
    int info_state = 0;                   // 0: none (capture was off), 1: enqueued, result not collected, 2: ready
    // async frame results
    imls_iter_trace* h_trace = nullptr;   // pinned
    double* h_misc = nullptr;             // pinned: pose[16], iters, status
    int pending_iters = 0;
    bool pending = false;
    // batched registration led by this context (imls_register_frames*): frame table, results
    PairDev* tab_h = nullptr;             // pinned [tab_cap]
    DevBuf tab_d, res_d;
    double* res_h = nullptr;              // pinned: [n][kResStride] results, then [n][iters] traces
    size_t res_h_bytes = 0;
    int tab_cap = 0;
    std::vector<imls_ctx*> members;       // frames of the pending batch (members[0] == this)
    std::vector<int> member_n;
    bool batch_pending = false, batch_fused = false, batch_traces = false;
    bool batch_member = false;            // part of a pending batch (as lead or member)
    hipEvent_t ev_batch = nullptr;
    // batched index builds of a batch's members (build_batch): scratch, job table, pinned staging
    DevBuf bscratch, btable;
    void* h_btable = nullptr;
    size_t h_btable_bytes = 0;
    DevBuf fscratch, ftable;              // batched filters (filter_batch)
    void* h_ftable = nullptr;
    size_t h_ftable_bytes = 0;
    hipEvent_t ev_build = nullptr;
    // traversal / neighbour counters (imls_traversal_stats): off by default — their per-wave
    // device-scope atomics onto a few shared words cost ~60 µs per projection at config B
    bool collect_stats = false;
    // timing: 0 off, 1 every launch kind (a batch's members then build one by one, each inside its
    // own events), 2 light — the projection / solve events of the iterations only (builds unchanged),
    // kept as intervals on a process-wide clock (imls_timing_intervals: busy time of concurrent work)
    int timing = 0;
    std::vector<std::pair<double, double>> iv[imlsgpu::kTimingKinds];
    std::vector<hipEvent_t> ev;
    int ev_used = 0;
    std::vector<std::pair<int, int>> ev_pairs[imlsgpu::kTimingKinds];
    double t_ms[imlsgpu::kTimingKinds] = {};
    uint64_t t_n[imlsgpu::kTimingKinds] = {};
};

// Helpers that more than one api*.hip unit calls (each commented at its definition).  Hidden: they are
// internal to the library and stay out of its dynamic symbol table.
namespace imlsgpu {
struct RansacParams;   // solve.h
#pragma GCC visibility push(hidden)
// api.hip
int fail(imls_ctx* c, int code, const std::string& m);
bool grow(DevBuf& b, size_t bytes);
bool grow_keep(DevBuf& b, size_t bytes, size_t keep, hipStream_t s);
int check_device(imls_ctx* c);
int info_begin(imls_ctx* c, int rows, hipStream_t s);
int info_enqueue(imls_ctx* c, imls_ctx* timer, hipStream_t s, int method, const double* rows_d, const double* weights, int N,
                 int in_loop);
int check_tv_ready(imls_ctx* c);
int ensure_solve(imls_ctx* c, int N);
int ensure_trace(imls_ctx* c, int iters);
RansacParams ransac_params(const imls_params& p);
int prepare_ransac(imls_ctx* c, int rows);
TreeView tree_view(imls_ctx* c);
int finish_target(imls_ctx* c);
int ensure_built(imls_ctx* c);
int do_set_target(imls_ctx* c, const float* d_soa6, size_t n, size_t* n_kept);
int gather_tensors(imls_ctx* c, hipStream_t s, const float* d_ten6, size_t n);
unsigned* fb_count(imls_ctx* c);
unsigned long long* stats_ptr(imls_ctx* c);
unsigned* fb_list(imls_ctx* c);
// api_map.hip
int fifo_build(imls_ctx* c);
// api_support.hip
int ev_pair(imls_ctx* c);
void timed_begin(imls_ctx* c, int kind, int& slot);
void timed_end(imls_ctx* c, int kind, int slot);
hipEvent_t* project_marks(imls_ctx* c, hipEvent_t marks[3]);
hipEvent_t* pair_marks(imls_ctx* c, hipEvent_t marks[2], int& slot);
void harvest_timing(imls_ctx* c);
int upload_soa6(imls_ctx* c, DevBuf& dst, const float* xyz, const float* nrm, size_t n, size_t stride, int which);
#pragma GCC visibility pop
}  // namespace imlsgpu
