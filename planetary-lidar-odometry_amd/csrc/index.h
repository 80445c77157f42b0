// index.h — the spatial index family as its callers see it: the NaN filter and pose kernels
// (filter.hip), the lone and batched Morton builds (index.hip), the incremental FIFO index
// (fifo_index.hip).
#pragma once
#include <utility>

#include "internal.h"

namespace imlsgpu {

// filter.hip, index.hip — two phases, so many frames' uploads and filters can be enqueued before one wait:
// (A) filter_async: NaN filter + order-keeping compaction (kept: filtered → input index, nullable),
//     the kept count written to pinned *h_count by the compaction itself;
// (B) with that count known: build_target_tree (Morton sort, leaf boxes, node records) or
//     source_order (the source's Morton order = the wave kernels' query order).
// `pose` (nullable): the posed map push — a kept point leaves the scatter pass as float(pose·[p;1])
// and its normal rotated, in transform_query's arithmetic (geom.h); the filter tests the point as given.
int filter_async(hipStream_t s, const float* d_soa6, size_t n_in, DevBuf& pt, DevBuf& nr, DevBuf& scratch,
                 unsigned* d_kept, int* h_count, std::string& err, const Pose12* pose = nullptr);
// The same arithmetic elementwise: an SoA6 scan [6][n] into `out` (may be `in`; a point with a
// non-finite coordinate is copied as given), and filtered float4 records in place (w kept).
int pose_soa6(hipStream_t s, const float* in, float* out, size_t n, const Pose12& pose, std::string& err);
int pose_records(hipStream_t s, float4* pt, float4* nr, size_t n, const Pose12& pose, std::string& err);
// (A) for many frames at once (deferred filters of a batch's members), one launch sequence; the
// kept counts land in each job's pinned host word once the stream has passed it.
struct FilterJob {
    const float* soa;
    size_t n;
    DevBuf *pt, *nr;                   // grown to n records here
    unsigned* kept;                    // nullable
    int* h_count;
};
int filter_batch(hipStream_t s, const std::vector<FilterJob>& jobs, DevBuf& scratch, DevBuf& table, void* h_table,
                 size_t h_table_bytes, std::string& err);
size_t filter_job_bytes();
int build_target_tree(hipStream_t s, int M, int bucket, DevBuf& lkeys, DevBuf& tpt, DevBuf& tnr, DevBuf& mpt,
                      DevBuf& nodes, DevBuf& scratch, DevBuf& treescratch, DevBuf& permbuf, int* P_out, int* levels_out,
                      std::string& err);
int source_order(hipStream_t s, int N, DevBuf& spt, DevBuf& scratch, DevBuf& qperm, std::string& err);
// the kNN queries' order (imls_knn): Morton keys under the target's quantisation qp (device, [4])
int query_order(hipStream_t s, const float4* pts, int n, const float* qp, DevBuf& scratch, DevBuf& perm, std::string& err);
// a small frame's source order (≤ kSmallOrderN points) in one launch — the same permutation
constexpr int kSmallOrderN = 2048;
int small_source_order(hipStream_t s, const float4* pts, int N, unsigned* perm, std::string& err);
// (B) for many frames at once, one launch sequence: each job a target tree (B > 0: lkeys [L + 2]
// words, mpt [3·n] records, nodes [(P+1)·3] float4, sized by the caller; P / levels returned in the
// job) or a source order (B = 0: perm [n]).  h_table: pinned host memory for the job table.
struct BuildJob {
    const float4* pts;
    const float4* nrm;
    int n, B;
    unsigned long long* lkeys;
    float4* mpt;
    float4* nodes;
    unsigned* perm;
    int P, levels;                     // out (targets)
};
int build_batch(hipStream_t s, std::vector<BuildJob>& jobs, DevBuf& scratch, DevBuf& table, void* h_table,
                size_t h_table_bytes, std::string& err);
size_t build_job_bytes();              // bytes per job of the device job table

// fifo_index.hip — incremental index of the map FIFO (api_map.hip map_push / fifo_build, from api.hip finish_target).  A run = one
// scan's filtered points Morton-sorted under the FIFO's fixed quantisation: [n] sorted keys, [n]
// records (xyz, bits(local filtered index)), [n] normals, 256-B aligned parts of one buffer.
struct FifoRun {
    const float4* rpt;
    const float4* rnr;
    unsigned off;                      // concatenated filtered index of the run's first point
    unsigned pad;
};
constexpr int kMaxFifoRuns = 32;       // run ids (5 bits of a merged entry's value; 27 bits of position)
struct FifoRunTable { FifoRun r[kMaxFifoRuns]; };   // by value in the gather launch (768 B of arguments)
inline size_t fifo_part(size_t bytes) { return (bytes + 255) / 256 * 256; }
inline size_t fifo_run_bytes(int n) { return fifo_part((size_t)n * 8) + 2 * fifo_part((size_t)n * 16); }
inline unsigned long long* fifo_run_keys(void* run, int) { return (unsigned long long*)run; }
inline float4* fifo_run_pts(void* run, int n) { return (float4*)((char*)run + fifo_part((size_t)n * 8)); }
inline float4* fifo_run_nrm(void* run, int n) { return (float4*)((char*)run + fifo_part((size_t)n * 8) + fifo_part((size_t)n * 16)); }
// scratch every fifo_* step of one build fits in (sized before the build enqueues anything: the
// steps share it in stream order and never reallocate it under a pending kernel)
size_t fifo_scratch_bytes(int max_run, int nruns, int M);
// the FIFO's quantisation frame (fq: lo xyz, scale) from the bboxes of filtered point sets
int fifo_frame(hipStream_t s, const std::vector<std::pair<const float4*, int>>& runs, float* fq, DevBuf& scratch,
               std::string& err);
// one run from n filtered points (clamp: device counter of points outside fq's cube)
int fifo_run_build(hipStream_t s, const float4* fpt, const float4* fnr, int n, const float* fq, unsigned* clamp,
                   DevBuf& run, DevBuf& scratch, std::string& err);
// stable compaction of a merged order to the entries of live runs (bit id of `live`)
int fifo_keep(hipStream_t s, const unsigned long long* key, const unsigned* val, int n, unsigned live,
              unsigned long long* okey, unsigned* oval, DevBuf& scratch, std::string& err);
// merge(A, run B) by key, A first on equal keys; B's values become (bid << 27) | index
int fifo_merge(hipStream_t s, const unsigned long long* a, const unsigned* av, int na, const unsigned long long* b,
               unsigned bid, int nb, unsigned long long* okey, unsigned* oval, std::string& err);
// the target index from the merged order (records, ipos, leaf keys + fq, leaf boxes, tree)
// (clamp: the device clamp counter, copied to the host's coherent word h_clamp behind the build)
int fifo_index(hipStream_t s, const unsigned long long* mkey, const unsigned* mval, int M, const FifoRunTable& runs,
               const float* fq, const unsigned* clamp, unsigned* h_clamp, int B, DevBuf& lkeys, DevBuf& mpt, DevBuf& nodes,
               DevBuf& treescratch, int* P_out, int* levels_out, std::string& err);

}  // namespace imlsgpu
