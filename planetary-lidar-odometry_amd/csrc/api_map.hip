// api_map.hip — the map FIFO of the C ABI (imls_map_push* … imls_map_size, imls_set_initial_pose,
// imls_map_rebase) and its incremental index build (fifo_build, reached from api.hip finish_target).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "context.h"
#include "index.h"

using namespace imlsgpu;

// accumulateTargetCloud (laser_odometry.cpp:116-136) + setTargetPointCloud(accumulatedTargetCloud)
// (imls_icp.cpp:80-103): the new scan goes to a FIFO slot (`from_host`: packed + uploaded, the only
// PCIe traffic; else copied device-to-device), the oldest entry is dropped once when the FIFO holds
// more than max_queue_size (the reference's `if`, not a loop), the entries are concatenated oldest
// first into one SoA6 map in HBM (one 2-D device copy per entry) and the index is rebuilt over it.
// (These helpers sit inside extern "C", as they always have: that puts their five names in the
// library's dynamic symbol table, which is left as it was.)
extern "C" {
namespace {
// ---- incremental FIFO index -----------------------------------------------------------------
// Used for max_queue_size 2 … kMaxFifoRuns − 1 (queue 1 indexes its one scan in place; a run id
// must be unique among the FIFO's entries).
bool fifo_incremental(const imls_ctx* c) { return c->P.max_queue_size >= 2 && c->P.max_queue_size < kMaxFifoRuns; }

int ensure_fifo(imls_ctx* c) {
    if (c->h_fifo_cnt) return IMLS_OK;
    if (hipHostMalloc((void**)&c->h_fifo_cnt, kMaxFifoRuns * sizeof(int), hipHostMallocCoherent) != hipSuccess ||
        // coherent: the FIFO gather kernel writes the clamp count here directly
        hipHostMalloc((void**)&c->h_fifo_clamp, 64, hipHostMallocCoherent) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "hipHostMalloc (FIFO)");
    *c->h_fifo_clamp = 0;
    if (!grow(c->fifo_dev, 256 + kMaxFifoRuns * sizeof(FifoRun))) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (FIFO)");
    if (hipMemsetAsync(c->fifo_dev.p, 0, 256, c->stream) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "hipMemset (FIFO)");
    if (hipEventCreateWithFlags(&c->ev_fifo, hipEventDisableTiming) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "hipEventCreate");
    return IMLS_OK;
}
float* fifo_fq(imls_ctx* c) { return (float*)c->fifo_dev.p; }
unsigned* fifo_clamp(imls_ctx* c) { return (unsigned*)((char*)c->fifo_dev.p + 64); }

// the target is the FIFO's incremental index: pending until its first use (or at once with n_map)
int fifo_set_target(imls_ctx* c, size_t* n_map) {
    c->has_tensors = false;
    c->ten_pending = false;
    c->tgt_filter_deferred = false;
    c->has_corr = false;
    c->rnr_valid = false;
    if (c->map_points == 0) {             // empty map (max_queue_size 0 or empty scans): no target
        c->tgt_pending = false;
        c->has_target = false;
        c->fifo_inc = false;
        c->M = 0;
        if (n_map) *n_map = 0;
        return IMLS_OK;
    }
    if (!c->ev_tgt && hipEventCreateWithFlags(&c->ev_tgt, hipEventDisableTiming) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "hipEventCreate");
    if (c->tgt_slot < 0) timed_begin(c, kTimeIndex, c->tgt_slot);
    if (hipEventRecord(c->ev_tgt, c->stream) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "event record");
    c->n_target_in = c->map_points;
    c->fifo_inc = true;
    c->tgt_pending = true;
    c->has_target = true;                 // provisional: the build decides (an all-NaN map has none)
    if (n_map) {
        if (int rc = finish_target(c)) return rc;
        *n_map = (size_t)c->M;
    }
    return IMLS_OK;
}

}  // namespace
}  // extern "C"

// The build: the kept counts (one wait for every pending filter), the frame (first build, or after
// a scan fell outside it), the runs not sorted yet, the merged order (drop evicted runs, merge the
// new ones after the kept ones: the FIFO is oldest first), the index from it.
int imlsgpu::fifo_build(imls_ctx* c) {
    if (hipEventSynchronize(c->ev_tgt) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "map filter failed");
    c->stage_pending[0] = false;
    hipStream_t s = c->stream;
    size_t M = 0;
    for (auto& e : c->fifo) {
        if (e.nk < 0) e.nk = e.n ? c->h_fifo_cnt[e.id] : 0;
        M += (size_t)e.nk;
    }
    c->M = (int)M;
    c->has_target = M > 0;
    if (M == 0) {
        timed_end(c, kTimeIndex, c->tgt_slot);
        c->tgt_slot = -1;
        return IMLS_OK;
    }
    if (M > (size_t)0x7fffffff) return fail(c, IMLS_ERR_CAPACITY, "map too large");
    {   // the build's scratch, before anything is enqueued (its steps never reallocate it)
        int max_run = 0, nruns = 0;
        for (auto& e : c->fifo) { max_run = std::max(max_run, e.nk); nruns += e.nk > 0; }
        if (!grow(c->fscr, fifo_scratch_bytes(max_run, nruns, (int)M))) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (FIFO scratch)");
    }
    // re-frame when the last build's new scans fell outside the frame (their keys were clamped)
    if (c->fq_valid && *c->h_fifo_clamp != 0) c->fq_valid = false;
    if (!c->fq_valid) {
        // every entry's filtered points stay in its fpt / fnr while it is in the FIFO: re-key them all
        std::vector<std::pair<const float4*, int>> pts;
        for (auto& e : c->fifo)
            if (e.nk > 0) {
                pts.push_back({(const float4*)e.fpt.p, e.nk});
                e.sorted = false;
            }
        if (int rc = fifo_frame(s, pts, fifo_fq(c), c->fscr, c->err)) return rc;
        if (hipMemsetAsync(fifo_clamp(c), 0, 4, s) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "hipMemset (clamp)");
        c->merged_ids.clear();
        c->m_n = 0;
        c->fq_valid = true;
    }
    for (auto& e : c->fifo)
        if (e.nk > 0 && !e.sorted) {
            if (int rc = fifo_run_build(s, (const float4*)e.fpt.p, (const float4*)e.fnr.p, e.nk, fifo_fq(c), fifo_clamp(c), e.run,
                                        c->fscr, c->err))
                return rc;
            e.sorted = true;
        }
    // the merged order: its runs must be a prefix of the FIFO's (new runs are the newest) — else restart
    auto merged = [&](int id) { return std::find(c->merged_ids.begin(), c->merged_ids.end(), id) != c->merged_ids.end(); };
    bool seen_new = false, prefix = true;
    unsigned live = 0;
    int kept_n = 0;
    for (auto& e : c->fifo) {
        if (e.nk <= 0) continue;
        if (!merged(e.id)) { seen_new = true; continue; }
        if (seen_new) prefix = false;
        live |= 1u << e.id;
        kept_n += e.nk;
    }
    if (!prefix) { c->merged_ids.clear(); c->m_n = 0; live = 0; kept_n = 0; }
    // the current order's buffers keep their m_n entries when they grow (a plain grow drops them:
    // the merge would read stale run ids); the other pair is output only
    if (!grow_keep(c->mkey[c->mcur], M * 8 + 64, (size_t)c->m_n * 8, s) ||
        !grow_keep(c->mval[c->mcur], M * 4 + 64, (size_t)c->m_n * 4, s) || !grow(c->mkey[c->mcur ^ 1], M * 8 + 64) ||
        !grow(c->mval[c->mcur ^ 1], M * 4 + 64))
        return fail(c, IMLS_ERR_DEVICE, "hipMalloc (FIFO order)");
    auto K = [&](int k) { return (unsigned long long*)c->mkey[k].p; };
    auto V = [&](int k) { return (unsigned*)c->mval[k].p; };
    if (c->m_n > 0 && kept_n != c->m_n) {            // evicted runs: stable compaction
        if (int rc = fifo_keep(s, K(c->mcur), V(c->mcur), c->m_n, live, K(c->mcur ^ 1), V(c->mcur ^ 1), c->fscr, c->err)) return rc;
        c->mcur ^= 1;
    }
    c->m_n = c->m_n > 0 ? kept_n : 0;
    std::vector<int> ids;
    for (auto& e : c->fifo)
        if (e.nk > 0 && (live >> e.id & 1u)) ids.push_back(e.id);
    for (auto& e : c->fifo) {
        if (e.nk <= 0 || (live >> e.id & 1u)) continue;
        if (int rc = fifo_merge(s, K(c->mcur), V(c->mcur), c->m_n, fifo_run_keys(e.run.p, e.nk), (unsigned)e.id, e.nk,
                                K(c->mcur ^ 1), V(c->mcur ^ 1), c->err))
            return rc;
        c->mcur ^= 1;
        c->m_n += e.nk;
        ids.push_back(e.id);
    }
    c->merged_ids = ids;
    // run table (by value in the gather launch): each run's records and its offset in the
    // concatenation (the libnabo tie order)
    FifoRunTable rt{};
    unsigned off = 0;
    for (auto& e : c->fifo) {
        if (e.nk <= 0) continue;
        rt.r[e.id] = FifoRun{fifo_run_pts(e.run.p, e.nk), fifo_run_nrm(e.run.p, e.nk), off, 0u};
        off += (unsigned)e.nk;
    }
    // the gather also copies this build's clamp count into the host's coherent word, read at the next
    // build (after its wait for the map filter, which this stream runs after the gather)
    int rc = fifo_index(s, K(c->mcur), V(c->mcur), c->M, rt, fifo_fq(c), fifo_clamp(c), c->h_fifo_clamp, c->B, c->lkeys,
                        c->mpt, c->nodes, c->treescratch, &c->Pl, &c->levels, c->err);
    if (rc) return rc;
    (void)hipEventRecord(c->ev_fifo, s);
    timed_end(c, kTimeIndex, c->tgt_slot);
    c->tgt_slot = -1;
    return IMLS_OK;
}

extern "C" {

// The concatenation of the FIFO's raw scans (max_queue_size 1 or ≥ kMaxFifoRuns) as the target.
static int map_assemble(imls_ctx* c, size_t* n_map) {
    for (const auto& e : c->fifo)     // a scan indexed in place (max_queue_size was 1) is not held
        if (e.ghost && e.n > 0) return fail(c, IMLS_ERR_STATE, "map FIFO holds a scan pushed with max_queue_size 1 (not kept): push again");
    const size_t M = c->map_points;
    if (M == 0) {                     // empty map (max_queue_size 0 or empty scans): no target
        c->tgt_pending = false;
        c->has_target = false;
        c->has_corr = false;
        c->M = 0;
        if (n_map) *n_map = 0;
        return IMLS_OK;
    }
    for (const auto& e : c->fifo)     // one non-empty entry (max_queue_size 1): index it in place
        if (e.n == M) return do_set_target(c, (const float*)e.buf.p, M, n_map);
    if (!grow(c->macc, M * 24)) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (map)");
    size_t off = 0;
    for (const auto& e : c->fifo) {
        if (e.n == 0) continue;
        if (hipMemcpy2DAsync((float*)c->macc.p + off, M * 4, e.buf.p, e.n * 4, e.n * 4, 6, hipMemcpyDeviceToDevice,
                             c->stream) != hipSuccess)
            return fail(c, IMLS_ERR_DEVICE, "map assembly copy");
        off += e.n;
    }
    return do_set_target(c, (const float*)c->macc.p, M, n_map);
}

// `pose` (nullable = the plain push): map ← scan.  The scan enters the FIFO in the map frame — the
// incremental index transforms it inside its NaN filter's scatter pass (filter_async); the raw-scan
// modes (queue 1, concatenation) write the slot's copy transformed (a device scan: in place of the
// plain device-to-device copy; a host scan: over its upload).  The pose is a launch argument, so it
// is copied at the call.
static int map_push(imls_ctx* c, const float* xyz, const float* nrm, size_t n, size_t stride, const float* d_soa6,
                    size_t* n_map, const Pose12* pose = nullptr) {
    if (n > (size_t)0x7fffffff) return fail(c, IMLS_ERR_ARG, "scan too large");
    if (c->vox.n > 0) return fail(c, IMLS_ERR_STATE, "the context holds a voxel map: imls_map_clear first");
    // max_queue_size 1 with a device scan (the shipped config, device frames): the map IS this
    // scan, dropped at the next push — index it where it lies (its NaN filter reads it on this
    // stream, as the slot copy would), no FIFO copy.  (A posed scan needs its transformed copy.)
    if (d_soa6 && c->P.max_queue_size == 1 && !pose) {
        for (auto& e : c->fifo)
            if (!e.ghost) c->slot_pool.push_back(e);
        c->fifo.clear();
        c->merged_ids.clear();
        c->m_n = 0;
        imls_ctx::MapSlot ghost;          // bookkeeping only: its data stays with the caller
        ghost.n = n;
        ghost.ghost = true;
        c->fifo.push_back(ghost);
        c->map_points = n;
        if (n == 0) {
            c->tgt_pending = false;
            c->has_target = false;
            c->has_corr = false;
            c->M = 0;
            if (n_map) *n_map = 0;
            return IMLS_OK;
        }
        return do_set_target(c, d_soa6, n, n_map);
    }
    imls_ctx::MapSlot sl;
    if (!c->slot_pool.empty()) { sl = c->slot_pool.back(); c->slot_pool.pop_back(); }
    sl.n = n;
    sl.ghost = false;
    sl.nk = -1;
    sl.sorted = false;
    const bool inc = fifo_incremental(c);
    sl.id = -1;                           // a pooled slot's run id / run belong to its last use
    if (inc) {
        for (const auto& e : c->fifo)     // a scan indexed in place (max_queue_size was 1) is not held
            if (e.ghost && e.n > 0) return fail(c, IMLS_ERR_STATE, "map FIFO holds a scan pushed with max_queue_size 1 (not kept): push again");
        sl.id = (int)(c->fifo_seq++ % kMaxFifoRuns);
        // an id is reused after kMaxFifoRuns pushes: if the merged order still holds its old run
        // (that many pushes without a build), the merged order restarts from the runs
        if (std::find(c->merged_ids.begin(), c->merged_ids.end(), sl.id) != c->merged_ids.end()) {
            c->merged_ids.clear();
            c->m_n = 0;
        }
    }
    if (n > 0) {
        int rc = IMLS_OK;
        const float* raw = d_soa6;
        if (!d_soa6 || !inc) {            // the incremental index filters a device scan where it lies
            if (!grow(sl.buf, n * 24)) { c->slot_pool.push_back(sl); return fail(c, IMLS_ERR_DEVICE, "hipMalloc (map slot)"); }
            if (d_soa6 && pose && !inc) {
                rc = pose_soa6(c->stream, d_soa6, (float*)sl.buf.p, n, *pose, c->err);
            } else if (d_soa6) {
                if (hipMemcpyAsync(sl.buf.p, d_soa6, n * 24, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
                    rc = fail(c, IMLS_ERR_DEVICE, "map slot copy");
            } else {
                rc = upload_soa6(c, sl.buf, xyz, nrm, n, stride, 0);
                if (!rc && pose && !inc) rc = pose_soa6(c->stream, (const float*)sl.buf.p, (float*)sl.buf.p, n, *pose, c->err);
            }
            raw = (const float*)sl.buf.p;
        }
        // incremental: this scan's NaN filter now, on the stream (its kept count into the pinned word
        // of its run id); its run is sorted at the next build
        if (!rc && inc && (rc = ensure_fifo(c)) == IMLS_OK)
            rc = filter_async(c->stream, raw, n, sl.fpt, sl.fnr, c->tscratch, nullptr, &c->h_fifo_cnt[sl.id], c->err, pose);
        if (rc) { c->slot_pool.push_back(sl); return rc; }
    }
    c->fifo.push_back(sl);
    c->map_points += n;
    if (c->fifo.size() > (size_t)std::max(c->P.max_queue_size, 0)) {
        c->map_points -= c->fifo.front().n;
        if (!c->fifo.front().ghost) c->slot_pool.push_back(c->fifo.front());
        c->fifo.pop_front();
    }
    if (inc) return fifo_set_target(c, n_map);
    return map_assemble(c, n_map);
}

// a caller's pose: every entry finite; *identity when it is exactly I (then the plain path runs:
// the same bits by construction, signed zeros included)
static bool read_pose(const double pose[16], Pose12* out, bool* identity) {
    bool id = true;
    for (int k = 0; k < 16; ++k) {
        if (!std::isfinite(pose[k])) return false;
        if (pose[k] != ((k % 5 == 0) ? 1.0 : 0.0)) id = false;
        if (k < 12) out->T[k] = pose[k];
    }
    *identity = id;
    return true;
}

int imls_set_initial_pose(imls_ctx* c, const double pose[16]) {
    if (!c) return IMLS_ERR_ARG;
    if (!pose) {
        for (int k = 0; k < 16; ++k) c->init_pose[k] = (k % 5 == 0) ? 1.0 : 0.0;
        return IMLS_OK;
    }
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(pose[k])) return fail(c, IMLS_ERR_ARG, "initial pose: non-finite entry");
    std::memcpy(c->init_pose, pose, sizeof(c->init_pose));
    return IMLS_OK;
}

int imls_map_push_posed(imls_ctx* c, const float* xyz, const float* nrm, size_t n, size_t stride, const double pose[16],
                        size_t* n_map) {
    if (!c) return IMLS_ERR_ARG;
    if (n > 0 && (!xyz || !nrm || stride < 3)) return fail(c, IMLS_ERR_ARG, "bad cloud pointer/stride");
    Pose12 P;
    bool identity = false;
    if (!pose || !read_pose(pose, &P, &identity)) return fail(c, IMLS_ERR_ARG, "map pose: null or non-finite entry");
    if (int rc = check_device(c)) return rc;
    return map_push(c, xyz, nrm, n, stride, nullptr, n_map, identity ? nullptr : &P);
}

int imls_map_push_posed_device(imls_ctx* c, const float* d_soa6, size_t n, const double pose[16], size_t* n_map) {
    if (!c || (n > 0 && !d_soa6)) return IMLS_ERR_ARG;
    Pose12 P;
    bool identity = false;
    if (!pose || !read_pose(pose, &P, &identity)) return fail(c, IMLS_ERR_ARG, "map pose: null or non-finite entry");
    if (int rc = check_device(c)) return rc;
    return map_push(c, nullptr, nullptr, n, 0, d_soa6, n_map, identity ? nullptr : &P);
}

// Every FIFO entry re-expressed in a new map frame (pose = new ← old), elementwise on the arrays the
// entries keep (the incremental index: each scan's filtered records; else its raw SoA6 scan); the
// quantisation frame is dropped, so the next build re-keys every run (fifo_build, !fq_valid).
int imls_map_rebase(imls_ctx* c, const double pose[16]) {
    if (!c) return IMLS_ERR_ARG;
    Pose12 P;
    bool identity = false;
    if (!pose || !read_pose(pose, &P, &identity)) return fail(c, IMLS_ERR_ARG, "map pose: null or non-finite entry");
    if (c->pending || c->batch_member) return fail(c, IMLS_ERR_STATE, "a registration is pending: collect its result first");
    if (int rc = check_device(c)) return rc;
    if (!identity && c->vox.n > 0) {      // the voxel map: its stored floats in place, the target re-installed
        if (int rc = pose_soa6(c->stream, (const float*)c->vox.buf[c->vox.cur].p, (float*)c->vox.buf[c->vox.cur].p, c->vox.n, P, c->err))
            return rc;
        return do_set_target(c, (const float*)c->vox.buf[c->vox.cur].p, c->vox.n, nullptr);
    }
    if (identity || c->map_points == 0) return IMLS_OK;
    for (const auto& e : c->fifo)
        if (e.ghost && e.n > 0)
            return fail(c, IMLS_ERR_STATE, "map FIFO holds a scan indexed in place (max_queue_size 1, not kept): nothing to rebase");
    const bool inc = fifo_incremental(c);
    for (auto& e : c->fifo) {
        if (e.n == 0) continue;
        // (a filter whose count has not been read yet kept at most e.n records: the arrays hold e.n)
        const int rc = inc ? pose_records(c->stream, (float4*)e.fpt.p, (float4*)e.fnr.p, e.nk >= 0 ? (size_t)e.nk : e.n, P, c->err)
                           : pose_soa6(c->stream, (const float*)e.buf.p, (float*)e.buf.p, e.n, P, c->err);
        if (rc) return rc;
    }
    if (!inc) return map_assemble(c, nullptr);
    c->fq_valid = false;
    c->merged_ids.clear();
    c->m_n = 0;
    return fifo_set_target(c, nullptr);
}

int imls_map_push(imls_ctx* c, const float* xyz, const float* nrm, size_t n, size_t stride, size_t* n_map) {
    if (!c) return IMLS_ERR_ARG;
    if (n > 0 && (!xyz || !nrm || stride < 3)) return fail(c, IMLS_ERR_ARG, "bad cloud pointer/stride");
    if (int rc = check_device(c)) return rc;
    return map_push(c, xyz, nrm, n, stride, nullptr, n_map);
}

int imls_map_push_device(imls_ctx* c, const float* d_soa6, size_t n, size_t* n_map) {
    if (!c || (n > 0 && !d_soa6)) return IMLS_ERR_ARG;
    if (int rc = check_device(c)) return rc;
    return map_push(c, nullptr, nullptr, n, 0, d_soa6, n_map);
}

int imls_map_clear(imls_ctx* c) {
    if (!c) return IMLS_ERR_ARG;
    for (auto& e : c->fifo)
        if (!e.ghost) c->slot_pool.push_back(e);
    c->fifo.clear();
    c->map_points = 0;
    c->merged_ids.clear();
    c->m_n = 0;
    c->fq_valid = false;
    c->vox.n = 0;
    return IMLS_OK;
}

int imls_map_size(imls_ctx* c, size_t* entries, size_t* points) {
    if (!c) return IMLS_ERR_ARG;
    if (entries) *entries = c->vox.n > 0 ? 1 : c->fifo.size();
    if (points) *points = c->vox.n > 0 ? c->vox.n : c->map_points;
    return IMLS_OK;
}

// ---- voxel map (include/imls_gpu.h "voxel map"; kernels in voxel_map.hip) ---------------------------
void imls_default_voxel_map_params(imls_voxel_map_params* p) {
    if (!p) return;
    p->voxel_size = 0.5f;
    p->max_per_voxel = 20;
    p->max_range = 100.0f;
}

int imls_voxel_map_set_params(imls_ctx* c, const imls_voxel_map_params* p) {
    if (!c || !p) return IMLS_ERR_ARG;
    if (!std::isfinite(p->voxel_size) || !(p->voxel_size > 0.f)) return fail(c, IMLS_ERR_ARG, "voxel_size must be finite and > 0");
    if (p->max_per_voxel < 1) return fail(c, IMLS_ERR_ARG, "max_per_voxel must be >= 1");
    if (!(p->max_range > 0.f)) return fail(c, IMLS_ERR_ARG, "max_range must be > 0 (+inf allowed)");
    c->vox.P = *p;
    return IMLS_OK;
}

// One update: the scan to its staging buffer (a host scan: uploaded there and transformed in place),
// the merge into the other map buffer, one wait for the record, the new map installed as the target.
static int voxel_update(imls_ctx* c, const float* xyz, const float* nrm, size_t n, size_t stride, const float* d_soa6,
                        const double pose[16], size_t* n_map) {
    auto& v = c->vox;
    VoxelGrid G{};
    bool identity = false;
    if (!pose || !read_pose(pose, &G.P, &identity)) return fail(c, IMLS_ERR_ARG, "map pose: null or non-finite entry");
    if (n > (size_t)0x7fffffff || v.n + n > (size_t)0x7fffffff) return fail(c, IMLS_ERR_ARG, "scan too large");
    if (c->pending || c->batch_member) return fail(c, IMLS_ERR_STATE, "a registration is pending: collect its result first");
    // (points on both sides: map_push tests vox.n; a FIFO of empty scans holds nothing)
    if (c->map_points > 0) return fail(c, IMLS_ERR_STATE, "the context holds a map FIFO: imls_map_clear first");
    if (int rc = check_device(c)) return rc;
    G.identity = identity ? 1 : 0;
    G.voxel = (double)v.P.voxel_size;
    G.r2 = (double)v.P.max_range * (double)v.P.max_range;
    G.cap = (unsigned long long)v.P.max_per_voxel;
    if (!v.h_rec && hipHostMalloc((void**)&v.h_rec, kVoxRecWords * sizeof(unsigned)) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "hipHostMalloc (voxel map)");
    if (!v.ev && hipEventCreateWithFlags(&v.ev, hipEventDisableTiming) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "hipEventCreate");
    const size_t n_old = v.n, total = n_old + n;
    const float* scan_in = d_soa6;
    if (n > 0 && !d_soa6) {
        if (int rc = upload_soa6(c, v.scan, xyz, nrm, n, stride, 0)) return rc;
        scan_in = (const float*)v.scan.p;
    } else if (n > 0 && !grow(v.scan, n * 24)) {
        return fail(c, IMLS_ERR_DEVICE, "hipMalloc (voxel map scan)");
    }
    if (total > 0 && !grow(v.buf[v.cur ^ 1], total * 24)) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (voxel map)");
    int slot = -1;
    timed_begin(c, kTimeVoxelMap, slot);
    const int rc = voxel_map_merge(c->stream, (const float*)v.buf[v.cur].p, n_old, scan_in, (float*)v.scan.p, n, G,
                                   (float*)v.buf[v.cur ^ 1].p, v.scratch, v.h_rec, c->err);
    timed_end(c, kTimeVoxelMap, slot);
    if (rc) return rc;
    if (hipEventRecord(v.ev, c->stream) != hipSuccess || hipEventSynchronize(v.ev) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "voxel map update failed");
    c->stage_pending[0] = false;          // the stream has passed every reader of an uploaded scan
    const unsigned* r = v.h_rec;
    imls_voxel_map_info& I = v.info;
    I.points = r[kVoxKept];
    I.voxels = r[kVoxVoxels];
    I.scan_nonfinite = r[kVoxScanNonfinite];
    I.scan_out_of_grid = r[kVoxScanGrid];
    I.scan_out_of_range = r[kVoxScanRange];
    I.scan_full = r[kVoxScanFull];
    I.map_out_of_grid = r[kVoxMapGrid];
    I.map_out_of_range = r[kVoxMapRange];
    I.map_trimmed = r[kVoxMapTrimmed];
    I.scan_inserted = (uint64_t)n - I.scan_nonfinite - I.scan_out_of_grid - I.scan_out_of_range - I.scan_full;
    v.cur ^= 1;
    v.n = (size_t)I.points;
    if (n_map) *n_map = v.n;
    if (v.n == 0) {                       // an empty map: no target (as map_assemble's M = 0)
        c->tgt_pending = false;
        c->has_target = false;
        c->has_corr = false;
        c->fifo_inc = false;
        c->M = 0;
        return IMLS_OK;
    }
    // (every stored point is finite, so the target's NaN filter keeps them all: no second wait for its count)
    return do_set_target(c, (const float*)v.buf[v.cur].p, v.n, nullptr);
}

int imls_voxel_map_update(imls_ctx* c, const float* xyz, const float* nrm, size_t n, size_t stride, const double pose[16],
                          size_t* n_map) {
    if (!c) return IMLS_ERR_ARG;
    if (n > 0 && (!xyz || !nrm || stride < 3)) return fail(c, IMLS_ERR_ARG, "bad cloud pointer/stride");
    return voxel_update(c, xyz, nrm, n, stride, nullptr, pose, n_map);
}

int imls_voxel_map_update_device(imls_ctx* c, const float* d_soa6, size_t n, const double pose[16], size_t* n_map) {
    if (!c || (n > 0 && !d_soa6)) return IMLS_ERR_ARG;
    return voxel_update(c, nullptr, nullptr, n, 0, d_soa6, pose, n_map);
}

int imls_voxel_map_info_get(imls_ctx* c, imls_voxel_map_info* out) {
    if (!c || !out) return IMLS_ERR_ARG;
    *out = c->vox.info;
    return IMLS_OK;
}

int imls_voxel_map_download(imls_ctx* c, float* soa6_out, size_t cap, size_t* n) {
    if (!c || !n) return IMLS_ERR_ARG;
    *n = c->vox.n;
    if (!soa6_out || c->vox.n == 0) return IMLS_OK;
    if (cap < c->vox.n) return fail(c, IMLS_ERR_CAPACITY, "voxel map download: buffer too small");
    if (int rc = check_device(c)) return rc;
    if (hipMemcpyAsync(soa6_out, c->vox.buf[c->vox.cur].p, c->vox.n * 24, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "voxel map download failed");
    return IMLS_OK;
}

}  // extern "C"
