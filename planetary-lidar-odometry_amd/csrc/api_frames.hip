// api_frames.hip — batched registration of the C ABI: imls_register_frames*, imls_batch*, and the
// batch's own index builds (batch_builds).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "context.h"
#include "index.h"
#include "solve.h"

using namespace imlsgpu;

// ------------------------------------------------------------------------------------------------
// Batched registration (imls_register_frames*): the frames loaded into n contexts run through ONE
// launch sequence — every per-iteration kernel once for all frames (grid y = frame) — on the lead
// context's stream, so n small frames fill the GPU together instead of n queues of tiny launches.
// ------------------------------------------------------------------------------------------------
namespace {

// IMLS_DEBUG_HOST=1: host-time split of imls_register_frames_async on stderr (diagnostics only)
struct HostSplit {
    bool on = std::getenv("IMLS_DEBUG_HOST") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), t = t0;
    char buf[512];
    int len = 0;
    void mark(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        len += std::snprintf(buf + len, sizeof(buf) - (size_t)len, " %s %.2f", what,
                             std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
    ~HostSplit() {
        if (on) std::fprintf(stderr, "[imls host ms]%s total %.2f\n", buf,
                             std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};

// The pending builds of a batch's members in ONE launch sequence on the lead's stream (index.hip
// build_batch: one radix sort for every frame's points): after each member's filter count (one
// host wait each, all filters already enqueued), the trees and source orders of all of them; the
// members' streams are then ordered after it.  Members with per-launch timing on keep their own
// build (its timing events are on their streams).
int batch_builds(imls_ctx* L, imls_ctx* const* ctxs, size_t n, bool fused, HostSplit* hs = nullptr) {
    bool any = false, timing = false;
    for (size_t k = 0; k < n; ++k) {
        any |= ctxs[k]->tgt_pending || ctxs[k]->src_pending;
        timing |= ctxs[k]->timing == 1;
    }
    if (!any) return IMLS_OK;
    // incremental FIFO targets (fifo_index.hip fifo_*): each member's own build on its stream (a merge of
    // sorted runs, not the batch's one radix sort), joined by the lead's stream
    for (size_t k = 0; k < n; ++k) {
        imls_ctx* c = ctxs[k];
        if (!c->tgt_pending || !c->fifo_inc) continue;
        if (int rc = finish_target(c)) return fail(L, rc, "context " + std::to_string(k) + ": " + c->err);
        if (c != L && c->has_target && hipStreamWaitEvent(L->stream, c->ev_fifo, 0) != hipSuccess)
            return fail(L, IMLS_ERR_DEVICE, "FIFO build join");
    }
    if (timing) {
        for (size_t k = 0; k < n; ++k)
            if (int rc = ensure_built(ctxs[k])) return fail(L, rc, "context " + std::to_string(k) + ": " + ctxs[k]->err);
        return IMLS_OK;
    }
    // the deferred NaN filters of every member: one launch sequence on the lead's stream, ordered
    // after each member's stream (its uploads), then one wait for all their counts
    {
        std::vector<FilterJob> fj;
        for (size_t k = 0; k < n; ++k) {
            imls_ctx* c = ctxs[k];
            // (a join only where the member's stream still has work: an idle stream's is done)
            if (c->tgt_pending && c->tgt_filter_deferred) {
                if (c != L && hipEventQuery(c->ev_tgt) != hipSuccess && hipStreamWaitEvent(L->stream, c->ev_tgt, 0) != hipSuccess)
                    return fail(L, IMLS_ERR_DEVICE, "filter join");
                if (!grow(c->tkept, c->tf_n * 4 + 16)) return fail(L, IMLS_ERR_DEVICE, "hipMalloc (kept)");
                fj.push_back(FilterJob{c->tf_soa, c->tf_n, &c->tpt, &c->tnr, (unsigned*)c->tkept.p, &c->h_cnt[0]});
                c->tgt_filter_deferred = false;
            }
            if (c->src_pending && c->src_filter_deferred) {
                if (c != L && hipEventQuery(c->ev_src) != hipSuccess && hipStreamWaitEvent(L->stream, c->ev_src, 0) != hipSuccess)
                    return fail(L, IMLS_ERR_DEVICE, "filter join");
                fj.push_back(FilterJob{c->sf_soa, c->sf_n, &c->spt, &c->snr, nullptr, &c->h_cnt[1]});
                c->src_filter_deferred = false;
            }
        }
        if (!fj.empty()) {
            const size_t tb = fj.size() * filter_job_bytes();
            if (L->h_ftable_bytes < tb) {
                if (L->h_ftable) (void)hipHostFree(L->h_ftable);
                L->h_ftable = nullptr;
                L->h_ftable_bytes = 0;
                if (hipHostMalloc(&L->h_ftable, tb + tb / 2 + 1024) != hipSuccess) return fail(L, IMLS_ERR_DEVICE, "hipHostMalloc (filter table)");
                L->h_ftable_bytes = tb + tb / 2 + 1024;
            }
            (void)hipSetDevice(L->device);
            if (int rc = filter_batch(L->stream, fj, L->fscratch, L->ftable, L->h_ftable, L->h_ftable_bytes, L->err)) return rc;
            if (hs) hs->mark("filter-launch");
            if (hipStreamSynchronize(L->stream) != hipSuccess) return fail(L, IMLS_ERR_DEVICE, "batched filter failed");
            if (hs) hs->mark("filter-wait");
        }
    }
    std::vector<BuildJob> jobs;
    std::vector<std::pair<imls_ctx*, int>> who;   // (context, 0 target / 1 source)
    for (size_t k = 0; k < n; ++k) {
        imls_ctx* c = ctxs[k];
        if (c->tgt_pending) {
            c->tgt_pending = false;
            if (hipEventSynchronize(c->ev_tgt) != hipSuccess) return fail(L, IMLS_ERR_DEVICE, "target filter failed");
            c->stage_pending[0] = false;
            c->M = c->h_cnt[0];
            c->Pl = c->levels = 0;
            c->has_target = c->M > 0;
            timed_end(c, kTimeIndex, c->tgt_slot);
            c->tgt_slot = -1;
            if (c->M > 0) {
                const int Lv = (c->M + c->B - 1) / c->B;
                int P = 1;
                while (P < Lv) P <<= 1;
                if (!grow(c->lkeys, (size_t)Lv * 8 + 16) || !grow(c->mpt, (size_t)c->M * 36 + 64) ||
                    !grow(c->nodes, (size_t)(P + 1) * 48))
                    return fail(L, IMLS_ERR_DEVICE, "hipMalloc (index)");
                jobs.push_back(BuildJob{(const float4*)c->tpt.p, (const float4*)c->tnr.p, c->M, c->B,
                                        (unsigned long long*)c->lkeys.p, (float4*)c->mpt.p, (float4*)c->nodes.p, nullptr, 0, 0});
                who.push_back({c, 0});
            }
        }
        if (c->src_pending) {
            c->src_pending = false;
            if (hipEventSynchronize(c->ev_src) != hipSuccess) return fail(L, IMLS_ERR_DEVICE, "source filter failed");
            c->stage_pending[1] = false;
            c->N = c->h_cnt[1];
            c->has_source = c->N > 0;
            c->src_kept_out = nullptr;
            if (c->N > 0) {
                if (!grow(c->qperm, (size_t)c->N * 4 + 16)) return fail(L, IMLS_ERR_DEVICE, "hipMalloc (source order)");
                if (n == 1 && c == L && c->N <= kSmallOrderN) {
                    // a lone small frame: its source order in one launch (index.hip), not the
                    // batched build's 6-8 — the same permutation
                    if (int rc = small_source_order(L->stream, (const float4*)c->spt.p, c->N, (unsigned*)c->qperm.p, L->err))
                        return fail(L, rc, L->err);
                } else {
                    jobs.push_back(BuildJob{(const float4*)c->spt.p, nullptr, c->N, 0, nullptr, nullptr, nullptr,
                                            (unsigned*)c->qperm.p, 0, 0});
                    who.push_back({c, 1});
                }
            }
            if (int rc = ensure_solve(c, c->N)) return fail(L, rc, c->err);
        }
    }
    if (jobs.empty()) return IMLS_OK;
    const size_t tb = jobs.size() * build_job_bytes();
    if (L->h_btable_bytes < tb) {
        if (L->h_btable) (void)hipHostFree(L->h_btable);
        L->h_btable = nullptr;
        L->h_btable_bytes = 0;
        if (hipHostMalloc(&L->h_btable, tb + tb / 2 + 1024) != hipSuccess) return fail(L, IMLS_ERR_DEVICE, "hipHostMalloc (build table)");
        L->h_btable_bytes = tb + tb / 2 + 1024;
    }
    (void)hipSetDevice(L->device);
    if (int rc = build_batch(L->stream, jobs, L->bscratch, L->btable, L->h_btable, L->h_btable_bytes, L->err)) return rc;
    for (size_t q = 0; q < jobs.size(); ++q)
        if (who[q].second == 0) {
            who[q].first->Pl = jobs[q].P;
            who[q].first->levels = jobs[q].levels;
        }
    for (size_t k = 0; k < n; ++k) {          // tensors set while the build was pending (config E)
        imls_ctx* c = ctxs[k];
        if (!c->ten_pending) continue;
        c->ten_pending = false;
        if (!c->has_target) { c->has_tensors = false; continue; }
        if (int rc = gather_tensors(c, L->stream, c->ten_src, c->ten_n)) return fail(L, rc, c->err);
    }
    // every member's later work on its own stream (its frame's launches when the batch is not fused)
    // is ordered after the build (a fused batch orders them after the whole batch instead)
    if (fused) return IMLS_OK;
    if (!L->ev_build && hipEventCreateWithFlags(&L->ev_build, hipEventDisableTiming) != hipSuccess)
        return fail(L, IMLS_ERR_DEVICE, "hipEventCreate (build)");
    if (hipEventRecord(L->ev_build, L->stream) != hipSuccess) return fail(L, IMLS_ERR_DEVICE, "build event");
    for (size_t k = 0; k < n; ++k)
        if (ctxs[k] != L && hipStreamWaitEvent(ctxs[k]->stream, L->ev_build, 0) != hipSuccess)
            return fail(L, IMLS_ERR_DEVICE, "build stream join");
    return IMLS_OK;
}


constexpr int kResStride = 20;   // per frame: pose[16], iters, status
// the batch's frame table is followed by every frame's initial pose ([n] records, then [n][16] doubles)
static_assert(sizeof(PairDev) % alignof(double) == 0, "initial poses follow the frame table");
constexpr size_t kTabEntryBytes = sizeof(PairDev) + 16 * sizeof(double);

// rPose = the frame's initial pose (init[16·frame]; identity unless imls_set_initial_pose), done /
// status / iters = 0, the frame's trace and counters cleared (one launch for the whole batch
// instead of six fills per frame)
__global__ void k_batch_init(const PairDev* __restrict__ tab, int iters, const double* __restrict__ init) {
    const PairDev A = tab[blockIdx.x];
    const int t = threadIdx.x;
    if (t < 16) A.st.pose[t] = init[(size_t)blockIdx.x * 16 + t];
    if (t == 0) { *A.st.done = 0; *A.st.status = 0; *A.st.iters = 0; }
    if (A.stats && t < 16) A.stats[t] = 0ull;
    unsigned long long* tr = reinterpret_cast<unsigned long long*>(A.trace);
    const int words = iters * (int)(sizeof(imls_iter_trace) / 8);
    for (int k = t; k < words; k += blockDim.x) tr[k] = 0ull;
}

// per frame: pose, iterations, status ([n][kResStride]), then every frame's trace records gathered
// after them ([n][iters] records) — one device-to-host copy for the whole batch
__global__ void k_batch_results(const PairDev* __restrict__ tab, int n, double* __restrict__ out, int iters) {
    const int words = iters * (int)(sizeof(imls_iter_trace) / 8);
    unsigned long long* tout = reinterpret_cast<unsigned long long*>(out + (size_t)n * kResStride);
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        const PairDev A = tab[k];
        const int t = threadIdx.x;
        if (t < 16) out[(size_t)k * kResStride + t] = A.st.pose[t];
        if (t == 16) out[(size_t)k * kResStride + 16] = (double)*A.st.iters;
        if (t == 17) out[(size_t)k * kResStride + 17] = (double)*A.st.status;
        const unsigned long long* tr = reinterpret_cast<const unsigned long long*>(A.trace);
        for (int w = t; w < words; w += blockDim.x) tout[(size_t)k * words + w] = tr[w];
    }
}

// The batched path covers both matchers (tensor-voting normals included) with the LS-family solvers,
// the robust solve and RANSAC (+ its LS / weighted LS / DRPM final solve); the projected-distance rule and the exact
// per-lane mode keep one launch sequence per frame (each on its own context stream, so they still
// overlap).
bool batch_fusable(const imls_ctx* c) {
    return !c->lane_mode && !c->kp.proj &&
           (c->P.solve_method == IMLS_SOLVE_LS || c->P.solve_method == IMLS_SOLVE_WEIGHTED_LS ||
            c->P.solve_method == IMLS_SOLVE_RANSAC || c->P.solve_method == IMLS_SOLVE_ROBUST);
}

PairDev pair_dev(imls_ctx* c) {
    PairDev A{};
    A.t = tree_view(c);
    A.spt = (const float4*)c->spt.p;
    A.snr = (const float4*)c->snr.p;
    A.qperm = (const unsigned*)c->qperm.p;
    A.N = c->N;
    A.cs = (float4*)c->cs.p;
    A.cd = (float4*)c->cd.p;
    A.cn = (float4*)c->cn.p;
    A.lists = (int*)c->prevnn.p;
    A.st = c->st;
    A.trace = (imls_iter_trace*)c->trace_mem.p;
    A.stats = stats_ptr(c);
    A.fb_list = fb_list(c);
    A.fb_count = fb_count(c);
    if (c->P.solve_method == IMLS_SOLVE_RANSAC) A.rf = ransac_frame(c->ransac_mem.p, c->N, (int*)c->rng.p);
    return A;
}

int frames_async(imls_ctx* const* ctxs, size_t n) {
    if (!ctxs || n == 0 || !ctxs[0]) return IMLS_ERR_ARG;
    HostSplit hs;
    imls_ctx* L = ctxs[0];
    if (L->batch_pending) return fail(L, IMLS_ERR_STATE, "a batch led by this context is pending");
    if (int rc = check_device(L)) return rc;
    for (size_t k = 0; k < n; ++k) {
        imls_ctx* c = ctxs[k];
        if (!c) return fail(L, IMLS_ERR_ARG, "null context in the batch");
        c->info_state = 0;                // the previous frame's report is gone, whatever happens below
        c->cap_iters = 0;                 // batched frames capture nothing: drop an older capture
        if (c->device != L->device) return fail(L, IMLS_ERR_ARG, "batch contexts must share one device");
        imls_params pc = c->P, pl = L->P;
        pc.ransac_seed = pl.ransac_seed = 0;    // each context runs its own rand() stream
        if (std::memcmp(&pc, &pl, sizeof(imls_params)) != 0)
            return fail(L, IMLS_ERR_ARG, "batch contexts must share their params (context " + std::to_string(k) + ")");
        if (!same_options(c->opt, L->opt))
            return fail(L, IMLS_ERR_ARG, "batch contexts must share their options (imls_set_option)");
        if (c->pending || c->batch_member || (k > 0 && c->batch_pending))
            return fail(L, IMLS_ERR_STATE, "context " + std::to_string(k) + " has a frame pending");
    }
    {   // no context twice (sorted copy: O(n log n) for batches of thousands of frames)
        std::vector<imls_ctx*> sorted(ctxs, ctxs + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return fail(L, IMLS_ERR_ARG, "a context appears twice in the batch");
    }
    // every member's deferred build: its filter count (one wait each, all filters already enqueued)
    // then all the members' index builds in one launch sequence on the lead's stream
    hs.mark("checks");
    bool fuse = batch_fusable(L) && (L->P.solve_method != IMLS_SOLVE_RANSAC || n <= (size_t)kMaxRansacBatch);
    if (int rc = batch_builds(L, ctxs, n, fuse, &hs))
        return rc;
    // a batch of ONE small frame takes the single-frame launches — the lone-frame path with the exact
    // stage fused into the wave-per-query traversal (two launches per ICP iteration, not three; the
    // same results): the 2000-query config B variant 1450 → 1835 pairs/s (profiles/r05_ab/r05n_q).
    // A large frame keeps the table-driven kernels, measured faster in flight (435-445 vs 430-433
    // pairs/s on config B, though each launch alone is slower: profiles/r05_ab/r05n)
    if (n == 1 && L->has_source && L->N <= kSmallRows && (L->kp.qwave > 0 || (L->kp.qwave < 0 && L->N <= kQwaveAutoN))) {
        fuse = false;                     // (its builds ran on its own stream: nothing to join)
    }
    hs.mark("filters+builds");
    (void)hipSetDevice(L->device);
    for (size_t k = 0; k < n; ++k) {
        imls_ctx* c = ctxs[k];
        if (!c->has_target || !c->has_source)
            return fail(L, IMLS_ERR_STATE, "context " + std::to_string(k) + ": set_target and set_source first");
    }
    L->members.assign(ctxs, ctxs + n);
    L->batch_fused = fuse;
    if (!L->batch_fused) {
        // one launch sequence per frame, each on its own context stream
        for (size_t k = 0; k < n; ++k) {
            if (int rc = imls_register_frame_async(ctxs[k])) {
                for (size_t j = 0; j < k; ++j) (void)imls_register_frame_result(ctxs[j], nullptr, nullptr, nullptr, nullptr);
                if (k > 0) L->err = imls_last_error(ctxs[k]);
                return rc;
            }
        }
        for (size_t k = 0; k < n; ++k) ctxs[k]->batch_member = true;
        L->batch_pending = true;
        return IMLS_OK;
    }
    const int iters = L->P.iterations;
    const size_t res_bytes = n * (kResStride * sizeof(double) + (size_t)std::max(iters, 0) * sizeof(imls_iter_trace));
    if ((size_t)L->tab_cap < n) {
        if (L->tab_h) (void)hipHostFree(L->tab_h);
        L->tab_h = nullptr;
        L->tab_cap = 0;
        if (hipHostMalloc((void**)&L->tab_h, n * kTabEntryBytes) != hipSuccess)
            return fail(L, IMLS_ERR_DEVICE, "hipHostMalloc (batch)");
        L->tab_cap = (int)n;
    }
    if (L->res_h_bytes < res_bytes) {
        if (L->res_h) (void)hipHostFree(L->res_h);
        L->res_h = nullptr;
        L->res_h_bytes = 0;
        if (hipHostMalloc((void**)&L->res_h, res_bytes) != hipSuccess) return fail(L, IMLS_ERR_DEVICE, "hipHostMalloc (batch)");
        L->res_h_bytes = res_bytes;
    }
    if (!grow(L->tab_d, n * kTabEntryBytes) || !grow(L->res_d, res_bytes))
        return fail(L, IMLS_ERR_DEVICE, "hipMalloc (batch)");
    if (!L->ev_batch && hipEventCreateWithFlags(&L->ev_batch, hipEventDisableTiming) != hipSuccess)
        return fail(L, IMLS_ERR_DEVICE, "hipEventCreate (batch)");
    hipStream_t s = L->stream;
    L->member_n.assign(n, 0);
    bool any_nrm = false;
    int max_m = 0;
    for (size_t k = 0; k < n; ++k) {
        imls_ctx* c = ctxs[k];
        if (int rc = ensure_solve(c, c->N)) return fail(L, rc, c->err);
        if (int rc = ensure_trace(c, iters)) return fail(L, rc, c->err);
        if (!grow(c->stats, 128)) return fail(L, IMLS_ERR_DEVICE, "hipMalloc");
        // count-mode map normals (get_normals false): flagged here, computed for all the frames that
        // need them by one batched launch ahead of the iterations
        const bool need_nrm = !c->P.get_normals && c->P.recompute_normal_count_mode &&
                              !(c->rnr_valid && c->rnr_k == c->P.search_number_normal && c->rnr_r == c->P.r_normal);
        if (need_nrm) {
            // (valid only once the launch below has been issued: a later member's failed check returns
            // before it, and this member's next use must then compute them)
            c->rnr_valid = false;
            if (!grow(c->rnr, (size_t)std::max(c->M, 1) * 16)) return fail(L, IMLS_ERR_DEVICE, "hipMalloc (normals)");
            any_nrm = true;
            max_m = std::max(max_m, c->M);
        }
        if (int rc = check_tv_ready(c)) return fail(L, rc, "context " + std::to_string(k) + ": " + c->err);
        if (int rc = prepare_ransac(c, c->N)) return fail(L, rc, c->err);
        if (int rc = info_begin(c, c->N, s)) return fail(L, rc, c->err);   // (its memset: ordered after the join below by the table's copy)
        L->tab_h[k] = pair_dev(c);
        std::memcpy(reinterpret_cast<double*>(L->tab_h + n) + 16 * k, c->init_pose, 16 * sizeof(double));
        L->tab_h[k].recompute_normals = need_nrm ? 1 : 0;
        L->member_n[k] = c->N;
        if (c != L && hipStreamQuery(c->stream) != hipSuccess) {
            // work of the frame still queued on its own stream (uploads, a counted filter or build):
            // the batch waits for it (an idle stream's work is complete: no join)
            if (!c->ev_batch && hipEventCreateWithFlags(&c->ev_batch, hipEventDisableTiming) != hipSuccess)
                return fail(L, IMLS_ERR_DEVICE, "hipEventCreate (batch)");
            if (hipEventRecord(c->ev_batch, c->stream) != hipSuccess || hipStreamWaitEvent(s, c->ev_batch, 0) != hipSuccess)
                return fail(L, IMLS_ERR_DEVICE, "batch stream join");
        }
    }
    (void)hipSetDevice(L->device);
    hs.mark("members");
    const PairDev* tab = (const PairDev*)L->tab_d.p;
    hipMemcpyAsync(L->tab_d.p, L->tab_h, n * kTabEntryBytes, hipMemcpyHostToDevice, s);
    k_batch_init<<<(unsigned)n, 64, 0, s>>>(tab, iters, reinterpret_cast<const double*>(tab + n));
    if (any_nrm && launch_map_normals_batch(s, tab, (int)n, max_m, L->P.search_number_normal, L->P.r_normal))
        return fail(L, IMLS_ERR_DEVICE, "batched map normal launch failed");
    for (size_t k = 0; k < n; ++k) {
        if (!L->tab_h[k].recompute_normals) continue;
        ctxs[k]->rnr_valid = true;
        ctxs[k]->rnr_k = ctxs[k]->P.search_number_normal;
        ctxs[k]->rnr_r = ctxs[k]->P.r_normal;
    }
    const KParams kp = L->kp;
    const RansacParams rp = ransac_params(L->P);
    const int* nh = L->member_n.data();
    for (int it = 0; it < iters; ++it) {
        int slot;
        timed_begin(L, kTimeProject, slot);
        launch_project_batch(s, tab, nh, (int)n, kp, it, it > 0 && L->temporal_seed);
        timed_end(L, kTimeProject, slot);
        timed_begin(L, kTimeSolve, slot);
        if (launch_solve_frames(s, tab, nh, (int)n, kp, rp, it))
            return fail(L, IMLS_ERR_CAPACITY, "RANSAC batch larger than kMaxRansacBatch frames");
        timed_end(L, kTimeSolve, slot);
    }
    // every capturing member's pose-info pass, the lone frame's two launches on the same rows: the
    // same bits alone and batched
    for (size_t k = 0; k < n; ++k)
        if (int rc = info_enqueue(ctxs[k], L, s, kp.solve_method, nullptr, nullptr, ctxs[k]->N, 1)) return fail(L, rc, ctxs[k]->err);
    hs.mark("iterations");
    k_batch_results<<<(unsigned)std::min<size_t>(n, 1024), 64, 0, s>>>(tab, (int)n, (double*)L->res_d.p, std::max(iters, 0));
    hipMemcpyAsync(L->res_h, L->res_d.p, res_bytes, hipMemcpyDeviceToHost, s);
    L->batch_traces = iters > 0;
    if (hipGetLastError() != hipSuccess) return fail(L, IMLS_ERR_DEVICE, "batch launch failed");
    // every member's later work (its next uploads / index build) is ordered after the batch
    if (hipEventRecord(L->ev_batch, s) != hipSuccess) return fail(L, IMLS_ERR_DEVICE, "batch event");
    for (size_t k = 1; k < n; ++k)
        if (hipStreamWaitEvent(ctxs[k]->stream, L->ev_batch, 0) != hipSuccess) return fail(L, IMLS_ERR_DEVICE, "batch stream join");
    for (size_t k = 0; k < n; ++k) { ctxs[k]->has_corr = true; ctxs[k]->batch_member = true; }
    L->batch_pending = true;
    return IMLS_OK;
}

int frames_result(imls_ctx* L, double* poses_out, int32_t* iters_out, int32_t* status_out, imls_iter_trace* traces) {
    if (!L) return IMLS_ERR_ARG;
    if (!L->batch_pending) return fail(L, IMLS_ERR_STATE, "no batch pending");
    L->batch_pending = false;
    const size_t n = L->members.size();
    for (imls_ctx* m : L->members) m->batch_member = false;
    const int iters = L->P.iterations;
    if (!L->batch_fused) {
        int first = IMLS_OK;
        for (size_t k = 0; k < n; ++k) {
            double pose[16];
            int it = 0, st = 0;
            const int rc = imls_register_frame_result(L->members[k], pose, &it, &st,
                                                      traces ? traces + k * (size_t)std::max(iters, 0) : nullptr);
            if (rc != IMLS_OK) {
                if (first == IMLS_OK) { first = rc; L->err = "frame " + std::to_string(k) + ": " + imls_last_error(L->members[k]); }
                continue;
            }
            if (poses_out) std::memcpy(poses_out + 16 * k, pose, sizeof(pose));
            if (iters_out) iters_out[k] = it;
            if (status_out) status_out[k] = st;
        }
        return first;
    }
    hipError_t e = hipStreamSynchronize(L->stream);
    if (e != hipSuccess) return fail(L, IMLS_ERR_DEVICE, std::string("batch failed: ") + hipGetErrorString(e));
    harvest_timing(L);
    for (imls_ctx* m : L->members)
        if (m->info_state == 1) m->info_state = 2;
    for (size_t k = 0; k < n; ++k) {
        const double* r = L->res_h + k * kResStride;
        if (poses_out) std::memcpy(poses_out + 16 * k, r, 16 * sizeof(double));
        if (iters_out) iters_out[k] = (int32_t)r[16];
        if (status_out) status_out[k] = (int32_t)r[17];
        if (traces && iters > 0)
            std::memcpy(traces + k * (size_t)iters,
                        reinterpret_cast<const imls_iter_trace*>(L->res_h + n * kResStride) + k * (size_t)iters,
                        (size_t)iters * sizeof(imls_iter_trace));
    }
    return IMLS_OK;
}

}  // namespace

extern "C" {

int imls_register_frames_async(imls_ctx* const* ctxs, size_t n) { return frames_async(ctxs, n); }

int imls_register_frames_result(imls_ctx* lead, double* poses_out, int32_t* iters_out, int32_t* status_out,
                                imls_iter_trace* traces) {
    return frames_result(lead, poses_out, iters_out, status_out, traces);
}

int imls_register_frames(imls_ctx* const* ctxs, size_t n, double* poses_out, int32_t* iters_out, int32_t* status_out,
                         imls_iter_trace* traces) {
    if (int rc = frames_async(ctxs, n)) return rc;
    return frames_result(ctxs[0], poses_out, iters_out, status_out, traces);
}

}  // extern "C"

struct imls_batch {
    std::vector<imls_ctx*> ctx;
    std::string err;
};

extern "C" {

imls_batch* imls_batch_create(int device, const imls_params* p, int32_t streams) {
    if (streams < 1 || streams > 256) return nullptr;
    imls_batch* b = new imls_batch();
    for (int s = 0; s < streams; ++s) {
        imls_ctx* c = imls_create(device, p);
        if (!c) {
            imls_batch_destroy(b);
            return nullptr;
        }
        b->ctx.push_back(c);
    }
    return b;
}

void imls_batch_destroy(imls_batch* b) {
    if (!b) return;
    for (imls_ctx* c : b->ctx) imls_destroy(c);
    delete b;
}

const char* imls_batch_last_error(const imls_batch* b) { return b ? b->err.c_str() : "null batch"; }

int imls_register_batch(imls_batch* b, size_t n_pairs, const imls_pair_input* pairs, double* poses_out,
                        int32_t* iters_out, int32_t* status_out) {
    if (!b) return IMLS_ERR_ARG;
    if (n_pairs > 0 && !pairs) { b->err = "null pairs"; return IMLS_ERR_ARG; }
    // groups of S pairs (one per context): upload + index every pair of the group, then register the
    // group as ONE launch sequence (imls_register_frames)
    const size_t S = b->ctx.size();
    for (size_t g = 0; g < n_pairs; g += S) {
        const size_t m = std::min(S, n_pairs - g);
        for (size_t k = 0; k < m; ++k) {
            imls_ctx* c = b->ctx[k];
            const imls_pair_input& q = pairs[g + k];
            // independent pairs: each starts the RANSAC rand() stream from params.ransac_seed (as the
            // reference's process does for its first frame), so a pair's result does not depend on
            // `streams` or on the pairs its context handled before
            ransac_seed_host(c->P.ransac_seed, c->rng_seed_state);
            c->rng_dirty = true;
            int rc = imls_set_target(c, q.tgt_xyz, q.tgt_nrm, q.n_tgt, q.stride_floats, nullptr);
            if (rc == IMLS_OK) rc = imls_set_source(c, q.src_xyz, q.src_nrm, q.n_src, q.stride_floats, nullptr, nullptr);
            if (rc != IMLS_OK) {
                b->err = "pair " + std::to_string(g + k) + ": " + imls_last_error(c);
                return rc;
            }
        }
        const int rc = imls_register_frames(b->ctx.data(), m, poses_out ? poses_out + 16 * g : nullptr,
                                            iters_out ? iters_out + g : nullptr, status_out ? status_out + g : nullptr,
                                            nullptr);
        if (rc != IMLS_OK) {
            b->err = "pairs " + std::to_string(g) + "..: " + imls_last_error(b->ctx[0]);
            return rc;
        }
    }
    return IMLS_OK;
}

}  // extern "C"
