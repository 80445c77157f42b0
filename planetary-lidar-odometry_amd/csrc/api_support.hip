// api_support.hip — what the C ABI units lean on and that touches no context state beyond its
// timing and upload staging: the retire-instead-of-free buffer registry, event-pair timing and
// its ABI (imls_enable_timing … imls_index_stats), and the host worker pool that packs uploads.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>
#include <unistd.h>

#include "context.h"

using namespace imlsgpu;

// ---- device buffers: retire instead of free (internal.h devbuf_grow) ------------------------------
namespace imlsgpu {
namespace {
struct Retired {
    void* p;
    size_t bytes;
    int device;
    std::vector<hipEvent_t> ev;       // one per stream that still had work when it was retired
};
std::mutex g_mem_mu;
struct StreamRef {
    hipStream_t s;
    int device, refs;
};
std::vector<StreamRef> g_streams;
std::vector<Retired> g_retired;

bool retired_ready(Retired& r) {
    for (size_t k = 0; k < r.ev.size(); ++k)
        if (hipEventQuery(r.ev[k]) != hipSuccess) return false;
    for (hipEvent_t e : r.ev) (void)hipEventDestroy(e);
    r.ev.clear();
    return true;
}
}  // namespace

void register_stream(hipStream_t s, int device) {
    if (!s) return;
    std::lock_guard<std::mutex> lk(g_mem_mu);
    for (auto& r : g_streams)
        if (r.s == s) { ++r.refs; return; }
    g_streams.push_back({s, device, 1});
}

void unregister_stream(hipStream_t s) {
    if (!s) return;
    std::lock_guard<std::mutex> lk(g_mem_mu);
    for (size_t k = 0; k < g_streams.size(); ++k)
        if (g_streams[k].s == s && --g_streams[k].refs == 0) {
            g_streams.erase(g_streams.begin() + (long)k);
            return;
        }
}

void devbuf_retire(DevBuf& b) {
    if (!b.p) return;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_mem_mu);
    Retired r{b.p, b.bytes, dev, {}};
    for (const auto& sr : g_streams) {
        if (sr.device != dev || hipStreamQuery(sr.s) == hipSuccess) continue;   // idle: all its work has run
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess && hipEventRecord(e, sr.s) == hipSuccess) {
            r.ev.push_back(e);
        } else {
            // no event to wait for (never expected): wait for that stream here instead
            if (e) (void)hipEventDestroy(e);
            (void)hipStreamSynchronize(sr.s);
        }
    }
    g_retired.push_back(std::move(r));
    b.p = nullptr;
    b.bytes = 0;
}

bool devbuf_grow(DevBuf& b, size_t bytes, size_t alloc) {
    if (b.bytes >= bytes) return true;
    devbuf_retire(b);
    alloc = std::max(alloc, bytes);
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        // a retired buffer whose readers have all finished: the smallest that fits, at most 4× the size
        std::lock_guard<std::mutex> lk(g_mem_mu);
        long best = -1;
        for (size_t k = 0; k < g_retired.size(); ++k) {
            Retired& r = g_retired[k];
            if (r.device != dev || r.bytes < alloc || r.bytes > 4 * alloc) continue;
            if (best >= 0 && r.bytes >= g_retired[(size_t)best].bytes) continue;
            if (retired_ready(r)) best = (long)k;
        }
        if (best >= 0) {
            b.p = g_retired[(size_t)best].p;
            b.bytes = g_retired[(size_t)best].bytes;
            g_retired.erase(g_retired.begin() + best);
            return true;
        }
    }
    if (hipMalloc(&b.p, alloc) != hipSuccess) {
        b.p = nullptr;
        return false;
    }
    b.bytes = alloc;
    return true;
}

void release_retired(int device) {
    std::lock_guard<std::mutex> lk(g_mem_mu);
    std::vector<Retired> keep;
    for (auto& r : g_retired) {
        if (r.device != device) { keep.push_back(std::move(r)); continue; }
        for (hipEvent_t e : r.ev) (void)hipEventDestroy(e);
        (void)hipFree(r.p);                                // teardown: hipFree waits for the device
    }
    g_retired.swap(keep);
}

// ---- timing: event pairs per launch kind (context.h TimingKind) -----------------------------------
int ev_pair(imls_ctx* c) {
    if (c->ev_used + 2 > (int)c->ev.size()) {
        for (int k = 0; k < 64; ++k) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return -1;
            c->ev.push_back(e);
        }
    }
    int i = c->ev_used;
    c->ev_used += 2;
    return i;
}

void timed_begin(imls_ctx* c, int kind, int& slot) {
    slot = -1;
    if (!c->timing) return;
    slot = ev_pair(c);
    if (slot >= 0) hipEventRecord(c->ev[slot], c->stream);
}
void timed_end(imls_ctx* c, int kind, int slot) {
    if (slot < 0) return;
    hipEventRecord(c->ev[slot + 1], c->stream);
    c->ev_pairs[kind].push_back({slot, slot + 1});
}
// Events around the two projection kernels (kTimeKnnWave, kTimeFinish): marks[0..2], or null when off.
hipEvent_t* project_marks(imls_ctx* c, hipEvent_t marks[3]) {
    if (!c->timing) return nullptr;
    const int a = ev_pair(c), b = ev_pair(c);
    if (a < 0 || b < 0) return nullptr;
    marks[0] = c->ev[a];
    marks[1] = c->ev[a + 1];
    marks[2] = c->ev[b];
    c->ev_pairs[kTimeKnnWave].push_back({a, a + 1});
    c->ev_pairs[kTimeFinish].push_back({a + 1, b});
    return marks;
}
// Events around one producer call's kernels: marks[0..1] = the pair at `slot`, or null (slot −1)
// when off.  The caller records {slot, slot + 1} under its kind, by its own rule.
hipEvent_t* pair_marks(imls_ctx* c, hipEvent_t marks[2], int& slot) {
    slot = -1;
    if (!c->timing || (slot = ev_pair(c)) < 0) return nullptr;
    marks[0] = c->ev[slot];
    marks[1] = c->ev[slot + 1];
    return marks;
}

namespace {
// Process-wide origin of the timing intervals (imls_timing_origin): one clock per device for every
// context of that device, so the busy time of concurrent launch sequences is the union of their
// intervals.  One origin per device, created once and never destroyed while the process runs (a
// context on another device cannot pull an origin out from under this one); the mutex orders the
// origin's (re)recording against the comparisons in harvest_timing.
constexpr int kMaxDevices = 64;
std::mutex g_origin_mu;
hipEvent_t g_origin[kMaxDevices] = {};
bool g_origin_set[kMaxDevices] = {};
// intervals kept per context and launch kind until imls_reset_timing / imls_timing_origin (a cap:
// a caller that never resets keeps a bounded record, the oldest first)
constexpr size_t kMaxIntervals = (size_t)1 << 20;
}  // namespace

void harvest_timing(imls_ctx* c) {
    std::lock_guard<std::mutex> lk(g_origin_mu);
    const bool dev_ok = c->device >= 0 && c->device < kMaxDevices;
    const bool iv = dev_ok && g_origin_set[c->device];
    for (int k = 0; k < kTimingKinds; ++k) {
        for (auto& pr : c->ev_pairs[k]) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, c->ev[pr.first], c->ev[pr.second]) == hipSuccess) {
                c->t_ms[k] += ms;
                c->t_n[k] += 1;
                float a = 0, b = 0;
                if (iv && c->iv[k].size() < kMaxIntervals &&
                    hipEventElapsedTime(&a, g_origin[c->device], c->ev[pr.first]) == hipSuccess &&
                    hipEventElapsedTime(&b, g_origin[c->device], c->ev[pr.second]) == hipSuccess)
                    c->iv[k].push_back({a, b});
            }
        }
        c->ev_pairs[k].clear();
    }
    c->ev_used = 0;
}

namespace {
// Persistent host workers for the upload packing: a scan of ~10^5 points is a strided gather of
// several MB, split over a few threads — created once per process, not per call (spawning 7
// std::threads per upload cost ~0.2 ms, more than the gather itself: round 3 measured 333 µs per
// 118k-point scan).  One job at a time (the mutex serialises contexts on other host threads).
class PackPool {
public:
    static PackPool& get() {
        static PackPool pool;
        return pool;
    }
    size_t width() const { return workers_.size() + 1; }
    // fn(i0, i1) over [0, n) in `parts` contiguous chunks (parts ≤ width()), the caller taking the first
    void run(size_t n, size_t parts, const std::function<void(size_t, size_t)>& fn) {
        parts = std::max<size_t>(1, std::min(parts, width()));
        // a forked child inherits the pool object but not its threads: pack serially there
        if (parts == 1 || n == 0 || getpid() != pid_) {
            fn(0, n);
            return;
        }
        std::lock_guard<std::mutex> job_lock(job_mu_);
        const size_t chunk = (n + parts - 1) / parts;
        {
            std::lock_guard<std::mutex> lk(mu_);
            fn_ = &fn;
            n_ = n;
            chunk_ = chunk;
            parts_ = parts;
            pending_ = parts - 1;
            pending_left_.store(parts - 1, std::memory_order_release);
            ++gen_;
        }
        gen_seen_.store(gen_, std::memory_order_release);
        cv_.notify_all();
        fn(0, std::min(n, chunk));
        // the helpers finish at about the caller's pace: poll briefly before sleeping on the cv
        const auto t0 = std::chrono::steady_clock::now();
        while (pending_left_.load(std::memory_order_acquire) != 0 &&
               std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(spin_us_)) {
        }
        std::unique_lock<std::mutex> lk(mu_);
        done_cv_.wait(lk, [&] { return pending_ == 0; });
        fn_ = nullptr;
        last_job_ns_.store(now_ns(), std::memory_order_release);
    }

private:
    PackPool() {
        // the process's CPU share, at most kMaxHelpers helpers: the gather is bound by each core's
        // memory bandwidth (round 4: 118k 48-B records took ~90 µs on 8 threads)
        size_t hw = std::max<unsigned>(std::thread::hardware_concurrency(), 1u);
        if (const char* e = std::getenv("OMP_NUM_THREADS")) hw = std::min<size_t>(hw, (size_t)std::max(1, std::atoi(e)));
        size_t cap = kMaxHelpers;
        const size_t helpers = std::min<size_t>(cap, hw > 1 ? hw - 1 : 0);
        for (size_t k = 0; k < helpers; ++k) workers_.emplace_back([this, k] { loop(k + 1); });
    }
    ~PackPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
    }
    void loop(size_t id) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(size_t, size_t)>* fn;
            size_t i0, i1;
            bool mine;
            {
                // a job soon after the last one (frames back to back) starts without a wake-up: a
                // helper polls up to spin_us_ only while jobs come in bursts (the last one ended
                // < kBurstNs ago), so an idle pool sleeps at once instead of holding cores
                const auto t0 = std::chrono::steady_clock::now();
                const bool burst = now_ns() - last_job_ns_.load(std::memory_order_acquire) < kBurstNs;
                while (burst && gen_seen_.load(std::memory_order_acquire) == seen &&
                       std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(spin_us_)) {
                }
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                mine = id < parts_;
                fn = fn_;
                i0 = std::min(n_, id * chunk_);
                i1 = std::min(n_, (id + 1) * chunk_);
            }
            if (!mine) continue;
            (*fn)(i0, i1);
            std::lock_guard<std::mutex> lk(mu_);
            pending_left_.fetch_sub(1, std::memory_order_release);
            if (--pending_ == 0) done_cv_.notify_one();
        }
    }
    std::vector<std::thread> workers_;
    std::mutex job_mu_, mu_;
    std::condition_variable cv_, done_cv_;
    const std::function<void(size_t, size_t)>* fn_ = nullptr;
    size_t n_ = 0, chunk_ = 0, parts_ = 0, pending_ = 0;
    static constexpr size_t kMaxHelpers = 15;
    std::atomic<uint64_t> gen_seen_{0};       // gen_, readable without the mutex (the helpers' poll)
    std::atomic<size_t> pending_left_{0};      // pending_, likewise (the caller's poll)
    static int64_t now_ns() {
        return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    static constexpr int64_t kBurstNs = 2000000;   // 2 ms
    std::atomic<int64_t> last_job_ns_{0};
    const pid_t pid_ = getpid();
    int spin_us_ = 200;
    uint64_t gen_ = 0;
    bool stop_ = false;
};
}  // namespace

// Pack a strided host cloud into SoA6 floats in pinned staging and upload asynchronously (no host
// wait: the staging buffer is reused only after its previous copy has run).  The reference's
// PointXYZINormal records (48 B: x y z pad | nx ny nz pad | intensity curvature pad pad, nrm =
// xyz + 4, stride 12 floats) take a record-at-a-time path (two 16-B loads per point).
int upload_soa6(imls_ctx* c, DevBuf& dst, const float* xyz, const float* nrm, size_t n, size_t stride, int which) {
    if (!xyz || !nrm || n == 0 || stride < 3) return fail(c, IMLS_ERR_ARG, "bad cloud pointer/size/stride");
    if (!c->ev_stage[which] && hipEventCreateWithFlags(&c->ev_stage[which], hipEventDisableTiming) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "hipEventCreate (staging)");
    if (hipEventSynchronize(c->ev_stage[which]) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "staging wait");
    if (c->stage_cap[which] < 6 * n) {
        if (c->h_stage[which]) (void)hipHostFree(c->h_stage[which]);
        c->h_stage[which] = nullptr;
        c->stage_cap[which] = 0;
        const size_t cap = 6 * n + 6 * n / 4 + 1024;
        if (hipHostMalloc((void**)&c->h_stage[which], cap * 4) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "hipHostMalloc (staging)");
        c->stage_cap[which] = cap;
    }
    float* h = c->h_stage[which];
    const bool rec48 = nrm == xyz + 4 && stride == 12 && (reinterpret_cast<uintptr_t>(xyz) & 15) == 0;
    const std::function<void(size_t, size_t)> pack = [=](size_t i0, size_t i1) {
        float *hx = h, *hy = h + n, *hz = h + 2 * n, *hnx = h + 3 * n, *hny = h + 4 * n, *hnz = h + 5 * n;
        if (rec48) {
            typedef float f4 __attribute__((ext_vector_type(4)));
            const f4* r = reinterpret_cast<const f4*>(xyz);
            for (size_t i = i0; i < i1; ++i) {
                const f4 p = r[3 * i], q = r[3 * i + 1];
                hx[i] = p.x; hy[i] = p.y; hz[i] = p.z;
                hnx[i] = q.x; hny[i] = q.y; hnz[i] = q.z;
            }
            return;
        }
        for (size_t i = i0; i < i1; ++i) {
            const float* p = xyz + i * stride;
            const float* q = nrm + i * stride;
            hx[i] = p[0]; hy[i] = p[1]; hz[i] = p[2];
            hnx[i] = q[0]; hny[i] = q[1]; hnz[i] = q[2];
        }
    };
    PackPool::get().run(n, n / 8192 + 1, pack);
    if (!grow(dst, 6 * n * 4)) return fail(c, IMLS_ERR_DEVICE, "hipMalloc (upload)");
    // the copy runs on the context's upload stream, not behind its running registrations: the
    // buffer's previous reader — the NaN filter of the last upload of this kind — has finished once a
    // build consumed its kept count (stage_pending false), else the copy is ordered after it on the
    // context's stream.  The context's stream waits for the copy (its filter reads the buffer).
    hipStream_t us = c->stream;
    if (!c->stage_pending[which]) {
        if (!c->ustream) {
            if (hipStreamCreateWithFlags(&c->ustream, hipStreamNonBlocking) != hipSuccess)
                return fail(c, IMLS_ERR_DEVICE, "hipStreamCreate (upload)");
            register_stream(c->ustream, c->device);
        }
        us = c->ustream;
    }
    if (hipMemcpyAsync(dst.p, h, 6 * n * 4, hipMemcpyHostToDevice, us) != hipSuccess ||
        hipEventRecord(c->ev_stage[which], us) != hipSuccess ||
        (us != c->stream && hipStreamWaitEvent(c->stream, c->ev_stage[which], 0) != hipSuccess))
        return fail(c, IMLS_ERR_DEVICE, "upload failed");
    c->stage_pending[which] = true;
    return IMLS_OK;
}

}  // namespace imlsgpu

extern "C" {

int imls_enable_stats(imls_ctx* c, int enable) {
    if (!c) return IMLS_ERR_ARG;
    c->collect_stats = enable != 0;
    return IMLS_OK;
}

int imls_enable_timing(imls_ctx* c, int enable) {
    if (!c || enable < 0 || enable > 2) return IMLS_ERR_ARG;
    c->timing = enable;
    return IMLS_OK;
}

int imls_timing_origin(imls_ctx* c) {
    if (!c) return IMLS_ERR_ARG;
    if (int rc = check_device(c)) return rc;
    if (c->device < 0 || c->device >= kMaxDevices) return fail(c, IMLS_ERR_ARG, "device index");
    std::lock_guard<std::mutex> lk(g_origin_mu);
    hipEvent_t& o = g_origin[c->device];
    if (!o && hipEventCreate(&o) != hipSuccess) return fail(c, IMLS_ERR_DEVICE, "hipEventCreate (origin)");
    if (hipEventRecord(o, c->stream) != hipSuccess || hipEventSynchronize(o) != hipSuccess)
        return fail(c, IMLS_ERR_DEVICE, "origin event");
    g_origin_set[c->device] = true;
    for (auto& v : c->iv) v.clear();
    return IMLS_OK;
}

int imls_timing_intervals(imls_ctx* c, int kernel, double* out, size_t cap, size_t* n) {
    if (!c || kernel < 0 || kernel >= kTimingKinds || !n) return IMLS_ERR_ARG;
    const auto& v = c->iv[kernel];
    *n = v.size();
    for (size_t k = 0; k < v.size() && k < cap && out; ++k) {
        out[2 * k] = v[k].first;
        out[2 * k + 1] = v[k].second;
    }
    return IMLS_OK;
}

int imls_kernel_timing(imls_ctx* c, int kernel, double* total_ms, uint64_t* launches) {
    if (!c || kernel < 0 || kernel >= kTimingKinds) return IMLS_ERR_ARG;
    if (total_ms) *total_ms = c->t_ms[kernel];
    if (launches) *launches = c->t_n[kernel];
    return IMLS_OK;
}

int imls_reset_timing(imls_ctx* c) {
    if (!c) return IMLS_ERR_ARG;
    for (int k = 0; k < kTimingKinds; ++k) { c->t_ms[k] = 0; c->t_n[k] = 0; c->ev_pairs[k].clear(); c->iv[k].clear(); }
    c->ev_used = 0;
    return IMLS_OK;
}

int imls_traversal_stats(imls_ctx* c, uint64_t out[8]) {
    if (!c || !out) return IMLS_ERR_ARG;
#ifdef IMLS_DEBUG_WAVE_TRACE
    constexpr int kOut = 16;   // debug build: the caller passes 16 slots
#else
    constexpr int kOut = 8;
#endif
    unsigned long long st[kOut] = {};
    if (c->stats.p) hipMemcpy(st, c->stats.p, sizeof(st), hipMemcpyDeviceToHost);
    for (int k = 0; k < kOut; ++k) out[k] = st[k];
    return IMLS_OK;
}

int imls_index_stats(imls_ctx* c, uint64_t out[8]) {
    if (!c || !out) return IMLS_ERR_ARG;
    if (int rc = ensure_built(c)) return rc;
    unsigned long long st[2] = {0, 0};
    if (c->stats.p) hipMemcpy(st, c->stats.p, 16, hipMemcpyDeviceToHost);
    out[0] = (uint64_t)c->M;
    out[1] = (uint64_t)((c->M + c->B - 1) / c->B);
    out[2] = (uint64_t)c->Pl;
    out[3] = (uint64_t)c->levels;
    out[4] = st[0];   // Σ k_q (neighbours returned to queries reaching the IMLS function)
    out[5] = st[1];   // queries whose NN-1 was found
    out[6] = (uint64_t)c->N;
    out[7] = (uint64_t)c->B;
    return IMLS_OK;
}

}  // extern "C"
