// sweep.hip — the upstream producer as one call on gfx950: a raw sweep to pcl_cloud (the filtered
// cloud) and pcl_surface_cloud (the flat cloud) without a host round trip of any cloud
// (laserCloudHandler, scan_registration.cpp:809-1503).
//
// The stages are the existing kernels on device buffers (front.hip, scanreg.hip, presample.hip,
// three_axis.hip, and sample.hip's k_major_avg / k_fps; deskew.hip's kernel after the front end once
// imls_sweep_set_motion gave a motion); this file adds what the host did between them:
//   k_sw_soa3        the sweep's records (any stride) → SoA xyz, the front end's input;
//   k_sw_flag / k_sw_scatter / k_sw_count   geometric-features candidates from the PCA flags, ascending;
//   k_sw_assemble    pcl_cloud: xyz / intensity / curvature gathered at the PCA's index + the normals,
//                    as SoA6 and side arrays, and as the float4 records k_major_avg reads next sweep;
//   k_sw_cbox        the 64-point chunk boxes of that cloud (one wave per chunk);
//   k_sw_bin         computeSphericalHistogram (536-564): the bin of every candidate; a radix sort by
//                    bin (stable: a bin lists its candidates in candidate order, as push_back does);
//   k_sw_boff / k_sw_fpts / k_sw_sub        bin offsets, the bins' points for k_fps, majorAxisSampling's
//                    per-bin subsets (656-664) for k_major_avg;
//   k_sw_plan        one block: the bin weights (666-723), k per bin (732 / 603), the FpsJob table with
//                    the glibc rand() replay in bin order, the output offsets;
//   k_sw_out         sampled_indices in bin order (all / FPS / random);
//   k_sw_pick, k_sw_ta_gather, k_sw_gather_flat, k_sw_pack   "random", three_axis' inputs, the flat
//                    cloud, and the 48-byte records of a download.
// randomSampling's shuffles are drawn on the host as POSITIONS (std::shuffle does not look at the
// contents) once the bin sizes are known — the one readback the sampler needs (two for major_axis
// with the "random" strategy, whose k per bin comes from the device).
// Arithmetic: the histogram's atan2 / asin are correctly rounded float / double values taken through
// fp64, the divisions in double, x86 truncation with INT_MIN for NaN; the weights' float
// sums run in the reference's order on one lane per bin.
// Roofline: every kernel here streams a few hundred KB once — launch-latency bound at one sweep.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <string>
#include <vector>

#include "internal.h"
#include "solve.h"

namespace imlsgpu {
namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr int kMaxBins = 4096;         // spherical-histogram bins the device sampler takes
constexpr int kCtlBins = 4;            // ctl words before the bin sizes: dropped, bad index, n_out, -

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
unsigned blocks_of(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// static_cast<int> as x86-64 evaluates it (cvttsd2si / cvttss2si): truncation, INT_MIN for NaN and
// out-of-range values
__device__ __forceinline__ int x86_d2i(double v) {
    if (!(v > -2147483649.0 && v < 2147483648.0)) return INT_MIN;
    return (int)v;
}
__device__ __forceinline__ int x86_f2i(float v) {
    return (v > -2147483904.0f && v < 2147483648.0f) ? (int)v : INT_MIN;
}

__global__ __launch_bounds__(kBlock) void k_sw_soa3(const float* __restrict__ raw, size_t stride, int n,
                                                    float* __restrict__ soa3) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float* r = raw + (size_t)i * stride;
    soa3[i] = r[0];
    soa3[(size_t)n + i] = r[1];
    soa3[2 * (size_t)n + i] = r[2];
}

__global__ __launch_bounds__(kBlock) void k_sw_flag(const unsigned char* __restrict__ fl, int rows, unsigned* __restrict__ keep) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r < rows) keep[r] = (fl[r] & IMLS_PCA_CANDIDATE) ? 1u : 0u;
}
__global__ __launch_bounds__(kBlock) void k_sw_scatter(const unsigned* __restrict__ keep, const unsigned* __restrict__ pos,
                                                       int rows, int* __restrict__ cand) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r < rows && keep[r]) cand[pos[r]] = r;
}
__global__ void k_sw_count(const unsigned* __restrict__ keep, const unsigned* __restrict__ pos, int rows, int* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = rows > 0 ? (int)(pos[rows - 1] + keep[rows - 1]) : 0;
}

// pcl_cloud row r = laserCloud point index[r] (1210-1220) with the PCA's normal
__global__ __launch_bounds__(kBlock) void k_sw_assemble(const float4* __restrict__ cloud, const unsigned* __restrict__ index,
                                                        const float* __restrict__ nrm, const float* __restrict__ curv,
                                                        int rows, float* __restrict__ soa6, float* __restrict__ inten,
                                                        float* __restrict__ curv_out, float4* __restrict__ prev4) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= rows) return;
    const unsigned i = index[r];
    const float4 q = cloud[i];
    const size_t R = (size_t)rows;
    soa6[r] = q.x;
    soa6[R + r] = q.y;
    soa6[2 * R + r] = q.z;
    soa6[3 * R + r] = nrm[3 * (size_t)r];
    soa6[4 * R + r] = nrm[3 * (size_t)r + 1];
    soa6[5 * R + r] = nrm[3 * (size_t)r + 2];
    inten[r] = q.w;
    curv_out[r] = curv ? curv[i] : 0.f;
    prev4[r] = make_float4(q.x, q.y, q.z, 0.f);
}

__global__ __launch_bounds__(kBlock) void k_sw_p4(const float* __restrict__ soa, size_t stride, int m, float4* __restrict__ p4) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j < m) p4[j] = make_float4(soa[j], soa[stride + j], soa[2 * stride + j], 0.f);
}

// AABB of chunk blockIdx.x (64 points, one wave); a non-finite coordinate makes the box unbounded:
// the chunk is always scanned
__global__ __launch_bounds__(64) void k_sw_cbox(const float4* __restrict__ p4, int m, float4* __restrict__ cbox) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    float lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
    bool bad = false;
    if (j < m) {
        const float4 q = p4[j];
        bad = !(isfinite(q.x) && isfinite(q.y) && isfinite(q.z));
        if (!bad) { lx = hx = q.x; ly = hy = q.y; lz = hz = q.z; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lx = fminf(lx, __shfl_xor(lx, o)); ly = fminf(ly, __shfl_xor(ly, o)); lz = fminf(lz, __shfl_xor(lz, o));
        hx = fmaxf(hx, __shfl_xor(hx, o)); hy = fmaxf(hy, __shfl_xor(hy, o)); hz = fmaxf(hz, __shfl_xor(hz, o));
    }
    const bool any_bad = __ballot(bad) != 0ull;
    if (threadIdx.x == 0) {
        if (any_bad) { lx = ly = lz = -INFINITY; hx = hy = hz = INFINITY; }
        cbox[2 * (size_t)blockIdx.x] = make_float4(lx, ly, lz, 0.f);
        cbox[2 * (size_t)blockIdx.x + 1] = make_float4(hx, hy, hz, 0.f);
    }
}

// computeSphericalHistogram (536-564): key = the candidate's bin, or NB for a candidate left out
__global__ __launch_bounds__(kBlock) void k_sw_bin(const float* __restrict__ soa6, int n, const int* __restrict__ cand, int nc,
                                                   int AZ, int EL, unsigned* __restrict__ keys, int* __restrict__ vals,
                                                   int* __restrict__ ctl) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= nc) return;
    const int idx = cand[k];
    unsigned key = (unsigned)(AZ * EL);
    if (idx < 0 || idx >= n) {
        atomicOr(&ctl[1], 1);
    } else {
        const size_t N = (size_t)n;
        const float nx = soa6[3 * N + idx], ny = soa6[4 * N + idx], nz = soa6[5 * N + idx];
        float azimuth = (float)atan2((double)ny, (double)nx);       // std::atan2(float, float), correctly rounded
        float elevation = (float)asin((double)nz);                  // ::asin(double) rounded to float
        if (azimuth < 0) azimuth = (float)((double)azimuth + 2 * kPi);
        elevation = (float)((double)elevation + kPi / 2);
        const int ai = min(x86_d2i((double)azimuth / (2 * kPi / AZ)), AZ - 1);
        const int ei = min(x86_d2i((double)elevation / (kPi / EL)), EL - 1);
        if (ai < 0 || ei < 0) {
            atomicAdd(&ctl[0], 1);                                  // no bin: left out and counted
        } else {
            key = (unsigned)(ai * EL + ei);
            atomicAdd(&ctl[kCtlBins + key], 1);
        }
    }
    keys[k] = key;
    vals[k] = idx;
}

__global__ void k_sw_boff(const int* __restrict__ binsz, int NB, int* __restrict__ boff) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int o = 0;
    for (int b = 0; b < NB; ++b) { boff[b] = o; o += binsz[b]; }
    boff[NB] = o;
}

// the binned candidates' points in bin order (k_fps' packed bin clouds)
__global__ __launch_bounds__(kBlock) void k_sw_fpts(const float* __restrict__ soa6, int n, const int* __restrict__ binlist,
                                                    const int* __restrict__ boff, int NB, float4* __restrict__ fpts) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= boff[NB]) return;
    const int i = binlist[j];
    const size_t N = (size_t)n;
    fpts[j] = make_float4(soa6[i], soa6[N + i], soa6[2 * N + i], 0.f);
}

struct SubDesc {
    int off, len, shuf;   // subset rows [off, off+len) of the bin; shuf ≥ 0: positions shuf1[shuf + t], else t
};

// majorAxisSampling's per-bin subsets (656-664) as k_major_avg's sample records
__global__ __launch_bounds__(kBlock) void k_sw_sub(const SubDesc* __restrict__ desc, const int* __restrict__ boff,
                                                   const int* __restrict__ binlist, const int* __restrict__ shuf1,
                                                   const float* __restrict__ soa6, int n, float4* __restrict__ spt,
                                                   float4* __restrict__ snr) {
    const SubDesc d = desc[blockIdx.x];
    const int b0 = boff[blockIdx.x];
    const size_t N = (size_t)n;
    for (int t = threadIdx.x; t < d.len; t += kBlock) {
        const int i = binlist[b0 + (d.shuf >= 0 ? shuf1[d.shuf + t] : t)];
        spt[d.off + t] = make_float4(soa6[i], soa6[N + i], soa6[2 * N + i], 0.f);
        snr[d.off + t] = make_float4(soa6[3 * N + i], soa6[4 * N + i], soa6[5 * N + i], 0.f);
    }
}

// a / b as x86 divss returns it, NaN results included: an invalid quotient (0/0, ∞/∞) is the default
// NaN 0xFFC00000 and a NaN operand is passed on (the first one, quieted) — the weights are compared
// as bit patterns
__device__ __forceinline__ float div_x86(float a, float b) {
    if (a != a) return __uint_as_float(__float_as_uint(a) | 0x00400000u);
    if (b != b) return __uint_as_float(__float_as_uint(b) | 0x00400000u);
    if ((a == 0.f && b == 0.f) || (isinf(a) && isinf(b))) return __uint_as_float(0xFFC00000u);
    return __fdiv_rn(a, b);
}

// glibc random() TYPE_3 step (the state ransac_seed_host produces)
__device__ __forceinline__ int rand_next(int* st) {
    unsigned* ring = reinterpret_cast<unsigned*>(st);
    const int f = st[31], r = st[32];
    ring[f] += ring[r];
    const int out = (int)(ring[f] >> 1);
    st[31] = (f + 1) % 31;
    st[32] = (r + 1) % 31;
    return out;
}

// The per-bin decisions (one block).  kind: −1 skipped, 0 all, 1 FPS, 2 random; kk: FPS count / the
// random strategy's k; out_off: start of the bin's output, out_off[NB] = the total (also ctl[2]).
__global__ __launch_bounds__(kBlock) void k_sw_plan(imls_sample_params p, int NB, const int* __restrict__ binsz,
                                                    const int* __restrict__ boff, const SubDesc* __restrict__ desc,
                                                    const int* __restrict__ cnt, const float* __restrict__ avg, int have_avg,
                                                    int* __restrict__ rng, float* __restrict__ w, int* __restrict__ kind,
                                                    int* __restrict__ kk, int* __restrict__ out_off,
                                                    FpsJob* __restrict__ jobs, int* __restrict__ ctl) {
    __shared__ float s_tw;
    const bool major = p.method == IMLS_SAMPLE_MAJOR_AXIS;
    for (int b = threadIdx.x; b < NB; b += kBlock) {               // 666-711, one lane per bin
        float wb = 0.0f;
        if (major && binsz[b] >= p.min_points_per_bin && have_avg) {
            const SubDesc d = desc[b];
            int valid = 0;
            float total = 0.0f;
            for (int t = d.off; t < d.off + d.len; ++t)
                if (cnt[t] >= 3) { total = __fadd_rn(total, avg[t]); valid++; }
            if (valid >= 3) wb = __fdiv_rn(total, (float)valid);
        }
        w[b] = wb;
    }
    __syncthreads();
    if (major) {                                                    // 715-723
        if (threadIdx.x == 0) {
            float tw = 0.0f;
            for (int b = 0; b < NB; ++b) tw = __fadd_rn(tw, w[b]);
            s_tw = tw;
        }
        __syncthreads();
        for (int b = threadIdx.x; b < NB; b += kBlock) w[b] = div_x86(w[b], s_tw);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    int st[34];
    for (int i = 0; i < 34; ++i) st[i] = rng[i];
    int o = 0;
    for (int b = 0; b < NB; ++b) {                                  // bin order: the rand() stream's order
        const int sz = binsz[b];
        int kd = -1, k = 0, n_out = 0;
        FpsJob J{0, 0, 0, 0, 0};
        if (sz >= p.min_points_per_bin && sz > 0) {
            k = major ? min(x86_f2i(__fmul_rn(w[b], (float)p.max_total_points)), sz) : p.max_points_per_bin;   // 732 / 603
            if (sz <= k) {
                kd = 0;
                n_out = sz;
            } else if (p.sampling_strategy == 0) {
                k = max(k, 1);               // farthestPointSampling pushes its first index even for k ≤ 0 (49-50)
                J = FpsJob{boff[b], sz, k, rand_next(st) % sz, o};
                kd = 1;
                n_out = k;
            } else {
                kd = 2;
                n_out = max(k, 0);
            }
        }
        kind[b] = kd;
        kk[b] = k;
        out_off[b] = o;
        jobs[b] = J;
        o += n_out;
    }
    out_off[NB] = o;
    ctl[2] = o;
}

__global__ __launch_bounds__(kBlock) void k_sw_out(const int* __restrict__ kind, const int* __restrict__ out_off,
                                                   const int* __restrict__ boff, const int* __restrict__ binlist,
                                                   const int* __restrict__ fres, const int* __restrict__ s2off,
                                                   const int* __restrict__ shuf2, int* __restrict__ sampled) {
    const int b = blockIdx.x, kd = kind[b];
    if (kd < 0) return;
    const int o = out_off[b], cnt = out_off[b + 1] - o, b0 = boff[b];
    for (int t = threadIdx.x; t < cnt; t += kBlock) {
        int pos = t;
        if (kd == 1) pos = fres[o + t];
        else if (kd == 2) pos = shuf2[s2off[b] + t];
        sampled[o + t] = binlist[b0 + pos];
    }
}

__global__ __launch_bounds__(kBlock) void k_sw_pick(const int* __restrict__ cand, const int* __restrict__ pos, int cnt,
                                                    int* __restrict__ rows) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t < cnt) rows[t] = cand[pos[t]];
}

// k_ta_keys' inputs: (x, y, z, λ1), (nx, ny, nz, λ2), (λ3, bits(idx)) of candidate k
__global__ __launch_bounds__(kBlock) void k_sw_ta_gather(const float* __restrict__ soa6, int n, const float* __restrict__ ev,
                                                         const int* __restrict__ cand, int nc, float4* __restrict__ ga,
                                                         float4* __restrict__ gb, float2* __restrict__ gc) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= nc) return;
    const int i = cand[k];
    const size_t N = (size_t)n;
    ga[k] = make_float4(soa6[i], soa6[N + i], soa6[2 * N + i], ev[3 * (size_t)i]);
    gb[k] = make_float4(soa6[3 * N + i], soa6[4 * N + i], soa6[5 * N + i], ev[3 * (size_t)i + 1]);
    gc[k] = make_float2(ev[3 * (size_t)i + 2], __int_as_float(i));
}

// pcl_surface_cloud = pcl_cloud[sampled rows] as SoA6 of its own length (d_nout, or nout when null)
__global__ __launch_bounds__(kBlock) void k_sw_gather_flat(const float* __restrict__ soa6, int rows, const int* __restrict__ sampled,
                                                           const int* __restrict__ d_nout, int nout, float* __restrict__ flat) {
    const int cnt = d_nout ? *d_nout : nout;
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= cnt) return;
    const int r = sampled[t];
#pragma unroll
    for (int c = 0; c < 6; ++c) flat[(size_t)c * cnt + t] = soa6[(size_t)c * rows + r];
}

// 48-byte pcl::PointXYZINormal records (imls_wire.hpp): x y z 0 | nx ny nz 0 | intensity curvature 0 0
__global__ __launch_bounds__(kBlock) void k_sw_pack(const float* __restrict__ soa6, int rows, const float* __restrict__ inten,
                                                    const float* __restrict__ curv, const int* __restrict__ pick, int cnt,
                                                    float4* __restrict__ rec) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= cnt) return;
    const int r = pick ? pick[t] : t;
    const size_t R = (size_t)rows;
    rec[3 * (size_t)t] = make_float4(soa6[r], soa6[R + r], soa6[2 * R + r], 0.f);
    rec[3 * (size_t)t + 1] = make_float4(soa6[3 * R + r], soa6[4 * R + r], soa6[5 * R + r], 0.f);
    rec[3 * (size_t)t + 2] = make_float4(inten[r], curv[r], 0.f, 0.f);
}

// events around a group of kernels, harvested by the caller as `kind`
struct Span {
    hipStream_t s;
    hipEvent_t ev[2];
    bool on;
    Span(SweepEnv& e, int kind) : s(e.s) {
        on = e.mark && e.mark(e.owner, kind, ev);
        if (on) (void)hipEventRecord(ev[0], s);
    }
    ~Span() {
        if (on) (void)hipEventRecord(ev[1], s);
    }
};

bool grow(DevBuf& b, size_t bytes) { return devbuf_grow(b, std::max<size_t>(bytes, 256), std::max<size_t>(bytes, 256) + bytes / 4); }

int dev_fail(SweepEnv& e, const char* what) {
    *e.err = what;
    return IMLS_ERR_DEVICE;
}

struct SamplerOut {
    const int* d_nout;                 // device word: sampled rows written
    const float* d_w;                  // device [NB]: the normalised major_axis weights (0 for "normal")
    uint64_t dropped;                  // candidates without a bin
    // host tables of the uploads enqueued by sampler_dev: kept until the caller's wait
    std::vector<SubDesc> hdesc;
    std::vector<int> hs1, hs2, hs2off;
    int hrng[34];
};

int check_sample_params(SweepEnv& e, const imls_sample_params& p) {
    if (p.method < 0 || p.method > 1 || p.azimuth_bins <= 0 || p.elevation_bins <= 0 || p.azimuth_bins > 1024 ||
        p.elevation_bins > 1024 || p.sampling_strategy < 0 || p.sampling_strategy > 1) {
        *e.err = "bad sample method / bins / strategy";
        return IMLS_ERR_ARG;
    }
    if ((long long)p.azimuth_bins * p.elevation_bins > kMaxBins) {
        *e.err = "device sampler: at most 4096 histogram bins";
        return IMLS_ERR_UNSUPPORTED;
    }
    return IMLS_OK;
}

// samplePointCloud "normal" / "major_axis" on device buffers.  Everything is enqueued on e.s; the
// host waits once for the bin sizes (twice for major_axis + "random").  d_sampled: capacity nc + NB.
int sampler_dev(SweepEnv& e, DevBuf& scratch, const imls_sample_params& p, const float* soa6, int n, const int* cand, int nc,
                const float4* last4, const float4* cbox, int m, int* d_sampled, SamplerOut* out, Xfer& x) {
    if (int rc = check_sample_params(e, p)) return rc;
    hipStream_t s = e.s;
    const int AZ = p.azimuth_bins, EL = p.elevation_bins, NB = AZ * EL;
    const bool major = p.method == IMLS_SAMPLE_MAJOR_AXIS;
    int key_bits = 1;
    while ((1 << key_bits) <= NB) key_bits++;
    const size_t c1 = (size_t)std::max(nc, 1);
    size_t cub_bytes = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, cub_bytes, (unsigned*)nullptr, (unsigned*)nullptr, (int*)nullptr,
                                           (int*)nullptr, (int)c1, 0, key_bits, s) != hipSuccess)
        return dev_fail(e, "hipcub sort size query failed");
    size_t total = 0;
    {
        const size_t parts[] = {c1 * 4, c1 * 4, c1 * 4, c1 * 4, cub_bytes, (size_t)(kCtlBins + NB) * 4, (size_t)(NB + 1) * 4,
                                (size_t)NB * sizeof(SubDesc), c1 * 4, (size_t)NB * 4, (c1 + 1) * 4, 34 * 4, c1 * 16, c1 * 16,
                                c1 * 4, c1 * 4, (size_t)NB * 4, (size_t)NB * 4, (size_t)NB * 4, (size_t)(NB + 1) * 4,
                                (size_t)NB * sizeof(FpsJob), c1 * 16, c1 * 8, c1, (c1 + NB) * 4};
        for (size_t b : parts) total += al256(b);
    }
    if (!grow(scratch, total)) return dev_fail(e, "hipMalloc (sampler scratch)");
    char* q = (char*)scratch.p;
    unsigned* keys = carve<unsigned>(q, c1);
    unsigned* keys2 = carve<unsigned>(q, c1);
    int* vals = carve<int>(q, c1);
    int* binlist = carve<int>(q, c1);
    void* cub_tmp = carve<char>(q, cub_bytes);
    int* ctl = carve<int>(q, kCtlBins + NB);
    int* boff = carve<int>(q, NB + 1);
    SubDesc* desc = carve<SubDesc>(q, NB);
    int* shuf1 = carve<int>(q, c1);
    int* s2off = carve<int>(q, NB);
    int* shuf2 = carve<int>(q, c1 + 1);
    int* rng = carve<int>(q, 34);
    float4* spt = carve<float4>(q, c1);
    float4* snr = carve<float4>(q, c1);
    int* cnt = carve<int>(q, c1);
    float* avg = carve<float>(q, c1);
    float* w = carve<float>(q, NB);
    int* kind = carve<int>(q, NB);
    int* kk = carve<int>(q, NB);
    int* out_off = carve<int>(q, NB + 1);
    FpsJob* jobs = carve<FpsJob>(q, NB);
    float4* fpts = carve<float4>(q, c1);
    double* md = carve<double>(q, c1);
    unsigned char* taken = carve<unsigned char>(q, c1);
    int* fres = carve<int>(q, c1 + NB);

    std::vector<int> hctl(kCtlBins + NB, 0);
    {
        Span sp(e, kTimeSweep);
        if (hipMemsetAsync(ctl, 0, (size_t)(kCtlBins + NB) * 4, s) != hipSuccess) return dev_fail(e, "sampler memset failed");
        if (nc > 0) {
            k_sw_bin<<<blocks_of(nc), kBlock, 0, s>>>(soa6, n, cand, nc, AZ, EL, keys, vals, ctl);
            hipcub::DeviceRadixSort::SortPairs(cub_tmp, cub_bytes, keys, keys2, vals, binlist, nc, 0, key_bits, s);
        }
        k_sw_boff<<<1, 64, 0, s>>>(ctl + kCtlBins, NB, boff);
        if (nc > 0 && p.sampling_strategy == 0) k_sw_fpts<<<blocks_of(nc), kBlock, 0, s>>>(soa6, n, binlist, boff, NB, fpts);
    }
    if (hipGetLastError() != hipSuccess) return dev_fail(e, "sampler launch failed");
    bool ok = hipMemcpyAsync(hctl.data(), ctl, hctl.size() * 4, hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) return dev_fail(e, "sampler histogram failed");
    x.d2h += hctl.size() * 4;
    x.syncs += 1;
    if (hctl[1]) { *e.err = "candidate index out of range"; return IMLS_ERR_ARG; }
    out->dropped = (uint64_t)hctl[0];
    const int* binsz = hctl.data() + kCtlBins;

    // randomSampling's shuffles as positions, in the host path's order of shuffle_take calls
    uint32_t calls = 0;
    int* hrng = out->hrng;
    ransac_seed_host(p.rand_seed, hrng);
    std::vector<SubDesc>& hdesc = out->hdesc;
    std::vector<int>&hs1 = out->hs1, &hs2 = out->hs2, &hs2off = out->hs2off;
    hdesc.assign(NB, SubDesc{0, 0, -1});
    hs1.clear();
    hs2.clear();
    hs2off.assign(NB, 0);
    int ns = 0;
    if (major) {
        for (int b = 0; b < NB; ++b) {                                 // 656-664
            const int sz = binsz[b];
            hdesc[b].off = ns;
            if (sz >= p.min_points_per_bin) {
                if (sz > p.max_points_per_bin) {
                    hdesc[b].shuf = (int)hs1.size();
                    shuffle_positions(p.shuffle_seed + calls++, sz, p.max_points_per_bin, hs1);
                    hdesc[b].len = (int)hs1.size() - hdesc[b].shuf;
                } else {
                    hdesc[b].len = sz;
                }
            }
            ns += hdesc[b].len;
        }
    }
    ok = hipMemcpyAsync(rng, hrng, 34 * 4, hipMemcpyHostToDevice, s) == hipSuccess;
    ok = ok && hipMemcpyAsync(desc, hdesc.data(), (size_t)NB * sizeof(SubDesc), hipMemcpyHostToDevice, s) == hipSuccess;
    x.h2d += 34 * 4 + (size_t)NB * sizeof(SubDesc);
    if (!hs1.empty()) {
        ok = ok && hipMemcpyAsync(shuf1, hs1.data(), hs1.size() * 4, hipMemcpyHostToDevice, s) == hipSuccess;
        x.h2d += hs1.size() * 4;
    }
    if (!ok) return dev_fail(e, "sampler table upload failed");
    const int have_avg = major && ns > 0 && m > 0;
    if (have_avg) {
        {
            Span sp(e, kTimeSweep);
            k_sw_sub<<<(unsigned)NB, kBlock, 0, s>>>(desc, boff, binlist, shuf1, soa6, n, spt, snr);
        }
        Span sp(e, kTimeMajorAvg);
        launch_major_avg(s, spt, snr, ns, last4, m, cbox, p.r, p.r_proj, cnt, avg);
    }
    {
        Span sp(e, kTimeSweep);
        k_sw_plan<<<1, kBlock, 0, s>>>(p, NB, ctl + kCtlBins, boff, desc, cnt, avg, have_avg, rng, w, kind, kk, out_off, jobs, ctl);
    }
    if (hipGetLastError() != hipSuccess) return dev_fail(e, "sampler launch failed");
    if (p.sampling_strategy == 1) {
        if (major) {                      // k per bin comes from the device's weights: one more readback
            std::vector<int> hk(2 * (size_t)NB);
            ok = hipMemcpyAsync(hk.data(), kind, (size_t)NB * 4, hipMemcpyDeviceToHost, s) == hipSuccess;
            ok = ok && hipMemcpyAsync(hk.data() + NB, kk, (size_t)NB * 4, hipMemcpyDeviceToHost, s) == hipSuccess;
            ok = ok && hipStreamSynchronize(s) == hipSuccess;
            if (!ok) return dev_fail(e, "sampler plan failed");
            x.d2h += 2 * (size_t)NB * 4;
            x.syncs += 1;
            for (int b = 0; b < NB; ++b) {
                if (hk[b] != 2) continue;
                hs2off[b] = (int)hs2.size();
                shuffle_positions(p.shuffle_seed + calls++, binsz[b], hk[NB + b], hs2);
            }
        } else {
            for (int b = 0; b < NB; ++b) {                             // 603-612
                const int sz = binsz[b];
                if (sz < p.min_points_per_bin || sz <= 0 || sz <= p.max_points_per_bin) continue;
                hs2off[b] = (int)hs2.size();
                shuffle_positions(p.shuffle_seed + calls++, sz, p.max_points_per_bin, hs2);
            }
        }
        ok = hipMemcpyAsync(s2off, hs2off.data(), (size_t)NB * 4, hipMemcpyHostToDevice, s) == hipSuccess;
        x.h2d += (size_t)NB * 4;
        if (!hs2.empty()) {
            ok = ok && hipMemcpyAsync(shuf2, hs2.data(), hs2.size() * 4, hipMemcpyHostToDevice, s) == hipSuccess;
            x.h2d += hs2.size() * 4;
        }
        if (!ok) return dev_fail(e, "sampler table upload failed");
    }
    {
        Span sp(e, kTimeSweep);
        if (p.sampling_strategy == 0 && nc > 0) launch_fps(s, fpts, jobs, NB, md, taken, fres);
        k_sw_out<<<(unsigned)NB, kBlock, 0, s>>>(kind, out_off, boff, binlist, fres, s2off, shuf2, d_sampled);
    }
    if (hipGetLastError() != hipSuccess) return dev_fail(e, "sampler launch failed");
    out->d_nout = ctl + 2;
    out->d_w = w;
    return IMLS_OK;
}

// the previous cloud's float4 records → chunk boxes
void enqueue_cbox(hipStream_t s, const float4* p4, int m, float4* cbox) {
    if (m > 0) k_sw_cbox<<<(unsigned)((m + 63) / 64), 64, 0, s>>>(p4, m, cbox);
}

}  // namespace

std::vector<DevBuf*> sweep_buffers(SweepState& st) {
    std::vector<DevBuf*> v = {&st.raw, &st.raw3, &st.cand, &st.scratch, &st.rec};
    for (auto& S : st.set)
        for (DevBuf* b : {&S.soa6, &S.side, &S.flat, &S.rows, &S.prev4, &S.cbox}) v.push_back(b);
    return v;
}

int sampler_run(SweepEnv& e, SweepState& st, const imls_sample_params& p, const float* d_soa6, size_t n, const int32_t* d_cand,
                size_t n_cand, const float* d_last_soa6, size_t m, int32_t* d_sampled, size_t* n_sampled, float* d_weights,
                uint64_t* nan_normals) {
    hipStream_t s = e.s;
    Xfer x;
    const bool major = p.method == IMLS_SAMPLE_MAJOR_AXIS;
    const size_t mm = major ? m : 0, nch = (mm + 63) / 64;
    float4 *p4 = nullptr, *cbox = nullptr;
    if (mm > 0) {
        if (!grow(st.rec, al256(mm * 16) + nch * 32)) return dev_fail(e, "hipMalloc (previous cloud)");
        p4 = (float4*)st.rec.p;
        cbox = (float4*)((char*)st.rec.p + al256(mm * 16));
        Span sp(e, kTimeSweep);
        k_sw_p4<<<blocks_of(mm), kBlock, 0, s>>>(d_last_soa6, m, (int)mm, p4);
        enqueue_cbox(s, p4, (int)mm, cbox);
    }
    SamplerOut so{};
    if (int rc = sampler_dev(e, st.scratch, p, d_soa6, (int)n, d_cand, (int)n_cand, p4, cbox, (int)mm, d_sampled, &so, x))
        return rc;
    int nout = 0;
    const int NB = p.azimuth_bins * p.elevation_bins;
    bool ok = hipMemcpyAsync(&nout, so.d_nout, 4, hipMemcpyDeviceToHost, s) == hipSuccess;
    if (d_weights) ok = ok && hipMemcpyAsync(d_weights, so.d_w, (size_t)NB * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) return dev_fail(e, "sampler failed");
    if (n_sampled) *n_sampled = (size_t)nout;
    if (nan_normals) *nan_normals = so.dropped;
    return IMLS_OK;
}

int sweep_run(SweepEnv& e, SweepState& st, const imls_sweep_params& p, const float* h_xyz, const float* d_xyz, size_t stride,
              size_t n, imls_sweep_info* info) {
    hipStream_t s = e.s;
    Xfer x;
    imls_sweep_info I{};
    I.sweep = st.counter;
    I.n_input = n;
    const int nxt = st.has ? 1 - st.cur : 0;
    SweepSet& S = st.set[nxt];
    const SweepSet* prev = st.has ? &st.set[st.cur] : nullptr;
    S.n_filtered = S.n_flat = S.cap_filtered = 0;

    // front end
    size_t m = 0;
    FrontDev fo{};
    int32_t ring_sizes[64];
    const float* raw3 = nullptr;
    if (n > 0 && n <= (size_t)0x3fffffff) {
        const float* raw = d_xyz;
        if (h_xyz) {
            if (!grow(st.raw, n * stride * 4)) return dev_fail(e, "hipMalloc (sweep upload)");
            if (hipMemcpyAsync(st.raw.p, h_xyz, n * stride * 4, hipMemcpyHostToDevice, s) != hipSuccess)
                return dev_fail(e, "sweep upload failed");
            x.h2d += n * stride * 4;
            raw = (const float*)st.raw.p;
        }
        if (!grow(st.raw3, n * 12)) return dev_fail(e, "hipMalloc (sweep SoA)");
        Span sp(e, kTimeSweep);
        k_sw_soa3<<<blocks_of(n), kBlock, 0, s>>>(raw, stride, (int)n, (float*)st.raw3.p);
        raw3 = (const float*)st.raw3.p;
    }
    {
        Span sp(e, kTimeFrontEnd);
        if (int rc = front_end_dev(s, p.front, raw3, nullptr, n, *e.front_mem, &fo, ring_sizes, &m, *e.err, &x)) return rc;
    }
    I.n_front = m;
    // deskew (imls_sweep_set_motion): the front end's records in place, relTime read from their
    // intensity; everything after this sees the compensated points
    if (st.deskew_on && m > 0) {
        Span sp(e, kTimeDeskew);
        deskew_enqueue(s, st.deskew, p.front.scan_period, const_cast<float4*>(fo.out), nullptr, m);
    }

    // ring PCA
    PcaDev po{};
    uint64_t pc[2] = {0, 0};
    if (m > 0) {
        hipEvent_t mk[2];
        const bool timed = e.mark && e.mark(e.owner, kTimeRingPca, mk);
        if (int rc = ring_pca_dev(s, p.pca, fo.out, nullptr, ring_sizes, p.front.n_scans, *e.pca_mem, timed ? mk : nullptr, &po,
                                  pc, *e.err, &x))
            return rc;
    }
    I.pca_failure = pc[0];
    I.plane_invalid = pc[1];
    const int rows = (int)po.rows;
    I.n_filtered = po.rows;

    int n_cand = 0, n_flat = 0;
    if (rows > 0) {
        const size_t R = (size_t)rows, nch = (R + 63) / 64;
        if (!grow(S.soa6, R * 24) || !grow(S.side, R * 8) || !grow(S.prev4, R * 16) || !grow(S.cbox, nch * 32) ||
            !grow(st.cand, al256(R * 4) + 256))
            return dev_fail(e, "hipMalloc (sweep clouds)");
        int* cand = (int*)st.cand.p;
        int* d_ncand = (int*)((char*)st.cand.p + al256(R * 4));
        float* inten = (float*)S.side.p;
        float* curv_rows = inten + R;
        // presample: candidates ascending
        size_t cub_bytes = 0;
        if (hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, (unsigned*)nullptr, (unsigned*)nullptr, rows, s) != hipSuccess)
            return dev_fail(e, "hipcub scan size query failed");
        const size_t need = al256((size_t)m * 4) + 2 * al256(R * 4) + al256(cub_bytes);
        if (!grow(st.scratch, need)) return dev_fail(e, "hipMalloc (presample scratch)");
        char* q = (char*)st.scratch.p;
        float* curv = carve<float>(q, m);
        unsigned* keep = carve<unsigned>(q, R);
        unsigned* pos = carve<unsigned>(q, R);
        void* cub_tmp = carve<char>(q, cub_bytes);
        const bool curvature = p.presample_method == IMLS_PRESAMPLE_CURVATURE;
        if (curvature) {
            Span sp(e, kTimeCurvature);
            curvature_enqueue(s, p.curvature, fo.out, po.ring_off, p.front.n_scans, (int)m, po.idx, po.fl, rows, curv, keep, pos,
                              cand, cub_tmp, cub_bytes);
        }
        {
            Span sp(e, kTimeSweep);
            if (!curvature) {
                k_sw_flag<<<blocks_of(R), kBlock, 0, s>>>(po.fl, rows, keep);
                hipcub::DeviceScan::ExclusiveSum(cub_tmp, cub_bytes, keep, pos, rows, s);
                k_sw_scatter<<<blocks_of(R), kBlock, 0, s>>>(keep, pos, rows, cand);
            }
            k_sw_count<<<1, 64, 0, s>>>(keep, pos, rows, d_ncand);
            k_sw_assemble<<<blocks_of(R), kBlock, 0, s>>>(fo.out, po.idx, po.nrm, curvature ? curv : nullptr, rows,
                                                         (float*)S.soa6.p, inten, curv_rows, (float4*)S.prev4.p);
            enqueue_cbox(s, (const float4*)S.prev4.p, rows, (float4*)S.cbox.p);
        }
        if (hipGetLastError() != hipSuccess) return dev_fail(e, "sweep launch failed");
        bool ok = hipMemcpyAsync(&n_cand, d_ncand, 4, hipMemcpyDeviceToHost, s) == hipSuccess;
        ok = ok && hipStreamSynchronize(s) == hipSuccess;
        if (!ok) return dev_fail(e, "sweep presample failed");
        x.d2h += 4;
        x.syncs += 1;
        S.cap_filtered = R;

        // sampling → the sampled rows of pcl_cloud
        const int* d_nout = nullptr;
        unsigned long long* d_nan = nullptr;
        SamplerOut so{};                 // (holds the host tables of its uploads until the wait below)
        std::vector<int> hp;
        int cap_flat = 0;
        if (p.sample_method == IMLS_SWEEP_THREE_AXIS) {
            const int k = std::min(p.points_per_list, n_cand);
            n_flat = 9 * k;
            cap_flat = n_flat;
            if (n_cand > 0) {
                const size_t C = (size_t)n_cand;
                const size_t tneed = 2 * al256(C * 16) + al256(C * 8) + al256(9 * C * 8) + 256;
                if (!grow(st.scratch, tneed) || !grow(S.rows, (size_t)n_flat * 4)) return dev_fail(e, "hipMalloc (three_axis)");
                char* t = (char*)st.scratch.p;
                float4* ga = carve<float4>(t, C);
                float4* gb = carve<float4>(t, C);
                float2* gc = carve<float2>(t, C);
                unsigned long long* keys = carve<unsigned long long>(t, 9 * C);
                d_nan = carve<unsigned long long>(t, 1);
                if (hipMemsetAsync(d_nan, 0, 8, s) != hipSuccess) return dev_fail(e, "three_axis memset failed");
                {
                    Span sp(e, kTimeSweep);
                    k_sw_ta_gather<<<blocks_of(C), kBlock, 0, s>>>((const float*)S.soa6.p, rows, po.ev, cand, n_cand, ga, gb, gc);
                }
                Span sp(e, kTimeThreeAxis);
                three_axis_enqueue(s, ga, gb, gc, n_cand, k, keys, (int*)S.rows.p, d_nan);
            }
        } else if (p.sample_method == IMLS_SWEEP_RANDOM) {
            shuffle_positions(p.shuffle_seed, n_cand, p.max_points, hp);
            n_flat = (int)hp.size();
            cap_flat = n_flat;
            if (n_flat > 0) {
                if (!grow(st.scratch, (size_t)n_flat * 4) || !grow(S.rows, (size_t)n_flat * 4)) return dev_fail(e, "hipMalloc (random)");
                if (hipMemcpyAsync(st.scratch.p, hp.data(), (size_t)n_flat * 4, hipMemcpyHostToDevice, s) != hipSuccess)
                    return dev_fail(e, "random table upload failed");
                x.h2d += (size_t)n_flat * 4;
                Span sp(e, kTimeSweep);
                k_sw_pick<<<blocks_of(n_flat), kBlock, 0, s>>>(cand, (const int*)st.scratch.p, n_flat, (int*)S.rows.p);
            }
        } else {
            const bool first = p.sample_method == IMLS_SWEEP_NORMAL || st.counter == 1;
            imls_sample_params sp = first ? p.normal : p.major_axis;
            sp.method = first ? IMLS_SAMPLE_NORMAL : IMLS_SAMPLE_MAJOR_AXIS;
            sp.shuffle_seed = p.shuffle_seed;
            sp.rand_seed = p.rand_seed;
            if (int rc = check_sample_params(e, sp)) return rc;
            cap_flat = n_cand + sp.azimuth_bins * sp.elevation_bins;
            if (!grow(S.rows, (size_t)cap_flat * 4)) return dev_fail(e, "hipMalloc (sampled rows)");
            const int pm = (!first && prev) ? (int)prev->n_filtered : 0;
            if (int rc = sampler_dev(e, st.scratch, sp, (const float*)S.soa6.p, rows, cand, n_cand,
                                     pm > 0 ? (const float4*)prev->prev4.p : nullptr, pm > 0 ? (const float4*)prev->cbox.p : nullptr,
                                     pm, (int*)S.rows.p, &so, x))
                return rc;
            d_nout = so.d_nout;
            I.nan_normals = so.dropped;
        }
        if (cap_flat > 0) {
            if (!grow(S.flat, (size_t)cap_flat * 24)) return dev_fail(e, "hipMalloc (flat cloud)");
            Span sp(e, kTimeSweep);
            k_sw_gather_flat<<<blocks_of(cap_flat), kBlock, 0, s>>>((const float*)S.soa6.p, rows, (const int*)S.rows.p, d_nout,
                                                                    n_flat, (float*)S.flat.p);
        }
        if (hipGetLastError() != hipSuccess) return dev_fail(e, "sweep launch failed");
        unsigned long long nan = 0;
        ok = true;
        if (d_nout) { ok = hipMemcpyAsync(&n_flat, d_nout, 4, hipMemcpyDeviceToHost, s) == hipSuccess; x.d2h += 4; }
        if (d_nan) { ok = ok && hipMemcpyAsync(&nan, d_nan, 8, hipMemcpyDeviceToHost, s) == hipSuccess; x.d2h += 8; }
        ok = ok && hipStreamSynchronize(s) == hipSuccess;
        if (!ok) return dev_fail(e, "sweep sampling failed");
        x.syncs += 1;
        I.nan_keys = nan;
    }
    I.n_candidates = (uint64_t)n_cand;
    I.n_flat = (uint64_t)n_flat;
    I.bytes_h2d = x.h2d;
    I.bytes_d2h = x.d2h;
    I.host_syncs = x.syncs;
    S.n_filtered = (size_t)rows;
    S.n_flat = (size_t)n_flat;
    st.cur = nxt;
    st.has = true;
    st.counter += 1;
    if (info) *info = I;
    return IMLS_OK;
}

int sweep_download(SweepEnv& e, SweepState& st, int which, void* records, size_t cap, size_t* n, int32_t* sampled_index) {
    hipStream_t s = e.s;
    const SweepSet& S = st.set[st.cur];
    const size_t cnt = which == 0 ? S.n_filtered : S.n_flat;
    if (n) *n = cnt;
    if (cnt == 0) return IMLS_OK;
    bool ok = true;
    if (records) {
        if (cap < cnt) { *e.err = "sweep_download: capacity below the cloud size"; return IMLS_ERR_CAPACITY; }
        if (!grow(st.rec, cnt * 48)) return dev_fail(e, "hipMalloc (records)");
        const float* inten = (const float*)S.side.p;
        k_sw_pack<<<blocks_of(cnt), kBlock, 0, s>>>((const float*)S.soa6.p, (int)S.n_filtered, inten, inten + S.cap_filtered,
                                                    which == 1 ? (const int*)S.rows.p : nullptr, (int)cnt, (float4*)st.rec.p);
        ok = hipGetLastError() == hipSuccess;
        ok = ok && hipMemcpyAsync(records, st.rec.p, cnt * 48, hipMemcpyDeviceToHost, s) == hipSuccess;
    }
    if (sampled_index && which == 1)
        ok = ok && hipMemcpyAsync(sampled_index, S.rows.p, cnt * 4, hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) return dev_fail(e, "sweep download failed");
    return IMLS_OK;
}

}  // namespace imlsgpu
