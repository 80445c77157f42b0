// three_axis.hip — the upstream producer's "three_axis" sampling on gfx950 (threeAxisSampling,
// scan_registration.cpp:492-533): nine lists of (value, idx) per candidate, each ordered by
// std::greater<std::pair<float, int>> (larger value first, equal values → larger idx first), the
// first points_per_list indices of every list concatenated in list order.
//
//   k_ta_keys — one thread per candidate (its point, normal and eigenvalues gathered by the host
//     into float4 records, so the loads are coalesced): aD through the fp64 square roots the
//     reference's unqualified sqrt() selects, a2D, p × n and the literal unit-axis dot products in
//     float without contraction, then the nine values as UNIQUE 64-bit composites
//     orderable(value) << 32 | idx (−0 canonicalised to +0; a NaN value → orderable 0, i.e. after
//     every other entry, by descending idx, and counted).  List l occupies keys[l·n_cand, (l+1)·n_cand).
//   k_ta_select — the top-k of a list, exact because the composites are unique; one block per list:
//     histograms over the composite's next 11 high bits narrow to the bin holding the k-th largest
//     key until the keys at or above that bin fit the LDS buffer (≤ 4096), which are then compacted
//     and sorted (bitonic) in LDS.  (The plain alternative, a descending hipcub segmented radix sort
//     of all 9·n_cand composites and each segment's head, gave the same indices 34× slower and was
//     not kept: DESIGN.md §4 has both timings.)
// Roofline: k_ta_keys streams 40 B in and 72 B out per candidate; the select re-reads a list's keys
// (8 B each, L2-resident: 9 × 71k keys = 5 MB on an HDL-64 sweep) once per pass, 2-3 passes.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "internal.h"

namespace imlsgpu {
namespace {

typedef unsigned long long u64;

constexpr int kTaLists = 9;
constexpr int kTaMaxK = 4096;          // points_per_list bound = the LDS survivor buffer
constexpr int kTaSelBlock = 1024;      // threads of a select block (one block per list)
constexpr int kTaDigit = 11;           // bits per narrowing pass (2048 bins = 2 per thread)

__device__ __forceinline__ unsigned ta_orderable(float v, int& nan) {
    if (v != v) { nan++; return 0u; }                // below −inf's 0x007FFFFF
    unsigned u = __float_as_uint(v);
    if ((u & 0x7FFFFFFFu) == 0u) u = 0u;             // −0 → +0: equal under std::greater
    return u ^ ((u & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u);
}

// ga[k] = (x, y, z, λ1), gb[k] = (nx, ny, nz, λ2), gc[k] = (λ3, bits(idx)) of candidate k
__global__ __launch_bounds__(kBlock) void k_ta_keys(const float4* __restrict__ ga, const float4* __restrict__ gb,
                                                    const float2* __restrict__ gc, int n_cand, u64* __restrict__ keys,
                                                    u64* __restrict__ nan_count) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_cand) return;
    const float4 a = ga[k], b = gb[k];
    const float2 c = gc[k];
    const u64 idx = (u64)__float_as_uint(c.y);
    // 506-507: sqrt(double) on the float eigenvalues, the quotient rounded to float, then squared
    const float aD = (float)__ddiv_rn(__dsub_rn(__dsqrt_rn((double)b.w), __dsqrt_rn((double)c.x)), __dsqrt_rn((double)a.w));
    const float a2 = __fmul_rn(aD, aD), na2 = -a2;
    // 510: cross = p × n
    const float cx = __fsub_rn(__fmul_rn(a.y, b.z), __fmul_rn(a.z, b.y));
    const float cy = __fsub_rn(__fmul_rn(a.z, b.x), __fmul_rn(a.x, b.z));
    const float cz = __fsub_rn(__fmul_rn(a.x, b.y), __fmul_rn(a.y, b.x));
    // 511-519: v.dot(unit axis), evaluated literally (a non-finite component makes every dot NaN)
    const float dcx = __fadd_rn(__fadd_rn(__fmul_rn(cx, 1.f), __fmul_rn(cy, 0.f)), __fmul_rn(cz, 0.f));
    const float dcy = __fadd_rn(__fadd_rn(__fmul_rn(cx, 0.f), __fmul_rn(cy, 1.f)), __fmul_rn(cz, 0.f));
    const float dcz = __fadd_rn(__fadd_rn(__fmul_rn(cx, 0.f), __fmul_rn(cy, 0.f)), __fmul_rn(cz, 1.f));
    const float dnx = __fadd_rn(__fadd_rn(__fmul_rn(b.x, 1.f), __fmul_rn(b.y, 0.f)), __fmul_rn(b.z, 0.f));
    const float dny = __fadd_rn(__fadd_rn(__fmul_rn(b.x, 0.f), __fmul_rn(b.y, 1.f)), __fmul_rn(b.z, 0.f));
    const float dnz = __fadd_rn(__fadd_rn(__fmul_rn(b.x, 0.f), __fmul_rn(b.y, 0.f)), __fmul_rn(b.z, 1.f));
    const float v[kTaLists] = {__fmul_rn(a2, dcx), __fmul_rn(na2, dcx), __fmul_rn(a2, dcy), __fmul_rn(na2, dcy),
                               __fmul_rn(a2, dcz), __fmul_rn(na2, dcz), __fmul_rn(a2, fabsf(dnx)),
                               __fmul_rn(a2, fabsf(dny)), __fmul_rn(a2, fabsf(dnz))};
    int nan = 0;
#pragma unroll
    for (int l = 0; l < kTaLists; ++l) keys[(size_t)l * n_cand + k] = ((u64)ta_orderable(v[l], nan) << 32) | idx;
    if (nan) atomicAdd(nan_count, (u64)nan);
}

// Top-k of list blockIdx.x (k ≤ min(n, kTaMaxK)), descending, as indices into out[l·k, (l+1)·k).
__global__ __launch_bounds__(kTaSelBlock) void k_ta_select(const u64* __restrict__ keys, int n, int k, int* __restrict__ out) {
    typedef hipcub::BlockScan<unsigned, kTaSelBlock> Scan;
    __shared__ typename Scan::TempStorage scan_tmp;
    __shared__ unsigned hist[1 << kTaDigit];
    __shared__ u64 surv[kTaMaxK];
    __shared__ unsigned s_digit, s_above, s_bin, s_cnt;
    const int tid = threadIdx.x;
    const u64* K = keys + (size_t)blockIdx.x * n;
    u64 prefix = 0;                                  // the high `done` bits of the k-th largest key
    int done = 0;
    unsigned above = 0;                              // keys whose high bits exceed the prefix
    if (n > kTaMaxK) {
        for (;;) {
            const int width = min(kTaDigit, 64 - done), shift = 64 - done - width;
            const unsigned mask = (1u << width) - 1u;
            for (int b = tid; b < (1 << kTaDigit); b += kTaSelBlock) hist[b] = 0u;
            __syncthreads();
            for (int i = tid; i < n; i += kTaSelBlock) {
                const u64 key = K[i];
                if (done == 0 || (key >> (64 - done)) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & mask], 1u);
            }
            __syncthreads();
            // suffix sums from the top bin: the digit at which `above + count` first reaches k
            const int b0 = (1 << kTaDigit) - 1 - 2 * tid, b1 = b0 - 1;
            unsigned item[2] = {hist[b0], hist[b1]}, incl[2];
            Scan(scan_tmp).InclusiveSum(item, incl);
            const unsigned need = (unsigned)k - above;   // ≥ 1: `above` < k by construction
#pragma unroll
            for (int e = 0; e < 2; ++e)
                if (incl[e] >= need && incl[e] - item[e] < need) {
                    s_digit = (unsigned)(e == 0 ? b0 : b1);
                    s_above = above + (incl[e] - item[e]);
                    s_bin = item[e];
                }
            __syncthreads();
            prefix = (prefix << width) | s_digit;
            done += width;
            above = s_above;
            const unsigned total = above + s_bin;
            __syncthreads();                         // s_* and scan_tmp are rewritten by the next pass
            if (total <= (unsigned)kTaMaxK || done == 64) break;
        }
    }
    if (tid == 0) s_cnt = 0u;
    __syncthreads();
    for (int i = tid; i < n; i += kTaSelBlock) {
        const u64 key = K[i];
        if (done == 0 || (key >> (64 - done)) >= prefix) {
            const unsigned slot = atomicAdd(&s_cnt, 1u);
            if (slot < (unsigned)kTaMaxK) surv[slot] = key;
        }
    }
    __syncthreads();
    const int cnt = (int)min(s_cnt, (unsigned)kTaMaxK);
    int m = 1;
    while (m < cnt) m <<= 1;
    for (int i = cnt + tid; i < m; i += kTaSelBlock) surv[i] = 0ull;   // padding sorts last
    // bitonic sort, descending
    for (int size = 2; size <= m; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < (m >> 1); t += kTaSelBlock) {
                const int pos = 2 * t - (t & (stride - 1));
                const u64 x = surv[pos], y = surv[pos + stride];
                const bool desc = (pos & size) == 0;
                if ((x < y) == desc) { surv[pos] = y; surv[pos + stride] = x; }
            }
        }
    __syncthreads();
    for (int t = tid; t < k; t += kTaSelBlock) out[(size_t)blockIdx.x * k + t] = (int)(unsigned)(surv[t] & 0xFFFFFFFFull);
}

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

void three_axis_enqueue(hipStream_t s, const float4* ga, const float4* gb, const float2* gc, int nc, int k, u64* keys,
                        int* out, u64* nan) {
    k_ta_keys<<<(nc + kBlock - 1) / kBlock, kBlock, 0, s>>>(ga, gb, gc, nc, keys, nan);
    k_ta_select<<<kTaLists, kTaSelBlock, 0, s>>>(keys, nc, k, out);
}

// Host side of imls_sample_three_axis: the per-candidate gather and upload, the keys, the per-list
// top-k (the kernels bracketed by marks[0..1] when non-null), the D2H of the 9·k indices.
int three_axis_run(hipStream_t s, int points_per_list, const float* xyz, const float* nrm, size_t stride, size_t n,
                   const float* evals, const int32_t* cand, size_t n_cand, DevBuf& mem, hipEvent_t* marks,
                   int32_t* sampled_out, size_t* n_sampled, uint64_t* nan_keys, std::string& err) {
    if (n_sampled) *n_sampled = 0;
    if (nan_keys) *nan_keys = 0;
    if (n_cand == 0) return IMLS_OK;
    const int nc = (int)n_cand, k = std::min(points_per_list, nc);
    std::vector<float4> ha(2 * n_cand);
    std::vector<float2> hc(n_cand);
    for (size_t j = 0; j < n_cand; ++j) {
        const int idx = cand[j];
        if (idx < 0 || (size_t)idx >= n) { err = "candidate index out of range"; return IMLS_ERR_ARG; }
        const size_t i = (size_t)idx;
        ha[j] = make_float4(xyz[i * stride], xyz[i * stride + 1], xyz[i * stride + 2], evals[3 * i]);
        ha[n_cand + j] = make_float4(nrm[i * stride], nrm[i * stride + 1], nrm[i * stride + 2], evals[3 * i + 1]);
        float bits;
        static_assert(sizeof(bits) == sizeof(idx), "index bits travel in a float lane");
        __builtin_memcpy(&bits, &idx, 4);
        hc[j] = make_float2(evals[3 * i + 2], bits);
    }
    const size_t nk = (size_t)kTaLists * n_cand;
    // device scratch: ga | gb | gc | keys[9·n_cand] | out[9·k] | nan count
    const size_t o_a = 0, o_c = al256(n_cand * 32), o_k = al256(o_c + n_cand * 8), o_o = al256(o_k + nk * 8),
                 o_n = al256(o_o + (size_t)kTaLists * k * 4), total = al256(o_n + 8);
    if (!devbuf_grow(mem, total, total)) { err = "hipMalloc (three_axis scratch)"; return IMLS_ERR_DEVICE; }
    char* d = (char*)mem.p;
    bool ok = hipMemcpyAsync(d + o_a, ha.data(), n_cand * 32, hipMemcpyHostToDevice, s) == hipSuccess;
    ok = ok && hipMemcpyAsync(d + o_c, hc.data(), n_cand * 8, hipMemcpyHostToDevice, s) == hipSuccess;
    ok = ok && hipMemsetAsync(d + o_n, 0, 8, s) == hipSuccess;
    if (!ok) { err = "three_axis upload failed"; return IMLS_ERR_DEVICE; }
    if (marks) (void)hipEventRecord(marks[0], s);
    three_axis_enqueue(s, (const float4*)(d + o_a), (const float4*)(d + o_a) + n_cand, (const float2*)(d + o_c), nc, k,
                       (u64*)(d + o_k), (int*)(d + o_o), (u64*)(d + o_n));
    if (marks) (void)hipEventRecord(marks[1], s);
    if (hipGetLastError() != hipSuccess) { err = "three_axis launch failed"; return IMLS_ERR_DEVICE; }
    unsigned long long nan = 0;
    ok = hipMemcpyAsync(sampled_out, d + o_o, (size_t)kTaLists * k * 4, hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = ok && hipMemcpyAsync(&nan, d + o_n, 8, hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) { err = "three_axis kernel failed"; return IMLS_ERR_DEVICE; }
    if (n_sampled) *n_sampled = (size_t)kTaLists * k;
    if (nan_keys) *nan_keys = nan;
    return IMLS_OK;
}

}  // namespace imlsgpu
