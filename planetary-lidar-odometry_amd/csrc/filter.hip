// filter.hip — the NaN filter with its order-preserving compaction (RemoveNANandINFData,
// imls_icp.cpp:58-72; the source loader setSourcePointCloud, imls_icp.cpp:74-78, is the filter
// alone), lone, posed and batched, and the pose kernels of the posed map.
// All kernels are HBM-streaming: coalesced float loads, float4 stores.
#include <hipcub/hipcub.hpp>

#include "index_common.h"

namespace imlsgpu {
namespace {

__global__ void k_flag_finite(const float* __restrict__ soa, size_t n, unsigned* __restrict__ flag) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x = soa[i], y = soa[n + i], z = soa[2 * n + i];
    flag[i] = (isfinite(x) && isfinite(y) && isfinite(z)) ? 1u : 0u;
}

// scatter kept points to float4 records; pos = exclusive prefix sum of flags.  POSED (a posed map
// push): each kept point written in the map frame.
template <bool POSED>
__device__ __forceinline__ void compact_body(const float* __restrict__ soa, size_t n, const unsigned* __restrict__ flag,
                                             const unsigned* __restrict__ pos, float4* __restrict__ pt,
                                             float4* __restrict__ nr, unsigned* __restrict__ kept_index,
                                             int* __restrict__ h_count, const Pose12* P) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i == n - 1) *h_count = (int)(pos[i] + flag[i]);   // pinned host memory, written directly (no copy launch per filter)
    if (!flag[i]) return;
    unsigned o = pos[i];
    if constexpr (POSED) {
        float x[3], nn[3];
        pose_point(*P, soa[i], soa[n + i], soa[2 * n + i], soa[3 * n + i], soa[4 * n + i], soa[5 * n + i], x, nn);
        pt[o] = make_float4(x[0], x[1], x[2], 0.f);
        nr[o] = make_float4(nn[0], nn[1], nn[2], 0.f);
    } else {
        pt[o] = make_float4(soa[i], soa[n + i], soa[2 * n + i], 0.f);
        nr[o] = make_float4(soa[3 * n + i], soa[4 * n + i], soa[5 * n + i], 0.f);
    }
    if (kept_index) kept_index[o] = (unsigned)i;
}

__global__ void k_compact(const float* __restrict__ soa, size_t n, const unsigned* __restrict__ flag,
                          const unsigned* __restrict__ pos, float4* __restrict__ pt, float4* __restrict__ nr,
                          unsigned* __restrict__ kept_index, int* __restrict__ h_count) {
    compact_body<false>(soa, n, flag, pos, pt, nr, kept_index, h_count, nullptr);
}

// The pose is a launch argument (constant address space: scalar loads, wave-uniform).
__global__ void k_compact_posed(const float* __restrict__ soa, size_t n, const unsigned* __restrict__ flag,
                                const unsigned* __restrict__ pos, float4* __restrict__ pt, float4* __restrict__ nr,
                                unsigned* __restrict__ kept_index, int* __restrict__ h_count, const Pose12 P) {
    compact_body<true>(soa, n, flag, pos, pt, nr, kept_index, h_count, &P);
}

// an SoA6 scan re-expressed under P (out may be in: every thread reads its point before it writes it)
__global__ void k_pose_soa6(const float* in, float* out, size_t n, const Pose12 P) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = in[k * n + i];
    if (isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2])) {
        float x[3], nn[3];
        pose_point(P, v[0], v[1], v[2], v[3], v[4], v[5], x, nn);
#pragma unroll
        for (int k = 0; k < 3; ++k) { v[k] = x[k]; v[3 + k] = nn[k]; }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k * n + i] = v[k];
}

// filtered float4 records re-expressed under P in place (imls_map_rebase): 16-B loads and stores
__global__ void k_pose_records(float4* __restrict__ pt, float4* __restrict__ nr, size_t n, const Pose12 P) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = pt[i], q = nr[i];
    float x[3], nn[3];
    pose_point(P, p.x, p.y, p.z, q.x, q.y, q.z, x, nn);
    pt[i] = make_float4(x[0], x[1], x[2], p.w);
    nr[i] = make_float4(nn[0], nn[1], nn[2], q.w);
}

}  // namespace

// NaN filter + order-keeping compaction, asynchronous: the kept count lands in *h_count (pinned,
// device-visible host memory) from the compaction kernel itself — valid once the stream has passed it.
int filter_async(hipStream_t s, const float* d_soa6, size_t n_in, DevBuf& pt, DevBuf& nr, DevBuf& scratch,
                 unsigned* d_kept, int* h_count, std::string& err, const Pose12* pose) {
    size_t cub_bytes = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, (unsigned*)nullptr, (unsigned*)nullptr, (int)n_in, s) != hipSuccess) {
        err = "hipcub scan size query failed";
        return IMLS_ERR_DEVICE;
    }
    size_t need = 2 * carve_bytes<unsigned>(n_in) + carve_bytes<char>(cub_bytes);
    if (!ensure(scratch, need, err) || !ensure(pt, n_in * 16 + 16, err) || !ensure(nr, n_in * 16 + 16, err)) return IMLS_ERR_DEVICE;
    char* p = (char*)scratch.p;
    unsigned* flag = carve<unsigned>(p, n_in);
    unsigned* pos = carve<unsigned>(p, n_in);
    void* cub_tmp = carve<char>(p, cub_bytes);
    k_flag_finite<<<grid_for(n_in), kBlock, 0, s>>>(d_soa6, n_in, flag);
    hipcub::DeviceScan::ExclusiveSum(cub_tmp, cub_bytes, flag, pos, (int)n_in, s);
    if (pose)
        k_compact_posed<<<grid_for(n_in), kBlock, 0, s>>>(d_soa6, n_in, flag, pos, (float4*)pt.p, (float4*)nr.p, d_kept,
                                                          h_count, *pose);
    else
        k_compact<<<grid_for(n_in), kBlock, 0, s>>>(d_soa6, n_in, flag, pos, (float4*)pt.p, (float4*)nr.p, d_kept, h_count);
    return launched("filter/compact launch failed", err);
}

int pose_soa6(hipStream_t s, const float* in, float* out, size_t n, const Pose12& pose, std::string& err) {
    if (n == 0) return IMLS_OK;
    k_pose_soa6<<<grid_for(n), kBlock, 0, s>>>(in, out, n, pose);
    return launched("pose launch failed", err);
}

int pose_records(hipStream_t s, float4* pt, float4* nr, size_t n, const Pose12& pose, std::string& err) {
    if (n == 0) return IMLS_OK;
    k_pose_records<<<grid_for(n), kBlock, 0, s>>>(pt, nr, n, pose);
    return launched("pose launch failed", err);
}

// ---------------------------------------------------------------------------------------------
// Batched NaN filters (imls_register_frames): every pending filter of a batch's members in three
// launches — per 256-point block counts, one scan block per job (its kept count to the job's
// pinned host word), order-keeping scatter.  Same output as filter_async, frame by frame.
// ---------------------------------------------------------------------------------------------
namespace {

struct FilterJobDev {
    const float* soa;                 // SoA6 input [6][n]
    size_t n;
    float4 *pt, *nr;                  // kept points / normals
    unsigned* kept;                   // kept → input index, or null
    int* h_count;                     // pinned host word
    int* blk;                         // [nb] block counts → offsets
};

__device__ __forceinline__ bool finite_at(const float* soa, size_t n, size_t i) {
    return isfinite(soa[i]) && isfinite(soa[n + i]) && isfinite(soa[2 * n + i]);
}

__global__ __launch_bounds__(kBlock) void k_filter_count_b(const FilterJobDev* __restrict__ jobs) {
    const FilterJobDev& J = jobs[blockIdx.y];
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if ((size_t)blockIdx.x * kBlock >= J.n) return;
    const bool keep = i < J.n && finite_at(J.soa, J.n, i);
    __shared__ int wc[kBlock / 64];
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int k = 0; k < kBlock / 64; ++k) c += wc[k];
        J.blk[blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(1024) void k_filter_scan_b(const FilterJobDev* __restrict__ jobs) {
    const FilterJobDev& J = jobs[blockIdx.x];
    const int nb = (int)((J.n + kBlock - 1) / kBlock);
    __shared__ int sc[1024];
    int carry = 0;
    for (int base = 0; base < nb; base += 1024) {
        const int b = base + threadIdx.x;
        const int v = b < nb ? J.blk[b] : 0;
        sc[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int t = threadIdx.x >= off ? sc[threadIdx.x - off] : 0;
            __syncthreads();
            sc[threadIdx.x] += t;
            __syncthreads();
        }
        if (b < nb) J.blk[b] = carry + sc[threadIdx.x] - v;
        __syncthreads();
        carry += sc[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *J.h_count = carry;
}

__global__ __launch_bounds__(kBlock) void k_filter_scatter_b(const FilterJobDev* __restrict__ jobs) {
    const FilterJobDev& J = jobs[blockIdx.y];
    if ((size_t)blockIdx.x * kBlock >= J.n) return;
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool keep = i < J.n && finite_at(J.soa, J.n, i);
    __shared__ int wc[kBlock / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wc[wv] = __popcll(m);
    __syncthreads();
    if (!keep) return;
    int o = J.blk[blockIdx.x];
    for (int k = 0; k < wv; ++k) o += wc[k];
    o += __popcll(m & ((1ull << lane) - 1ull));
    const float* s = J.soa;
    const size_t n = J.n;
    J.pt[o] = make_float4(s[i], s[n + i], s[2 * n + i], 0.f);
    J.nr[o] = make_float4(s[3 * n + i], s[4 * n + i], s[5 * n + i], 0.f);
    if (J.kept) J.kept[o] = (unsigned)i;
}

}  // namespace

size_t filter_job_bytes() { return sizeof(FilterJobDev); }

int filter_batch(hipStream_t s, const std::vector<FilterJob>& jobs, DevBuf& scratch, DevBuf& table, void* h_table,
                 size_t h_table_bytes, std::string& err) {
    const int nj = (int)jobs.size();
    if (nj == 0) return IMLS_OK;
    if ((size_t)nj * sizeof(FilterJobDev) > h_table_bytes) { err = "filter table too small"; return IMLS_ERR_CAPACITY; }
    if (nj > 65535) { err = "too many filter jobs"; return IMLS_ERR_CAPACITY; }
    size_t blk_bytes = 0, maxn = 1;
    for (const auto& f : jobs) {
        blk_bytes += carve_bytes<int>(grid_for(f.n) + 1);
        maxn = std::max(maxn, f.n);
    }
    if (!ensure(scratch, blk_bytes, err) || !ensure(table, (size_t)nj * sizeof(FilterJobDev) + 256, err)) return IMLS_ERR_DEVICE;
    char* p = (char*)scratch.p;
    FilterJobDev* J = (FilterJobDev*)h_table;
    for (int q = 0; q < nj; ++q) {
        const FilterJob& f = jobs[q];
        if (!ensure(*f.pt, f.n * 16 + 16, err) || !ensure(*f.nr, f.n * 16 + 16, err)) return IMLS_ERR_DEVICE;
        FilterJobDev d{};
        d.soa = f.soa;
        d.n = f.n;
        d.pt = (float4*)f.pt->p;
        d.nr = (float4*)f.nr->p;
        d.kept = f.kept;
        d.h_count = f.h_count;
        d.blk = carve<int>(p, grid_for(f.n) + 1);
        J[q] = d;
    }
    const FilterJobDev* jd = (const FilterJobDev*)table.p;
    hipMemcpyAsync(table.p, h_table, (size_t)nj * sizeof(FilterJobDev), hipMemcpyHostToDevice, s);
    const unsigned gx = grid_for(maxn);
    k_filter_count_b<<<dim3(gx, nj), kBlock, 0, s>>>(jd);
    k_filter_scan_b<<<nj, 1024, 0, s>>>(jd);
    k_filter_scatter_b<<<dim3(gx, nj), kBlock, 0, s>>>(jd);
    return launched("batched filter launch failed", err);
}

}  // namespace imlsgpu
