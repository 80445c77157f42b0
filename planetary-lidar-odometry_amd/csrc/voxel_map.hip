// voxel_map.hip — the voxel map's update (imls_voxel_map_update).
//
// The map is an ordered SoA6 list of (point, normal) floats in the map frame.  One update:
//   k_vox_keys   one lane per candidate (the old map's rows, then the scan's): the scan row enters the
//                map frame (pose_point, the posed push's arithmetic) and is written to the staging
//                scan; the voxel key comes from the stored floats (floor of an IEEE double division
//                per axis), the range test from the pose's translation; a dropped candidate gets the
//                sentinel key (above every valid key: 63 bits are used) and is counted by its class
//   hipcub radix sort of (key, candidate index), stable: old rows come first within a key
//   k_vox_keep   rank < cap ⇔ the row `cap` places earlier has another key (the order is sorted, so
//                no segmented scan is needed); heads counted as voxels, dropped rows by age
//   hipcub exclusive sum of the keep flags, k_vox_gather: order-keeping gather into the other map
//                buffer, whose column pitch is the kept count (read from the scan's last entry)
// Counters are integer wave ballots added with integer atomics: the sums do not depend on the
// launch order.  Ordinary vector loads and stores only.
#include <hipcub/hipcub.hpp>

#include "internal.h"

namespace imlsgpu {
namespace {

constexpr unsigned long long kVoxSentinel = ~0ull;
constexpr double kVoxLo = -1048576.0, kVoxHi = 1048575.0;   // −2²⁰ … 2²⁰ − 1

inline size_t part(size_t bytes) { return (bytes + 255) / 256 * 256; }
inline unsigned grid_for(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// the wave's count of lanes with `hit`, added once by its first active lane
__device__ __forceinline__ void wave_count(bool hit, unsigned* __restrict__ word) {
    const unsigned long long m = __ballot(hit);
    if (m != 0 && hit && (__ffsll((long long)m) - 1) == (int)(threadIdx.x & 63)) atomicAdd(word, (unsigned)__popcll(m));
}

__global__ void __launch_bounds__(kBlock) k_vox_keys(const float* __restrict__ map, size_t n_old, const float* scan_in,
                                                     float* scan_out, size_t n, const VoxelGrid G,
                                                     unsigned long long* __restrict__ key, unsigned* __restrict__ val,
                                                     unsigned* __restrict__ rec) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n_old + n;
    const bool old = i < n_old;
    float x = 0.f, y = 0.f, z = 0.f;
    bool finite = true;
    if (live && old) {
        x = map[i]; y = map[n_old + i]; z = map[2 * n_old + i];
    } else if (live) {
        const size_t j = i - n_old;
        float v[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = scan_in[k * n + j];
        finite = isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]);
        if (finite && !G.identity) {
            float p[3], q[3];
            pose_point(G.P, v[0], v[1], v[2], v[3], v[4], v[5], p, q);
#pragma unroll
            for (int k = 0; k < 3; ++k) { v[k] = p[k]; v[3 + k] = q[k]; }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) scan_out[k * n + j] = v[k];
        x = v[0]; y = v[1]; z = v[2];
    }
    // the voxel index from the stored floats; compared in double (a NaN or an infinity fails)
    const double ix = floor((double)x / G.voxel), iy = floor((double)y / G.voxel), iz = floor((double)z / G.voxel);
    const bool in_grid = ix >= kVoxLo && ix <= kVoxHi && iy >= kVoxLo && iy <= kVoxHi && iz >= kVoxLo && iz <= kVoxHi;
    const double dx = (double)x - G.P.T[3], dy = (double)y - G.P.T[7], dz = (double)z - G.P.T[11];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    const bool in_range = d2 <= G.r2;
    const bool grid_drop = live && finite && !in_grid;
    const bool range_drop = live && finite && in_grid && !in_range;
    wave_count(live && !finite, rec + kVoxScanNonfinite);
    wave_count(grid_drop && !old, rec + kVoxScanGrid);
    wave_count(grid_drop && old, rec + kVoxMapGrid);
    wave_count(range_drop && !old, rec + kVoxScanRange);
    wave_count(range_drop && old, rec + kVoxMapRange);
    if (!live) return;
    unsigned long long k = kVoxSentinel;
    if (finite && in_grid && in_range)
        k = ((unsigned long long)((long long)iz + 1048576ll) << 42) | ((unsigned long long)((long long)iy + 1048576ll) << 21) |
            (unsigned long long)((long long)ix + 1048576ll);
    key[i] = k;
    val[i] = (unsigned)i;
}

__global__ void __launch_bounds__(kBlock) k_vox_keep(const unsigned long long* __restrict__ key, const unsigned* __restrict__ val,
                                                     size_t total, size_t n_old, unsigned long long cap,
                                                     unsigned* __restrict__ keep, unsigned* __restrict__ rec) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < total;
    unsigned long long k = kVoxSentinel;
    bool head = false, full = false, old = false;
    if (live) {
        k = key[i];
        if (k != kVoxSentinel) {
            head = i == 0 || key[i - 1] != k;
            full = (unsigned long long)i >= cap && key[i - (size_t)cap] == k;
            old = val[i] < n_old;
        }
    }
    wave_count(head, rec + kVoxVoxels);
    wave_count(full && old, rec + kVoxMapTrimmed);
    wave_count(full && !old, rec + kVoxScanFull);
    if (live) keep[i] = (k != kVoxSentinel && !full) ? 1u : 0u;
}

__global__ void __launch_bounds__(kBlock) k_vox_gather(const float* __restrict__ map, size_t n_old, const float* __restrict__ scan,
                                                       size_t n, const unsigned* __restrict__ val,
                                                       const unsigned* __restrict__ keep, const unsigned* __restrict__ pos,
                                                       size_t total, float* __restrict__ out, unsigned* __restrict__ rec) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t kept = (size_t)pos[total - 1] + keep[total - 1];   // the new map's size = its column pitch
    if (i == total - 1) rec[kVoxKept] = (unsigned)kept;
    if (!keep[i]) return;
    const size_t src = val[i], o = pos[i];
    const float* col = src < n_old ? map + src : scan + (src - n_old);
    const size_t pitch = src < n_old ? n_old : n;
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k * kept + o] = col[k * pitch];
}

}  // namespace

int voxel_map_merge(hipStream_t s, const float* map, size_t n_old, const float* scan_in, float* scan_out, size_t n,
                    const VoxelGrid& g, float* out, DevBuf& scratch, unsigned* h_rec, std::string& err) {
    const size_t total = n_old + n;
    if (total == 0) {
        for (int k = 0; k < kVoxRecWords; ++k) h_rec[k] = 0;
        return IMLS_OK;
    }
    if (total > (size_t)0x7fffffff) {
        err = "voxel map: too many candidates";
        return IMLS_ERR_CAPACITY;
    }
    size_t sort_b = 0, scan_b = 0;
    {
        hipcub::DoubleBuffer<unsigned long long> kq(nullptr, nullptr);
        hipcub::DoubleBuffer<unsigned> vq(nullptr, nullptr);
        if (hipcub::DeviceRadixSort::SortPairs(nullptr, sort_b, kq, vq, (int)total, 0, 64, s) != hipSuccess ||
            hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, (unsigned*)nullptr, (unsigned*)nullptr, (int)total, s) != hipSuccess) {
            err = "hipcub size query failed";
            return IMLS_ERR_DEVICE;
        }
    }
    const size_t cub_b = std::max(sort_b, scan_b);
    const size_t need = 2 * part(total * 8) + 4 * part(total * 4) + part(kVoxRecWords * 4) + part(cub_b) + 256;
    if (!devbuf_grow(scratch, need, need + need / 4)) {
        err = "hipMalloc failed (voxel map scratch)";
        return IMLS_ERR_DEVICE;
    }
    char* p = (char*)scratch.p;
    unsigned long long* k0 = carve<unsigned long long>(p, total);
    unsigned long long* k1 = carve<unsigned long long>(p, total);
    unsigned* v0 = carve<unsigned>(p, total);
    unsigned* v1 = carve<unsigned>(p, total);
    unsigned* keep = carve<unsigned>(p, total);
    unsigned* pos = carve<unsigned>(p, total);
    unsigned* rec = carve<unsigned>(p, kVoxRecWords);
    void* cub_tmp = carve<char>(p, cub_b);
    if (hipMemsetAsync(rec, 0, kVoxRecWords * 4, s) != hipSuccess) {
        err = "hipMemset (voxel map record)";
        return IMLS_ERR_DEVICE;
    }
    k_vox_keys<<<grid_for(total), kBlock, 0, s>>>(map, n_old, scan_in, scan_out, n, g, k0, v0, rec);
    hipcub::DoubleBuffer<unsigned long long> kb(k0, k1);
    hipcub::DoubleBuffer<unsigned> vb(v0, v1);
    size_t tmp_b = cub_b;
    if (hipcub::DeviceRadixSort::SortPairs(cub_tmp, tmp_b, kb, vb, (int)total, 0, 64, s) != hipSuccess) {
        err = "voxel map sort failed";
        return IMLS_ERR_DEVICE;
    }
    k_vox_keep<<<grid_for(total), kBlock, 0, s>>>(kb.Current(), vb.Current(), total, n_old, g.cap, keep, rec);
    tmp_b = cub_b;
    if (hipcub::DeviceScan::ExclusiveSum(cub_tmp, tmp_b, keep, pos, (int)total, s) != hipSuccess) {
        err = "voxel map scan failed";
        return IMLS_ERR_DEVICE;
    }
    k_vox_gather<<<grid_for(total), kBlock, 0, s>>>(map, n_old, scan_out, n, vb.Current(), keep, pos, total, out, rec);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(h_rec, rec, kVoxRecWords * 4, hipMemcpyDeviceToHost, s) != hipSuccess) {
        err = "voxel map launch failed";
        return IMLS_ERR_DEVICE;
    }
    return IMLS_OK;
}

}  // namespace imlsgpu
