// presample.hip — the upstream producer's curvature presample on gfx950 (scan_registration.cpp:
// 1071-1113 the per-point "curvature by difference", 1462-1473 the threshold, 1481-1489 the
// invalid-index erase).
//
// Layout: the ring-concatenated cloud `laserCloud` (1064-1069) as float4 (x, y, z, 0) in HBM and the
// ring prefix table ring_off[n_rings + 1].
//   k_curvature — a streaming stencil, one thread per point j: its ring comes from a binary search
//     of the prefix table; j is visited when it lies in [scanStartInd, scanEndInd) = [off + 5,
//     off + size − 6) of that ring (1076) and gets a value when w ≤ j < N − w (1081); the 2w + 1
//     window is read at GLOBAL indices (it runs across ring boundaries exactly as the reference's
//     laserCloud->points[j + k] does), three float sums in k order, no contraction.  Every other
//     point keeps 0 (UNPINNED: pcl::PointXYZINormal's default constructor zeroes curvature — inferred,
//     PCL itself is not part of this project's test oracle).
//   k_curv_flag / hipcub exclusive scan / k_curv_scatter — the candidate rows in ascending order.
// Roofline: memory-bound; 16 B read per point from HBM (the window's other 2w reads hit L1/L2: a
// wave's 64 consecutive points share them), 4 B written.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "internal.h"

namespace imlsgpu {
namespace {

__global__ __launch_bounds__(kBlock) void k_curvature(const float4* __restrict__ pts, const int* __restrict__ ring_off,
                                                      int n_rings, int n, int w, float* __restrict__ curv) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    // the ring holding j: the last i with ring_off[i] <= j (empty rings share an offset and are skipped)
    int lo = 0, hi = n_rings;                       // ring_off[lo] <= j < ring_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ring_off[mid] <= j) lo = mid; else hi = mid;
    }
    const int b = ring_off[lo], e = ring_off[lo + 1];
    float c = 0.f;
    // visited (1076) and enough neighbours (1081: j >= w && j < N − w; N ≥ w here since j < N − 6)
    if (j >= b + 5 && j < e - 6 && j >= w && j < n - w) {
        const float4 p = pts[j];
        float dx = 0.f, dy = 0.f, dz = 0.f;
        for (int k = -w; k <= w; ++k) {
            const float4 q = pts[j + k];
            dx = __fadd_rn(dx, __fsub_rn(q.x, p.x));
            dy = __fadd_rn(dy, __fsub_rn(q.y, p.y));
            dz = __fadd_rn(dz, __fsub_rn(q.z, p.z));
        }
        c = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));   // 1103
    }
    curv[j] = c;
}

// row r is a candidate when its point's curvature exceeds the threshold (1467, float compare) and
// the row is not one of the plane-invalid rows kept under use_all_points (1481-1489)
__global__ __launch_bounds__(kBlock) void k_curv_flag(const float* __restrict__ curv, const unsigned* __restrict__ row_index,
                                                      const unsigned char* __restrict__ row_flags, int n_rows, float thr,
                                                      unsigned* __restrict__ keep) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_rows) return;
    keep[r] = (curv[row_index[r]] > thr && !(row_flags[r] & IMLS_PCA_PLANE_INVALID)) ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void k_curv_scatter(const unsigned* __restrict__ keep, const unsigned* __restrict__ pos,
                                                         int n_rows, int* __restrict__ cand) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_rows || !keep[r]) return;
    cand[pos[r]] = r;
}

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

void curvature_enqueue(hipStream_t s, const imls_curvature_params& p, const float4* pts, const int* ring_off, int n_rings,
                       int n, const unsigned* row_index, const unsigned char* row_flags, int nr, float* curv,
                       unsigned* keep, unsigned* pos, int* cand, void* cub_tmp, size_t cub_bytes) {
    k_curvature<<<(n + kBlock - 1) / kBlock, kBlock, 0, s>>>(pts, ring_off, n_rings, n, p.window_size, curv);
    if (nr > 0) {
        k_curv_flag<<<(nr + kBlock - 1) / kBlock, kBlock, 0, s>>>(curv, row_index, row_flags, nr, p.curvature_threshold, keep);
        hipcub::DeviceScan::ExclusiveSum(cub_tmp, cub_bytes, keep, pos, nr, s);
        k_curv_scatter<<<(nr + kBlock - 1) / kBlock, kBlock, 0, s>>>(keep, pos, nr, cand);
    }
}

// Host side of imls_presample_curvature: upload, the stencil, the candidate compaction (the kernels
// are bracketed by marks[0..1] when non-null), and the D2H of the requested outputs.
int presample_curvature_run(hipStream_t s, const imls_curvature_params& p, const float* xyz, size_t stride,
                            const int32_t* sizes, int n_rings, const uint32_t* row_index, const uint8_t* row_flags,
                            size_t n_rows, DevBuf& mem, hipEvent_t* marks, float* curvature_out, int32_t* candidates_out,
                            size_t* n_cand, std::string& err) {
    std::vector<int> off(n_rings + 1, 0);
    for (int i = 0; i < n_rings; ++i) {
        if (sizes[i] < 0 || sizes[i] > (1 << 20)) { err = "ring size out of range"; return IMLS_ERR_ARG; }
        off[i + 1] = off[i] + sizes[i];
    }
    const int n = off[n_rings];
    for (size_t r = 0; r < n_rows; ++r)
        if (row_index[r] >= (uint32_t)n) { err = "row index out of range"; return IMLS_ERR_ARG; }
    if (n_cand) *n_cand = 0;
    if (n == 0) return IMLS_OK;                      // no point, hence no row
    const int nr = (int)n_rows;
    size_t cub_bytes = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, (unsigned*)nullptr, (unsigned*)nullptr, std::max(nr, 1), s) !=
        hipSuccess) { err = "hipcub scan size query failed"; return IMLS_ERR_DEVICE; }
    const size_t nn = (size_t)n, rr = (size_t)std::max(nr, 1);
    // device scratch: pts float4[n] | ring_off | curv[n] | row_index | row_flags | keep | pos | cand | cub
    const size_t o_pts = 0, o_off = al256(nn * 16), o_cv = al256(o_off + (n_rings + 1) * 4ull), o_ri = al256(o_cv + nn * 4),
                 o_rf = al256(o_ri + rr * 4), o_keep = al256(o_rf + rr), o_pos = al256(o_keep + rr * 4),
                 o_cand = al256(o_pos + rr * 4), o_cub = al256(o_cand + rr * 4), total = al256(o_cub + cub_bytes);
    if (!devbuf_grow(mem, total, total)) { err = "hipMalloc (curvature scratch)"; return IMLS_ERR_DEVICE; }
    char* m = (char*)mem.p;
    std::vector<float4> h(nn);
    for (int k = 0; k < n; ++k) h[k] = make_float4(xyz[k * stride], xyz[k * stride + 1], xyz[k * stride + 2], 0.f);
    bool ok = hipMemcpyAsync(m + o_pts, h.data(), nn * 16, hipMemcpyHostToDevice, s) == hipSuccess;
    ok = ok && hipMemcpyAsync(m + o_off, off.data(), (n_rings + 1) * 4ull, hipMemcpyHostToDevice, s) == hipSuccess;
    if (nr > 0) {
        ok = ok && hipMemcpyAsync(m + o_ri, row_index, (size_t)nr * 4, hipMemcpyHostToDevice, s) == hipSuccess;
        ok = ok && hipMemcpyAsync(m + o_rf, row_flags, (size_t)nr, hipMemcpyHostToDevice, s) == hipSuccess;
    }
    if (!ok) { err = "curvature upload failed"; return IMLS_ERR_DEVICE; }
    if (marks) (void)hipEventRecord(marks[0], s);
    curvature_enqueue(s, p, (const float4*)(m + o_pts), (const int*)(m + o_off), n_rings, n, (const unsigned*)(m + o_ri),
                      (const unsigned char*)(m + o_rf), nr, (float*)(m + o_cv), (unsigned*)(m + o_keep),
                      (unsigned*)(m + o_pos), (int*)(m + o_cand), m + o_cub, cub_bytes);
    if (marks) (void)hipEventRecord(marks[1], s);
    if (hipGetLastError() != hipSuccess) { err = "curvature launch failed"; return IMLS_ERR_DEVICE; }
    unsigned last_pos = 0, last_keep = 0;
    if (nr > 0) {
        ok = ok && hipMemcpyAsync(&last_pos, m + o_pos + (size_t)(nr - 1) * 4, 4, hipMemcpyDeviceToHost, s) == hipSuccess;
        ok = ok && hipMemcpyAsync(&last_keep, m + o_keep + (size_t)(nr - 1) * 4, 4, hipMemcpyDeviceToHost, s) == hipSuccess;
    }
    if (curvature_out) ok = ok && hipMemcpyAsync(curvature_out, m + o_cv, nn * 4, hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) { err = "curvature kernel failed"; return IMLS_ERR_DEVICE; }
    const size_t nc = (size_t)last_pos + last_keep;
    if (nc > 0 && candidates_out) {
        ok = hipMemcpyAsync(candidates_out, m + o_cand, nc * 4, hipMemcpyDeviceToHost, s) == hipSuccess;
        ok = ok && hipStreamSynchronize(s) == hipSuccess;
        if (!ok) { err = "curvature download failed"; return IMLS_ERR_DEVICE; }
    }
    if (n_cand) *n_cand = nc;
    return IMLS_OK;
}

}  // namespace imlsgpu
