// deskew.hip — per-point motion compensation of a sweep on gfx950: what A-LOAM's TransformToStart /
// TransformToEnd do (laser_odometry.cpp:62-114; switched off there by `#define DISTORTION 0`, 29-30,
// their calls commented out, 428 / 459), from the time of measurement the front end leaves in
// intensity = ring + scanPeriod·relTime (scan_registration.cpp:1042-1048).
//
// Model.  M = (R, t) is the sensor at the sweep's end in the frame of the sensor at its
// start.  R = R(a, θ); a point measured at fraction s of the sweep was seen from (R(a, s·θ), s·t), so
//   q_start = R(a, s·θ)·p + s·t            (Rodrigues: p·c + (a×p)·σ + a·(a·p)·(1 − c))
//   q_end   = Rᵀ·(q_start − t)
// with s = (I − float(int(I))) / scan_period from the float intensity I, not clamped.  Everything per
// point is fp64 from the float inputs, evaluated as written (-ffp-contract=off), each coordinate
// rounded to float once; the intensity is kept.  A normal is rotated the same way without the
// translations.  A row with a non-finite coordinate or intensity is left as it is (its normal too),
// and so is a normal with a non-finite component.
//
// One lane per point: one 16-byte load and one 16-byte store of the record (and of the normal), in
// place.  The motion is a by-value launch argument (kernarg → scalar loads): nothing is uploaded and
// the host waits for nothing.
// Roofline: 32 B (64 B with normals) of HBM traffic against one fp64 sincos and ~60 fp64 operations per
// point — VALU-bound, a few µs at one sweep (≤ 130k records), so launch latency is what a sweep sees.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "internal.h"

namespace imlsgpu {
namespace {

// static_cast<int>(float) as x86-64 evaluates it (cvttss2si): truncation, INT_MIN out of range
__device__ __forceinline__ int x86_f2i(float v) {
    return (v > -2147483904.0f && v < 2147483648.0f) ? (int)v : INT_MIN;
}

// R(a, φ)·p by Rodrigues' formula, c = cos φ, sn = sin φ
__device__ __forceinline__ void rodrigues(const DeskewArg& A, double c, double sn, double px, double py, double pz,
                                          double out[3]) {
    const double cx = A.a[1] * pz - A.a[2] * py, cy = A.a[2] * px - A.a[0] * pz, cz = A.a[0] * py - A.a[1] * px;
    const double k = ((A.a[0] * px + A.a[1] * py) + A.a[2] * pz) * (1.0 - c);
    out[0] = (px * c + cx * sn) + A.a[0] * k;
    out[1] = (py * c + cy * sn) + A.a[1] * k;
    out[2] = (pz * c + cz * sn) + A.a[2] * k;
}

__device__ __forceinline__ void rt_mul(const DeskewArg& A, const double v[3], double out[3]) {
    out[0] = (A.Rt[0] * v[0] + A.Rt[1] * v[1]) + A.Rt[2] * v[2];
    out[1] = (A.Rt[3] * v[0] + A.Rt[4] * v[1]) + A.Rt[5] * v[2];
    out[2] = (A.Rt[6] * v[0] + A.Rt[7] * v[1]) + A.Rt[8] * v[2];
}

__global__ __launch_bounds__(kBlock) void k_deskew(float4* __restrict__ rec, float4* __restrict__ nrm, size_t n,
                                                   float scan_period, const DeskewArg A) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 q = rec[i];
    if (!(isfinite(q.x) && isfinite(q.y) && isfinite(q.z) && isfinite(q.w))) return;   // in place: kept bit for bit
    const double s = (double)(q.w - (float)x86_f2i(q.w)) / (double)scan_period;          // laser_odometry.cpp:68 / 95
    const double phi = s * A.theta;
    double sn, c;
    sincos(phi, &sn, &c);
    double v[3], w[3];
    rodrigues(A, c, sn, (double)q.x, (double)q.y, (double)q.z, v);
    v[0] = v[0] + s * A.t[0];
    v[1] = v[1] + s * A.t[1];
    v[2] = v[2] + s * A.t[2];
    if (!A.to_start) {
        v[0] = v[0] - A.t[0];
        v[1] = v[1] - A.t[1];
        v[2] = v[2] - A.t[2];
        rt_mul(A, v, w);
        v[0] = w[0]; v[1] = w[1]; v[2] = w[2];
    }
    rec[i] = make_float4((float)v[0], (float)v[1], (float)v[2], q.w);
    if (nrm) {
        const float4 m = nrm[i];
        if (!(isfinite(m.x) && isfinite(m.y) && isfinite(m.z))) return;
        rodrigues(A, c, sn, (double)m.x, (double)m.y, (double)m.z, v);
        if (!A.to_start) {
            rt_mul(A, v, w);
            v[0] = w[0]; v[1] = w[1]; v[2] = w[2];
        }
        nrm[i] = make_float4((float)v[0], (float)v[1], (float)v[2], m.w);
    }
}

}  // namespace

int deskew_prepare(const double M[16], int to_frame, DeskewArg* out, bool* identity, std::string& err) {
    bool id = true;
    for (int k = 0; k < 16; ++k) {
        if (!std::isfinite(M[k])) { err = "deskew: non-finite motion entry"; return IMLS_ERR_ARG; }
        if (M[k] != ((k % 5 == 0) ? 1.0 : 0.0)) id = false;
    }
    if (to_frame != IMLS_DESKEW_TO_END && to_frame != IMLS_DESKEW_TO_START) {
        err = "deskew: to_frame must be 0 (sweep end) or 1 (sweep start)";
        return IMLS_ERR_ARG;
    }
    const double R[3][3] = {{M[0], M[1], M[2]}, {M[4], M[5], M[6]}, {M[8], M[9], M[10]}};
    const double v[3] = {0.5 * (R[2][1] - R[1][2]), 0.5 * (R[0][2] - R[2][0]), 0.5 * (R[1][0] - R[0][1])};
    const double nv = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const double theta = std::atan2(nv, (((R[0][0] + R[1][1]) + R[2][2]) - 1.0) / 2.0);
    if (!(theta < 1.5707963267948966)) { err = "deskew: the motion's rotation must be below 90 degrees"; return IMLS_ERR_ARG; }
    DeskewArg A{};
    if (nv == 0.0) {
        A.a[0] = 0.0; A.a[1] = 0.0; A.a[2] = 1.0;
    } else {
        for (int k = 0; k < 3; ++k) A.a[k] = v[k] / nv;
    }
    A.theta = theta;
    A.t[0] = M[3]; A.t[1] = M[7]; A.t[2] = M[11];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) A.Rt[3 * r + c] = R[c][r];
    A.to_start = to_frame == IMLS_DESKEW_TO_START;
    *out = A;
    *identity = id;
    return IMLS_OK;
}

void deskew_enqueue(hipStream_t s, const DeskewArg& A, float scan_period, float4* xyzi, float4* nrm, size_t n) {
    if (n == 0) return;
    k_deskew<<<(unsigned)((n + kBlock - 1) / kBlock), kBlock, 0, s>>>(xyzi, nrm, n, scan_period, A);
}

int deskew_host(hipStream_t s, const DeskewArg& A, float scan_period, float* xyzi, size_t stride, size_t n, float* nrm,
                size_t nstride, DevBuf& mem, hipEvent_t* marks, std::string& err) {
    if (n == 0) return IMLS_OK;
    const size_t bytes = n * 16;
    if (!devbuf_grow(mem, (nrm ? 2 : 1) * bytes, (nrm ? 2 : 1) * bytes + bytes / 2)) {
        err = "hipMalloc (deskew)";
        return IMLS_ERR_DEVICE;
    }
    float4* d_rec = (float4*)mem.p;
    float4* d_nrm = nrm ? d_rec + n : nullptr;
    // staging: records of another stride are packed to 16 bytes (a normal's fourth float is 0)
    std::vector<float> hrec, hnrm;
    const float* up = xyzi;
    if (stride != 4) {
        hrec.resize(4 * n);
        for (size_t i = 0; i < n; ++i) std::memcpy(&hrec[4 * i], xyzi + i * stride, 16);
        up = hrec.data();
    }
    bool ok = hipMemcpyAsync(d_rec, up, bytes, hipMemcpyHostToDevice, s) == hipSuccess;
    if (nrm) {
        hnrm.assign(4 * n, 0.f);
        for (size_t i = 0; i < n; ++i) std::memcpy(&hnrm[4 * i], nrm + i * nstride, 12);
        ok = ok && hipMemcpyAsync(d_nrm, hnrm.data(), bytes, hipMemcpyHostToDevice, s) == hipSuccess;
    }
    if (!ok) { err = "deskew upload failed"; return IMLS_ERR_DEVICE; }
    if (marks) (void)hipEventRecord(marks[0], s);
    deskew_enqueue(s, A, scan_period, d_rec, d_nrm, n);
    ok = hipGetLastError() == hipSuccess;
    if (marks) (void)hipEventRecord(marks[1], s);
    ok = ok && hipMemcpyAsync(stride == 4 ? xyzi : hrec.data(), d_rec, bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
    if (nrm) ok = ok && hipMemcpyAsync(hnrm.data(), d_nrm, bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) { err = "deskew failed"; return IMLS_ERR_DEVICE; }
    if (stride != 4)
        for (size_t i = 0; i < n; ++i) std::memcpy(xyzi + i * stride, &hrec[4 * i], 16);
    if (nrm)
        for (size_t i = 0; i < n; ++i) std::memcpy(nrm + i * nstride, &hnrm[4 * i], 12);
    return IMLS_OK;
}

}  // namespace imlsgpu
