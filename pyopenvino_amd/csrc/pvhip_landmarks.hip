// A landmark network's points become the (n, 7) table of the warp entry, on the device: the least-squares similarity from a template onto
// the points of every row, in binary64, every operation rounded once in the order include/pvhip.h writes (pvhip_landmarks_to_warps).
// pyopenvino_amd/landmarks.py is the same rule in Python floats, tests/landmark_warps_ref.py in numpy; all three agree bit for bit.
//
// A latency kernel: n threads of about 10 K binary64 operations each, one thread per row, 64 per workgroup, no LDS.  The K loops are
// serial, so the order of every sum is the rule's; this file is compiled with -ffp-contract=off like the rest and says so again below.
// A second launch of one wave behind the first on the same stream counts the valid rows: no atomics, every output word has one writer.
#include "pvhip_common.h"

#pragma clang fp contract(off)

using namespace pvhip;

namespace {

struct LandmarkArgs {
    const float*  points;    // [rows][2 k]: x0, y0, x1, y1, ... normalised to the region, 0 its left / top edge, 1 its right / bottom edge
    const int*    regions;   // [rows][5]: (id, x, y, w, h), or NULL: the whole frame
    const double* tmpl;      // [2 k + 3]: tbx, tby, S, cx_0, cy_0, ...
    long long*    table;     // [n][7]
    int*          valid;     // [n + 1]: valid[0..n), count
    int n, rows, k, m, src_h, src_w;
};

constexpr double kQ16       = 65536.0;
constexpr double kLinear    = 67108864.0;          // 2^26
constexpr double kTranslate = 1099511627776.0;     // 2^40
constexpr int    kExtent    = 1 << 24;

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }

__global__ __launch_bounds__(kWave) void landmarks_to_warps_kernel(LandmarkArgs a) {
    const int b = blockIdx.x * kWave + threadIdx.x;
    if (b >= a.n) return;
    long long row[7] = {-1, 0, 0, 0, 0, 0, 0};
    int id = -1, x = 0, y = 0, w = 0, h = 0;
    bool ok = b < a.rows;
    if (ok) {
        if (a.regions != nullptr) {
            const int* r = a.regions + 5 * (size_t)b;
            id = r[0]; x = r[1]; y = r[2]; w = r[3]; h = r[4];
        } else {
            id = a.m == 1 ? 0 : b; w = a.src_w; h = a.src_h;
        }
        ok = id >= 0 && id < a.m && w >= 1 && w <= kExtent && h >= 1 && h <= kExtent;
    }
    if (ok) {
        const float* u = a.points + 2 * (size_t)a.k * (size_t)b;
        const double xd = (double)x, yd = (double)y, wd = (double)w, hd = (double)h, kd = (double)a.k;
        // the means, and the finite check of the 2 k values
        double sx = 0.0, sy = 0.0;
        for (int i = 0; i < a.k; ++i) {
            const float ux = u[2 * i], uy = u[2 * i + 1];
            ok = ok && finite_f(ux) && finite_f(uy);
            const double px = (xd + (double)ux * wd) - 0.5, py = (yd + (double)uy * hd) - 0.5;
            sx = i == 0 ? px : sx + px;
            sy = i == 0 ? py : sy + py;
        }
        if (ok) {
            const double mx = sx / kd, my = sy / kd;
            const double tbx = a.tmpl[0], tby = a.tmpl[1], S = a.tmpl[2];
            double A = 0.0, B = 0.0;
            for (int i = 0; i < a.k; ++i) {
                const double px = (xd + (double)u[2 * i] * wd) - 0.5, py = (yd + (double)u[2 * i + 1] * hd) - 0.5;   // (the same bits as above)
                const double dx = px - mx, dy = py - my;
                const double cx = a.tmpl[3 + 2 * i], cy = a.tmpl[4 + 2 * i];
                const double ta = cx * dx + cy * dy, tb = cx * dy - cy * dx;
                A = i == 0 ? ta : A + ta;
                B = i == 0 ? tb : B + tb;
            }
            const double sa = A / S, sb = B / S;
            const double c0 = mx - (sa * tbx - sb * tby), c1 = my - (sb * tbx + sa * tby);
            const double q[6] = {sa * kQ16, -sb * kQ16, c0 * kQ16, sb * kQ16, sa * kQ16, c1 * kQ16};
            double r[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                r[j] = __builtin_rint(q[j]);                                   // ties to even
                const double limit = (j == 2 || j == 5) ? kTranslate : kLinear;
                ok = ok && finite_d(q[j]) && r[j] >= -limit && r[j] <= limit;   // (a NaN fails both compares)
            }
            ok = ok && !(r[0] == 0.0 && r[3] == 0.0);                          // every point in one place
            if (ok) {
                row[0] = id;
#pragma unroll
                for (int j = 0; j < 6; ++j) row[1 + j] = (long long)r[j];      // (|r| <= 2^40: exact)
            }
        }
    }
    long long* out = a.table + 7 * (size_t)b;
#pragma unroll
    for (int j = 0; j < 7; ++j) out[j] = row[j];
    a.valid[b] = ok ? 1 : 0;
}

// one wave: count = sum of valid[0..n)
__global__ __launch_bounds__(kWave) void landmarks_count_kernel(int* valid, int n) {
    int sum = 0;
    for (int i = threadIdx.x; i < n; i += kWave) sum += valid[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, kWave);
    if (threadIdx.x == 0) valid[n] = sum;
}

}  // namespace

extern "C" {

int pvhip_landmarks_to_warps(const float* points, const int* regions, const double* tmpl, long long* table, int* valid, int n, int rows,
                             int k, int m, int src_h, int src_w) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(points != nullptr && tmpl != nullptr && table != nullptr && valid != nullptr);
    PVHIP_CHECK_ARG(((uintptr_t)points & 3u) == 0 && ((uintptr_t)regions & 3u) == 0 && ((uintptr_t)valid & 3u) == 0);
    PVHIP_CHECK_ARG(((uintptr_t)tmpl & 7u) == 0 && ((uintptr_t)table & 7u) == 0);
    PVHIP_CHECK_ARG(n >= 1 && rows >= 1 && k >= 2 && k <= 32 && m >= 1);
    PVHIP_CHECK_ARG(src_h >= 1 && src_h <= kExtent && src_w >= 1 && src_w <= kExtent);
    const LandmarkArgs a{points, regions, tmpl, table, valid, n, rows, k, m, src_h, src_w};
    hipLaunchKernelGGL(landmarks_to_warps_kernel, dim3((n + kWave - 1) / kWave), dim3(kWave), 0, state().stream, a);
    hipLaunchKernelGGL(landmarks_count_kernel, dim3(1), dim3(kWave), 0, state().stream, valid, n);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
