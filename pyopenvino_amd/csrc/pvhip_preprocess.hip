// Input preprocessing (HBM-bound): the staged host input of a request -- a U8 or FP32 image of any extent, NHWC or NCHW -- becomes the
// fp32 NCHW tensor the network's Parameter expects, in ONE launch: bilinear resize, channel reversal, per-channel mean / scale and the
// layout change (IENetwork.input_info[name].preprocess_info).
//
// Resize: half-pixel centres clamped at the border, no antialiasing (cv2 INTER_LINEAR, torch interpolate bilinear with
// align_corners=False).  The source coordinate of destination index d is num / (2D) with num = max((2d+1)S - D, 0), computed exactly in
// 64-bit integers; i0 = min(num / 2D, S-1), i1 = min(i0+1, S-1), f = (num - 2D i0) / 2D as ONE correctly rounded fp32 division (0 at
// the last source index).  v = (1-fy)((1-fx)p00 + fx p01) + fy((1-fx)p10 + fx p11) in fp32, in that order, never contracted to fma.
// Then y = (v - mean[c]) / std_scale[c], output channel c reading source channel C-1-c under reversal.  tests/preprocess_ref.py is the
// same rule in numpy; the kernel matches it bit for bit.
//
// A workgroup owns a tile of `th` output rows x `tw` output columns of one image (normally whole rows).  It
//   1. tabulates the tile's column and row coordinates (x0, x1, fx), (y0, y1, fy) in LDS;
//   2. stages the source it reads -- per channel plane (NCHW) or for all channels at once (NHWC), the rows y0(first)..y1(last), each the
//      contiguous span of columns x0(first)..x1(last) -- into LDS with 16-byte loads; every span keeps its address modulo 16 in LDS, so
//      any source alignment takes the wide loads, with byte-wise head and tail;
//   3. has every lane produce 4 consecutive output pixels of one row, for every channel, stored as float4 nontemporal stores into each
//      channel plane (scalar stores when the destination rows are not 16-byte aligned).
#include "pvhip_common.h"

#pragma clang fp contract(off)

using namespace pvhip;

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));

constexpr size_t kStageBudget = 48 * 1024;   // LDS per workgroup at most (three workgroups per CU)
constexpr int    kMaxChannels = 1024;        // the smallest tile of an NHWC source still fits the budget

struct Tap {
    int i0, i1;
    float f;
};

// Source taps of destination index d along an axis of source extent S, destination extent D (see the file comment).
template <bool RESIZE>
__device__ __forceinline__ Tap tap(int d, int S, int D) {
    Tap t;
    if (!RESIZE) {
        t.i0 = t.i1 = d;
        t.f = 0.0f;
        return t;
    }
    const long long two_d = 2LL * D;
    long long num = (2LL * d + 1) * S - D;
    if (num < 0) num = 0;
    long long i0 = num / two_d;
    if (i0 > S - 1) i0 = S - 1;
    t.i0 = (int)i0;
    t.i1 = (int)(i0 + 1 < S ? i0 + 1 : S - 1);
    t.f = i0 == S - 1 ? 0.0f : (float)(num - i0 * two_d) / (float)two_d;
    return t;
}

struct PrepArgs {
    const unsigned char* src;
    float* dst;
    const float* mean;        // NULL: no mean
    const float* std_scale;   // NULL: no scale
    int c, hs, ws, hd, wd, tw, th;
    int nhwc, reverse;
    unsigned slot;            // LDS bytes per staged span (a multiple of 16)
    unsigned stage_bytes;     // LDS bytes of the staging area (the coordinate tables follow it)
};

template <bool U8>
__device__ __forceinline__ float pixel(const unsigned char* span, int e) {
    if (U8) return (float)span[e];
    return reinterpret_cast<const float*>(span)[e];
}

__device__ __forceinline__ void stg4_nt(float* p, const float (&v)[4]) {
    f4v w;
    w.x = v[0]; w.y = v[1]; w.z = v[2]; w.w = v[3];
    __builtin_nontemporal_store(w, reinterpret_cast<f4v*>(p));
}

// grid (ceil(wd / tw), ceil(hd / th), n); dynamic LDS stage_bytes + 12 (tw + th) bytes.
// VS: every tile's quads start 16-byte aligned in every output plane (dst aligned, wd and tw multiples of 4).
template <bool U8, bool RESIZE, bool VS>
__global__ __launch_bounds__(kBlock) void preprocess_kernel(PrepArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int ES = U8 ? 1 : 4;
    const int n = blockIdx.z, tx0 = blockIdx.x * a.tw, ty0 = blockIdx.y * a.th;
    const int twv = min(a.tw, a.wd - tx0), thv = min(a.th, a.hd - ty0);
    int* cx0 = reinterpret_cast<int*>(lds + a.stage_bytes);
    int* cx1 = cx0 + a.tw;
    float* cfx = reinterpret_cast<float*>(cx1 + a.tw);
    int* ry0 = reinterpret_cast<int*>(cfx + a.tw);
    int* ry1 = ry0 + a.th;
    float* rfy = reinterpret_cast<float*>(ry1 + a.th);
    for (int j = threadIdx.x; j < twv; j += kBlock) {
        const Tap t = tap<RESIZE>(tx0 + j, a.ws, a.wd);
        cx0[j] = t.i0; cx1[j] = t.i1; cfx[j] = t.f;
    }
    for (int j = threadIdx.x; j < thv; j += kBlock) {
        const Tap t = tap<RESIZE>(ty0 + j, a.hs, a.hd);
        ry0[j] = t.i0; ry1[j] = t.i1; rfy[j] = t.f;
    }
    // the source the tile reads (the taps are monotone in d): columns xs0..xs1 of rows ys0..ys1
    const int xs0 = tap<RESIZE>(tx0, a.ws, a.wd).i0, xs1 = tap<RESIZE>(tx0 + twv - 1, a.ws, a.wd).i1;
    const int ys0 = tap<RESIZE>(ty0, a.hs, a.hd).i0, ys1 = tap<RESIZE>(ty0 + thv - 1, a.hs, a.hd).i1;
    const int rows = ys1 - ys0 + 1;
    const int cs = a.nhwc ? a.c : 1, planes = a.nhwc ? 1 : a.c;
    const int span = (xs1 - xs0 + 1) * cs * ES;              // bytes of one staged span
    // span s = plane * rows + row: its first byte in the source
    auto span_src = [&](int s) -> const unsigned char* {
        const int p = s / rows, r = s - p * rows;
        const size_t e = a.nhwc ? ((size_t)n * a.hs + ys0 + r) * a.ws * (size_t)a.c + (size_t)xs0 * a.c
                                : (((size_t)n * a.c + p) * a.hs + ys0 + r) * a.ws + xs0;
        return a.src + e * ES;
    };
    const unsigned bps = (unsigned)span / 16 + 2;             // 16-byte blocks a span touches at most
    const unsigned nblk = (unsigned)(planes * rows) * bps;
    for (unsigned i = threadIdx.x; i < nblk; i += kBlock) {
        const unsigned s = i / bps, k = i - s * bps;
        const unsigned char* g = span_src((int)s);
        const int sh = (int)((uintptr_t)g & 15);
        const int lo = 16 * (int)k - sh;                      // the block's first byte, relative to the span's
        const unsigned char* b = g + lo;
        unsigned char* l = lds + s * a.slot + 16 * k;         // the span's byte j lies at s * slot + sh + j
        if (lo >= 0 && lo + 16 <= span) {
            *reinterpret_cast<u4v*>(l) = *reinterpret_cast<const u4v*>(b);
        } else {
            for (int t = lo < 0 ? -lo : 0; t < 16 && lo + t < span; ++t) l[t] = b[t];
        }
    }
    __syncthreads();

    const int nq = (twv + 3) >> 2;
    const size_t plane_out = (size_t)a.hd * a.wd;
    float* out_n = a.dst + (size_t)n * a.c * plane_out;
    for (int i = threadIdx.x; i < thv * nq; i += kBlock) {
        const int r = i / nq, j0 = 4 * (i - r * nq);
        const int y0 = ry0[r] - ys0, y1 = ry1[r] - ys0;
        const float fy = rfy[r], gy = 1.0f - fy;
        int xa[4], xb[4];
        float fx[4], gx[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u < twv ? j0 + u : j0;         // (a pixel past the tile computes column j0 again and is not stored)
            xa[u] = (cx0[j] - xs0) * cs;
            xb[u] = (cx1[j] - xs0) * cs;
            fx[u] = cfx[j];
            gx[u] = 1.0f - fx[u];
        }
        float* o = out_n + (size_t)(ty0 + r) * a.wd + tx0 + j0;
        for (int oc = 0; oc < a.c; ++oc, o += plane_out) {
            const int sc = a.reverse ? a.c - 1 - oc : oc;
            const int s0 = (a.nhwc ? 0 : sc) * rows + y0, s1 = (a.nhwc ? 0 : sc) * rows + y1;
            const unsigned char* l0 = lds + (unsigned)s0 * a.slot + ((uintptr_t)span_src(s0) & 15);
            const unsigned char* l1 = lds + (unsigned)s1 * a.slot + ((uintptr_t)span_src(s1) & 15);
            const int ch = a.nhwc ? sc : 0;
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (RESIZE) {
                    const float top = gx[u] * pixel<U8>(l0, xa[u] + ch) + fx[u] * pixel<U8>(l0, xb[u] + ch);
                    const float bot = gx[u] * pixel<U8>(l1, xa[u] + ch) + fx[u] * pixel<U8>(l1, xb[u] + ch);
                    v[u] = gy * top + fy * bot;
                } else {
                    v[u] = pixel<U8>(l0, xa[u] + ch);
                }
            }
            if (a.mean != nullptr) {
                const float m = a.mean[oc];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = v[u] - m;
            }
            if (a.std_scale != nullptr) {
                const float d = a.std_scale[oc];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = v[u] / d;
            }
            if (VS && j0 + 3 < twv) {
                stg4_nt(o, v);
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (j0 + u < twv) o[u] = v[u];
            }
        }
    }
}

template <bool U8, bool RESIZE>
void launch(const PrepArgs& a, dim3 grid, size_t lds, bool vs, hipStream_t st) {
    if (vs) hipLaunchKernelGGL((preprocess_kernel<U8, RESIZE, true>), grid, dim3(kBlock), lds, st, a);
    else    hipLaunchKernelGGL((preprocess_kernel<U8, RESIZE, false>), grid, dim3(kBlock), lds, st, a);
}

}  // namespace

extern "C" {

int pvhip_input_preprocess_f32(const void* src, float* dst, int n, int c, int src_h, int src_w, int dst_h, int dst_w,
                               int src_u8, int src_nhwc, int reverse_channels, const float* mean, const float* std_scale) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(src != nullptr && dst != nullptr);
    PVHIP_CHECK_ARG(n > 0 && n <= 65535 && c > 0 && c <= kMaxChannels && src_h > 0 && src_w > 0 && dst_h > 0 && dst_w > 0);
    PVHIP_CHECK_ARG((size_t)src_h * (size_t)src_w * (size_t)c < ((size_t)1 << 31));   // one image's elements index in 32 bits
    PVHIP_CHECK_ARG((size_t)dst_h * (size_t)dst_w * (size_t)c < ((size_t)1 << 31));
    PVHIP_CHECK_ARG(src_u8 || (uintptr_t)src % 4 == 0);                              // fp32 sources are element-aligned
    const bool resize = src_h != dst_h || src_w != dst_w;
    if (!resize && !reverse_channels && mean == nullptr && std_scale == nullptr)      // the format alone: the same bits as the
        return pvhip_input_to_nchw_f32(src, dst, n, c, dst_h, dst_w, src_u8, src_nhwc);   // path without preprocessing
    const size_t es = src_u8 ? 1 : 4;
    const size_t cs = src_nhwc ? (size_t)c : 1, planes = src_nhwc ? 1 : (size_t)c;
    // source rows (columns) a tile of t destination rows (columns) reads at most: the taps advance by S/D per step
    auto extent = [&](int t, int S, int D) -> size_t {
        if (!resize) return (size_t)t;
        const size_t e = ((size_t)(t - 1) * (size_t)S + (size_t)D - 1) / (size_t)D + 2;
        return e < (size_t)S ? e : (size_t)S;
    };
    auto slot_of = [&](int tw) { return (extent(tw, src_w, dst_w) * cs * es + 30) / 16 * 16; };
    auto stage_of = [&](int tw, int th) { return planes * extent(th, src_h, dst_h) * slot_of(tw); };
    auto lds_of = [&](int tw, int th) { return stage_of(tw, th) + 12 * ((size_t)tw + (size_t)th); };
    int tw = dst_w;                        // whole rows, unless one row's sources do not fit
    while (tw > 1 && lds_of(tw, 1) > kStageBudget) tw = tw > 4 ? (((tw + 1) / 2 + 3) & ~3) : tw - 1;
    int th = 2 * kBlock / ((tw + 3) / 4);  // about two quads per lane
    th = th < 1 ? 1 : (th > dst_h ? dst_h : th);
    while (th > 1 && lds_of(tw, th) > kStageBudget) th = (th + 1) / 2;
    PVHIP_CHECK_ARG(lds_of(tw, th) <= kStageBudget);
    const dim3 grid((unsigned)((dst_w + tw - 1) / tw), (unsigned)((dst_h + th - 1) / th), (unsigned)n);
    PVHIP_CHECK_ARG(grid.y <= 65535);
    PrepArgs a;
    a.src = (const unsigned char*)src; a.dst = dst; a.mean = mean; a.std_scale = std_scale;
    a.c = c; a.hs = src_h; a.ws = src_w; a.hd = dst_h; a.wd = dst_w; a.tw = tw; a.th = th;
    a.nhwc = src_nhwc ? 1 : 0; a.reverse = reverse_channels ? 1 : 0;
    a.slot = (unsigned)slot_of(tw); a.stage_bytes = (unsigned)stage_of(tw, th);
    const bool vs = (uintptr_t)dst % 16 == 0 && dst_w % 4 == 0 && tw % 4 == 0;
    const size_t lds = lds_of(tw, th);
    hipStream_t st = state().stream;
    if (src_u8) resize ? launch<true, true>(a, grid, lds, vs, st) : launch<true, false>(a, grid, lds, vs, st);
    else        resize ? launch<false, true>(a, grid, lds, vs, st) : launch<false, false>(a, grid, lds, vs, st);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
