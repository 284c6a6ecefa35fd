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
//
// YUV 4:2:0 frames (NV12, I420) take the same launch with a colour conversion in front of the taps: preprocess_yuv_kernel, further down.
//
// Regions of interest (the ROI entries): image b of the output is the rectangle rois[b] = (id, x, y, w, h) of frame id of m frames, cropped
// and then resized -- the taps clamp at the rectangle's edge, not the frame's.  Both kernels take it as a template parameter: a workgroup
// reads its image's five ints, takes S = (h, w) for its taps and adds (id, y, x) to the addresses it stages from; a rectangle of exactly
// the destination's extent is copied (fp32 sources: no 0 * inf; bytes give the same bits either way).  The table is device data, so an image whose rectangle does not lie inside a frame, or
// exceeds the maxima the launch was sized for, is written as quiet NaN and nothing is read for it.  tests/roi_ref.py is the rule in numpy.
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
    const int* rois;          // ROI kernels: n x (id, x, y, w, h); hs, ws are then the extent of each of the m frames
    int m, mh, mw;            // ... the frame count and the largest h and w the launch was sized for
};

// One image's rectangle (ROI kernels), read once per workgroup; ok: it lies inside frame id and within the launch's maxima.
struct Roi {
    int id, x, y, w, h;
    bool ok;
};

__device__ __forceinline__ Roi roi_of(const int* rois, int b, int m, int hs, int ws, int mh, int mw) {
    const int* q = rois + 5 * (size_t)b;
    Roi r;
    r.id = q[0]; r.x = q[1]; r.y = q[2]; r.w = q[3]; r.h = q[4];
    r.ok = r.id >= 0 && r.id < m && r.x >= 0 && r.y >= 0 && r.w >= 1 && r.h >= 1 && r.w <= mw && r.h <= mh
        && (long long)r.x + r.w <= ws && (long long)r.y + r.h <= hs;
    return r;
}

// The tile (tx0.., ty0..) of twv x thv pixels in every one of c planes of one image: quiet NaN (an invalid rectangle).
__device__ __forceinline__ void fill_nan(float* out_n, int c, size_t plane_out, int wd, int tx0, int ty0, int twv, int thv) {
    const float q = __builtin_nanf("");
    for (int oc = 0; oc < c; ++oc)
        for (int i = threadIdx.x; i < thv * twv; i += kBlock) {
            const int r = i / twv;
            out_n[oc * plane_out + (size_t)(ty0 + r) * wd + tx0 + (i - r * twv)] = q;
        }
}

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
// ROI (with RESIZE): image n is a rectangle of a frame (see the file comment); hs, ws below are the extent the taps see.
template <bool U8, bool RESIZE, bool VS, bool ROI>
__global__ __launch_bounds__(kBlock) void preprocess_kernel(PrepArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int ES = U8 ? 1 : 4;
    const int n = blockIdx.z, tx0 = blockIdx.x * a.tw, ty0 = blockIdx.y * a.th;
    const int twv = min(a.tw, a.wd - tx0), thv = min(a.th, a.hd - ty0);
    int hs = a.hs, ws = a.ws, img = n, ox = 0, oy = 0;
    bool copy = false;                                        // (workgroup-uniform) the rectangle has the destination's extent
    if (ROI) {
        const Roi q = roi_of(a.rois, n, a.m, a.hs, a.ws, a.mh, a.mw);
        if (!q.ok) {
            fill_nan(a.dst + (size_t)n * a.c * ((size_t)a.hd * a.wd), a.c, (size_t)a.hd * a.wd, a.wd, tx0, ty0, twv, thv);
            return;
        }
        hs = q.h; ws = q.w; img = q.id; ox = q.x; oy = q.y;
        copy = !U8 && q.h == a.hd && q.w == a.wd;             // (bytes interpolate to the same bits: weight 0 on a finite value)
    }
    auto taps = [&](int d, int S, int D) { return ROI && copy ? tap<false>(d, S, D) : tap<RESIZE>(d, S, D); };
    int* cx0 = reinterpret_cast<int*>(lds + a.stage_bytes);
    int* cx1 = cx0 + a.tw;
    float* cfx = reinterpret_cast<float*>(cx1 + a.tw);
    int* ry0 = reinterpret_cast<int*>(cfx + a.tw);
    int* ry1 = ry0 + a.th;
    float* rfy = reinterpret_cast<float*>(ry1 + a.th);
    for (int j = threadIdx.x; j < twv; j += kBlock) {
        const Tap t = taps(tx0 + j, ws, a.wd);
        cx0[j] = t.i0; cx1[j] = t.i1; cfx[j] = t.f;
    }
    for (int j = threadIdx.x; j < thv; j += kBlock) {
        const Tap t = taps(ty0 + j, hs, a.hd);
        ry0[j] = t.i0; ry1[j] = t.i1; rfy[j] = t.f;
    }
    // the source the tile reads (the taps are monotone in d): columns xs0..xs1 of rows ys0..ys1
    const int xs0 = taps(tx0, ws, a.wd).i0, xs1 = taps(tx0 + twv - 1, ws, a.wd).i1;
    const int ys0 = taps(ty0, hs, a.hd).i0, ys1 = taps(ty0 + thv - 1, hs, a.hd).i1;
    const int rows = ys1 - ys0 + 1;
    const int cs = a.nhwc ? a.c : 1, planes = a.nhwc ? 1 : a.c;
    const int span = (xs1 - xs0 + 1) * cs * ES;              // bytes of one staged span
    // span s = plane * rows + row: its first byte in the source
    auto span_src = [&](int s) -> const unsigned char* {
        const int p = s / rows, r = s - p * rows;
        const size_t e = a.nhwc ? ((size_t)img * a.hs + oy + ys0 + r) * a.ws * (size_t)a.c + (size_t)(ox + xs0) * a.c
                                : (((size_t)img * a.c + p) * a.hs + oy + ys0 + r) * a.ws + ox + xs0;
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
                if (RESIZE && !(ROI && copy)) {
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

template <bool U8, bool RESIZE, bool ROI>
void launch(const PrepArgs& a, dim3 grid, size_t lds, bool vs, hipStream_t st) {
    if (vs) hipLaunchKernelGGL((preprocess_kernel<U8, RESIZE, true, ROI>), grid, dim3(kBlock), lds, st, a);
    else    hipLaunchKernelGGL((preprocess_kernel<U8, RESIZE, false, ROI>), grid, dim3(kBlock), lds, st, a);
}

// ---------------------------------------------------------------------------------------------------------------- YUV 4:2:0 sources
// A decoder's frame -- uint8, 3 h / 2 rows of w bytes per image: the Y plane, then NV12's h/2 rows of w/2 (U, V) pairs or I420's U plane
// and V plane of h/2 x w/2 bytes each -- converted to B, G, R by the BT.601 limited-range rule in 20-bit fixed point
//   t = max(Y - 16, 0) * 1220542 + 2^19,  R = (t + 1673527 (V - 128)) >> 20,  G = (t - 852492 (V - 128) - 409993 (U - 128)) >> 20,
//   B = (t + 2116026 (U - 128)) >> 20  (arithmetic shifts), each clamped to [0, 255],
// with the (U, V) of the pixel's 2 x 2 block (no chroma interpolation); the uint8 image that gives is then resized, reversed and scaled
// exactly as a U8 NHWC source is above.  tests/yuv_ref.py is the conversion in numpy; every intermediate stays within +-5.7e8.
//
// The kernel has preprocess_kernel's shape.  A tile stages the Y spans it reads and, behind them, the chroma spans under them: rows
// ys0/2..ys1/2, of each the pairs xs0/2..xs1/2 of the ABSOLUTE columns (a tile may start on an odd column) -- one span per row for NV12,
// one in each plane for I420.  A pixel is converted where it is tapped, so a downscale converts four pixels per output pixel however
// many it staged, and the three channels of a quad come from one pass over its taps.
struct YuvArgs {
    const unsigned char* src;
    float* dst;
    const float* mean;        // NULL: no mean
    const float* std_scale;   // NULL: no scale
    int hs, ws, hd, wd, tw, th;
    int planar, reverse;
    unsigned yslot, cslot;    // LDS bytes per staged Y span and per staged chroma span (multiples of 16)
    unsigned stage_bytes;     // LDS bytes of the staging area (the coordinate tables follow it)
    const int* rois;          // ROI kernels: as in PrepArgs
    int m, mh, mw;
};

// B, G, R (in that order) of one pixel, as the floats of the converted bytes.
__device__ __forceinline__ void yuv_to_bgr(int y, int u, int v, float (&o)[3]) {
    y = y - 16 < 0 ? 0 : y - 16;
    u -= 128; v -= 128;
    const int t = y * 1220542 + (1 << 19);
    const int b = (t + 2116026 * u) >> 20;
    const int g = (t - 852492 * v - 409993 * u) >> 20;
    const int r = (t + 1673527 * v) >> 20;
    o[0] = (float)min(max(b, 0), 255);
    o[1] = (float)min(max(g, 0), 255);
    o[2] = (float)min(max(r, 0), 255);
}

// grid (ceil(wd / tw), ceil(hd / th), n); dynamic LDS stage_bytes + 12 (tw + th) bytes.  VS as in preprocess_kernel.
// ROI as in preprocess_kernel; the chroma of a pixel is that of its ABSOLUTE 2 x 2 block of the frame, so a rectangle may start on odd
// coordinates and have odd sizes.
template <bool RESIZE, bool VS, bool ROI>
__global__ __launch_bounds__(kBlock) void preprocess_yuv_kernel(YuvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int n = blockIdx.z, tx0 = blockIdx.x * a.tw, ty0 = blockIdx.y * a.th;
    const int twv = min(a.tw, a.wd - tx0), thv = min(a.th, a.hd - ty0);
    int hs = a.hs, ws = a.ws, img = n, ox = 0, oy = 0;
    if (ROI) {
        const Roi q = roi_of(a.rois, n, a.m, a.hs, a.ws, a.mh, a.mw);
        if (!q.ok) {
            fill_nan(a.dst + (size_t)n * 3 * ((size_t)a.hd * a.wd), 3, (size_t)a.hd * a.wd, a.wd, tx0, ty0, twv, thv);
            return;
        }
        hs = q.h; ws = q.w; img = q.id; ox = q.x; oy = q.y;
    }
    // (a rectangle of the destination's extent needs no copy path here: the converted pixels are bytes, and weight 0 on a finite value
    // interpolates to the same bits)
    auto taps = [&](int d, int S, int D) { return tap<RESIZE>(d, S, D); };
    int* cx0 = reinterpret_cast<int*>(lds + a.stage_bytes);
    int* cx1 = cx0 + a.tw;
    float* cfx = reinterpret_cast<float*>(cx1 + a.tw);
    int* ry0 = reinterpret_cast<int*>(cfx + a.tw);
    int* ry1 = ry0 + a.th;
    float* rfy = reinterpret_cast<float*>(ry1 + a.th);
    for (int j = threadIdx.x; j < twv; j += kBlock) {
        const Tap t = taps(tx0 + j, ws, a.wd);
        cx0[j] = t.i0; cx1[j] = t.i1; cfx[j] = t.f;
    }
    for (int j = threadIdx.x; j < thv; j += kBlock) {
        const Tap t = taps(ty0 + j, hs, a.hd);
        ry0[j] = t.i0; ry1[j] = t.i1; rfy[j] = t.f;
    }
    const int xs0 = taps(tx0, ws, a.wd).i0, xs1 = taps(tx0 + twv - 1, ws, a.wd).i1;
    const int ys0 = taps(ty0, hs, a.hd).i0, ys1 = taps(ty0 + thv - 1, hs, a.hd).i1;
    const int rows = ys1 - ys0 + 1, yspan = xs1 - xs0 + 1;
    const int ps0 = (ox + xs0) >> 1, cr0 = (oy + ys0) >> 1, crows = ((oy + ys1) >> 1) - cr0 + 1;   // first chroma pair and row, chroma rows
    const int cstep = a.planar ? 1 : 2;                                            // bytes from one U (V) to the next
    const int cspan = (((ox + xs1) >> 1) - ps0 + 1) * cstep;
    const int hw = a.ws >> 1;
    const unsigned char* frame = a.src + (size_t)img * ((size_t)a.hs * a.ws / 2 * 3);
    const unsigned char* chroma = frame + (size_t)a.hs * a.ws;
    auto y_src = [&](int r) -> const unsigned char* { return frame + (size_t)(oy + ys0 + r) * a.ws + ox + xs0; };
    // chroma span s: NV12 row s of the pairs; I420 row s of U for s < crows, row s - crows of V after them
    auto c_src = [&](int s) -> const unsigned char* {
        if (!a.planar) return chroma + (size_t)(cr0 + s) * a.ws + 2 * ps0;
        const int p = s >= crows ? 1 : 0;
        return chroma + ((size_t)p * (a.hs >> 1) + cr0 + s - p * crows) * hw + ps0;
    };
    unsigned char* lds_c = lds + (unsigned)rows * a.yslot;
    // one 16-byte block k of a span of `span` bytes at g, into its slot at l (byte j of the span lies at l + (g & 15) + j)
    auto stage = [&](const unsigned char* g, int span, unsigned char* l, unsigned k) {
        const int lo = 16 * (int)k - (int)((uintptr_t)g & 15);
        const unsigned char* b = g + lo;
        l += 16 * k;
        if (lo >= 0 && lo + 16 <= span) {
            *reinterpret_cast<u4v*>(l) = *reinterpret_cast<const u4v*>(b);
        } else {
            for (int t = lo < 0 ? -lo : 0; t < 16 && lo + t < span; ++t) l[t] = b[t];
        }
    };
    const unsigned ybps = (unsigned)yspan / 16 + 2, cbps = (unsigned)cspan / 16 + 2;
    const unsigned yblk = (unsigned)rows * ybps, cblk = (unsigned)(crows * (a.planar ? 2 : 1)) * cbps;
    for (unsigned i = threadIdx.x; i < yblk + cblk; i += kBlock) {
        if (i < yblk) {
            const unsigned s = i / ybps;
            stage(y_src((int)s), yspan, lds + s * a.yslot, i - s * ybps);
        } else {
            const unsigned s = (i - yblk) / cbps;
            stage(c_src((int)s), cspan, lds_c + s * a.cslot, i - yblk - s * cbps);
        }
    }
    __syncthreads();

    const int nq = (twv + 3) >> 2;
    const size_t plane_out = (size_t)a.hd * a.wd;
    float* out_n = a.dst + (size_t)n * 3 * plane_out;
    for (int i = threadIdx.x; i < thv * nq; i += kBlock) {
        const int r = i / nq, j0 = 4 * (i - r * nq);
        const float fy = rfy[r], gy = 1.0f - fy;
        // the two tapped rows: their Y spans, and the U and V of the chroma rows under them
        const unsigned char *ly[2], *lu[2], *lv[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int ya = k ? ry1[r] : ry0[r];
            const int yr = ya - ys0, cr = ((oy + ya) >> 1) - cr0;
            ly[k] = lds + (unsigned)yr * a.yslot + ((uintptr_t)y_src(yr) & 15);
            lu[k] = lds_c + (unsigned)cr * a.cslot + ((uintptr_t)c_src(cr) & 15);
            lv[k] = a.planar ? lds_c + (unsigned)(crows + cr) * a.cslot + ((uintptr_t)c_src(crows + cr) & 15) : lu[k] + 1;
        }
        float v[3][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u < twv ? j0 + u : j0;         // (a pixel past the tile computes column j0 again and is not stored)
            const int xa = cx0[j], xb = cx1[j];
            const int pa = (((ox + xa) >> 1) - ps0) * cstep, pb = (((ox + xb) >> 1) - ps0) * cstep;
            float p00[3];
            yuv_to_bgr(ly[0][xa - xs0], lu[0][pa], lv[0][pa], p00);
            if (RESIZE) {
                const float fx = cfx[j], gx = 1.0f - fx;
                float p01[3], p10[3], p11[3];
                yuv_to_bgr(ly[0][xb - xs0], lu[0][pb], lv[0][pb], p01);
                yuv_to_bgr(ly[1][xa - xs0], lu[1][pa], lv[1][pa], p10);
                yuv_to_bgr(ly[1][xb - xs0], lu[1][pb], lv[1][pb], p11);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float top = gx * p00[c] + fx * p01[c];
                    const float bot = gx * p10[c] + fx * p11[c];
                    v[c][u] = gy * top + fy * bot;
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][u] = p00[c];
            }
        }
        float* o = out_n + (size_t)(ty0 + r) * a.wd + tx0 + j0;
#pragma unroll
        for (int oc = 0; oc < 3; ++oc, o += plane_out) {
            float w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) w[u] = a.reverse ? v[2 - oc][u] : v[oc][u];
            if (a.mean != nullptr) {
                const float m = a.mean[oc];
#pragma unroll
                for (int u = 0; u < 4; ++u) w[u] = w[u] - m;
            }
            if (a.std_scale != nullptr) {
                const float d = a.std_scale[oc];
#pragma unroll
                for (int u = 0; u < 4; ++u) w[u] = w[u] / d;
            }
            if (VS && j0 + 3 < twv) {
                stg4_nt(o, w);
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (j0 + u < twv) o[u] = w[u];
            }
        }
    }
}

template <bool RESIZE, bool ROI>
void launch_yuv(const YuvArgs& a, dim3 grid, size_t lds, bool vs, hipStream_t st) {
    if (vs) hipLaunchKernelGGL((preprocess_yuv_kernel<RESIZE, true, ROI>), grid, dim3(kBlock), lds, st, a);
    else    hipLaunchKernelGGL((preprocess_yuv_kernel<RESIZE, false, ROI>), grid, dim3(kBlock), lds, st, a);
}

// The one launcher of preprocess_kernel.  rois == NULL: image b is the whole of source image b (m, roi_h, roi_w are not read).  Else image
// b is a rectangle of one of m frames; the tiles and LDS slots are sized for the largest rectangle (roi_h, roi_w): extent() is monotone
// in S, so the budget holds for every image.
int preprocess_launch(const void* src, float* dst, const int* rois, int n, int m, int c, int src_h, int src_w, int dst_h, int dst_w,
                      int roi_h, int roi_w, int src_u8, int src_nhwc, int reverse_channels, const float* mean, const float* std_scale) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(src != nullptr && dst != nullptr);
    PVHIP_CHECK_ARG(n > 0 && n <= 65535 && c > 0 && c <= kMaxChannels && src_h > 0 && src_w > 0 && dst_h > 0 && dst_w > 0);
    PVHIP_CHECK_ARG((size_t)src_h * (size_t)src_w * (size_t)c < ((size_t)1 << 31));   // one image's elements index in 32 bits
    PVHIP_CHECK_ARG((size_t)dst_h * (size_t)dst_w * (size_t)c < ((size_t)1 << 31));
    PVHIP_CHECK_ARG(src_u8 || (uintptr_t)src % 4 == 0);                              // fp32 sources are element-aligned
    const bool roi = rois != nullptr;
    if (roi) PVHIP_CHECK_ARG(m >= 1 && roi_h >= 1 && roi_h <= src_h && roi_w >= 1 && roi_w <= src_w);
    const bool resize = roi || src_h != dst_h || src_w != dst_w;
    if (!resize && !reverse_channels && mean == nullptr && std_scale == nullptr)      // the format alone: the same bits as the
        return pvhip_input_to_nchw_f32(src, dst, n, c, dst_h, dst_w, src_u8, src_nhwc);   // path without preprocessing
    const int tap_h = roi ? roi_h : src_h, tap_w = roi ? roi_w : src_w;               // the largest extent the taps of an image see
    const size_t es = src_u8 ? 1 : 4;
    const size_t cs = src_nhwc ? (size_t)c : 1, planes = src_nhwc ? 1 : (size_t)c;
    // source rows (columns) a tile of t destination rows (columns) reads at most: the taps advance by S/D per step
    auto extent = [&](int t, int S, int D) -> size_t {
        if (!resize) return (size_t)t;
        const size_t e = ((size_t)(t - 1) * (size_t)S + (size_t)D - 1) / (size_t)D + 2;
        return e < (size_t)S ? e : (size_t)S;
    };
    auto slot_of = [&](int tw) { return (extent(tw, tap_w, dst_w) * cs * es + 30) / 16 * 16; };
    auto stage_of = [&](int tw, int th) { return planes * extent(th, tap_h, dst_h) * slot_of(tw); };
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
    a.rois = rois; a.m = m; a.mh = roi_h; a.mw = roi_w;
    const bool vs = (uintptr_t)dst % 16 == 0 && dst_w % 4 == 0 && tw % 4 == 0;
    const size_t lds = lds_of(tw, th);
    hipStream_t st = state().stream;
    if (roi)         src_u8 ? launch<true, true, true>(a, grid, lds, vs, st) : launch<false, true, true>(a, grid, lds, vs, st);
    else if (src_u8) resize ? launch<true, true, false>(a, grid, lds, vs, st) : launch<true, false, false>(a, grid, lds, vs, st);
    else             resize ? launch<false, true, false>(a, grid, lds, vs, st) : launch<false, false, false>(a, grid, lds, vs, st);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

// The one launcher of preprocess_yuv_kernel; rois, m, roi_h, roi_w as above.
int preprocess_yuv_launch(const void* src, float* dst, const int* rois, int n, int m, int src_h, int src_w, int dst_h, int dst_w,
                          int roi_h, int roi_w, int planar, int reverse_channels, const float* mean, const float* std_scale) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(src != nullptr && dst != nullptr);
    PVHIP_CHECK_ARG(n > 0 && n <= 65535 && src_h > 0 && src_w > 0 && dst_h > 0 && dst_w > 0);
    PVHIP_CHECK_ARG(src_h % 2 == 0 && src_w % 2 == 0);                               // 4:2:0: one (U, V) per 2 x 2 block
    PVHIP_CHECK_ARG(planar == 0 || planar == 1);
    PVHIP_CHECK_ARG((size_t)src_h * (size_t)src_w * 3 < ((size_t)1 << 31));           // one image's elements index in 32 bits
    PVHIP_CHECK_ARG((size_t)dst_h * (size_t)dst_w * 3 < ((size_t)1 << 31));
    const bool roi = rois != nullptr;
    if (roi) PVHIP_CHECK_ARG(m >= 1 && roi_h >= 1 && roi_h <= src_h && roi_w >= 1 && roi_w <= src_w);
    const bool resize = roi || src_h != dst_h || src_w != dst_w;
    const int tap_h = roi ? roi_h : src_h, tap_w = roi ? roi_w : src_w;
    auto extent = [&](int t, int S, int D) -> size_t {                                // as above
        if (!resize) return (size_t)t;
        const size_t e = ((size_t)(t - 1) * (size_t)S + (size_t)D - 1) / (size_t)D + 2;
        return e < (size_t)S ? e : (size_t)S;
    };
    // e consecutive rows (columns) lie over at most e / 2 + 1 chroma rows (pairs): the first may be an odd one
    auto halves = [](size_t e, int S) { return e / 2 + 1 < (size_t)S / 2 ? e / 2 + 1 : (size_t)S / 2; };
    auto yslot_of = [&](int tw) { return (extent(tw, tap_w, dst_w) + 30) / 16 * 16; };
    auto cslot_of = [&](int tw) { return (halves(extent(tw, tap_w, dst_w), src_w) * (planar ? 1 : 2) + 30) / 16 * 16; };
    auto stage_of = [&](int tw, int th) {
        const size_t e = extent(th, tap_h, dst_h);
        return e * yslot_of(tw) + halves(e, src_h) * (planar ? 2 : 1) * cslot_of(tw);
    };
    auto lds_of = [&](int tw, int th) { return stage_of(tw, th) + 12 * ((size_t)tw + (size_t)th); };
    int tw = dst_w;                        // whole rows, unless one row's sources do not fit
    while (tw > 1 && lds_of(tw, 1) > kStageBudget) tw = tw > 4 ? (((tw + 1) / 2 + 3) & ~3) : tw - 1;
    int th = 2 * kBlock / ((tw + 3) / 4);  // about two quads per lane
    th = th < 1 ? 1 : (th > dst_h ? dst_h : th);
    while (th > 1 && lds_of(tw, th) > kStageBudget) th = (th + 1) / 2;
    PVHIP_CHECK_ARG(lds_of(tw, th) <= kStageBudget);
    const dim3 grid((unsigned)((dst_w + tw - 1) / tw), (unsigned)((dst_h + th - 1) / th), (unsigned)n);
    PVHIP_CHECK_ARG(grid.y <= 65535);
    YuvArgs a;
    a.src = (const unsigned char*)src; a.dst = dst; a.mean = mean; a.std_scale = std_scale;
    a.hs = src_h; a.ws = src_w; a.hd = dst_h; a.wd = dst_w; a.tw = tw; a.th = th;
    a.planar = planar; a.reverse = reverse_channels ? 1 : 0;
    a.yslot = (unsigned)yslot_of(tw); a.cslot = (unsigned)cslot_of(tw); a.stage_bytes = (unsigned)stage_of(tw, th);
    a.rois = rois; a.m = m; a.mh = roi_h; a.mw = roi_w;
    const bool vs = (uintptr_t)dst % 16 == 0 && dst_w % 4 == 0 && tw % 4 == 0;
    const size_t lds = lds_of(tw, th);
    hipStream_t st = state().stream;
    if (roi) launch_yuv<true, true>(a, grid, lds, vs, st);
    else     resize ? launch_yuv<true, false>(a, grid, lds, vs, st) : launch_yuv<false, false>(a, grid, lds, vs, st);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // namespace

extern "C" {

int pvhip_input_preprocess_f32(const void* src, float* dst, int n, int c, int src_h, int src_w, int dst_h, int dst_w,
                               int src_u8, int src_nhwc, int reverse_channels, const float* mean, const float* std_scale) {
    return preprocess_launch(src, dst, nullptr, n, n, c, src_h, src_w, dst_h, dst_w, src_h, src_w, src_u8, src_nhwc, reverse_channels,
                             mean, std_scale);
}

int pvhip_input_preprocess_yuv_f32(const void* src, float* dst, int n, int src_h, int src_w, int dst_h, int dst_w, int planar,
                                   int reverse_channels, const float* mean, const float* std_scale) {
    return preprocess_yuv_launch(src, dst, nullptr, n, n, src_h, src_w, dst_h, dst_w, src_h, src_w, planar, reverse_channels, mean, std_scale);
}

int pvhip_input_preprocess_roi_f32(const void* src, float* dst, const int* rois, int n, int m, int c, int src_h, int src_w, int dst_h,
                                   int dst_w, int max_roi_h, int max_roi_w, int src_u8, int src_nhwc, int reverse_channels,
                                   const float* mean, const float* std_scale) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(rois != nullptr);
    return preprocess_launch(src, dst, rois, n, m, c, src_h, src_w, dst_h, dst_w, max_roi_h, max_roi_w, src_u8, src_nhwc, reverse_channels,
                             mean, std_scale);
}

int pvhip_input_preprocess_yuv_roi_f32(const void* src, float* dst, const int* rois, int n, int m, int src_h, int src_w, int dst_h,
                                       int dst_w, int max_roi_h, int max_roi_w, int planar, int reverse_channels, const float* mean,
                                       const float* std_scale) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(rois != nullptr);
    return preprocess_yuv_launch(src, dst, rois, n, m, src_h, src_w, dst_h, dst_w, max_roi_h, max_roi_w, planar, reverse_channels, mean,
                                 std_scale);
}

}  // extern "C"
