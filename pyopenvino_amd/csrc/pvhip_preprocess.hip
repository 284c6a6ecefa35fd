// Input preprocessing (HBM-bound): the staged host input of a request -- a U8 or FP32 image of any extent, NHWC or NCHW -- becomes the
// fp32 NCHW tensor the network's Parameter expects, in ONE launch: bilinear resize, channel reversal, per-channel mean / scale and the
// layout change (IENetwork.input_info[name].preprocess_info).
//
// Resize: half-pixel centres clamped at the border, no antialiasing (cv2 INTER_LINEAR, torch interpolate bilinear with
// align_corners=False).  The source coordinate of destination index d is num / (2D) with num = max((2d+1)S - D, 0), computed exactly in
// 64-bit integers; i0 = min(num / 2D, S-1), i1 = min(i0+1, S-1), f = (num - 2D i0) / 2D as ONE correctly rounded fp32 division (0 at
// the last source index).  v = (1-fy)((1-fx)p00 + fx p01) + fy((1-fx)p10 + fx p11) in fp32, in that order, never contracted to fma.
// Then y = (v - mean[c]) / std_scale[c], output channel c reading source channel C-1-c under reversal.  tests/preprocess_ref.py is the
// same rule in numpy; the kernels match it bit for bit.
//
// ONE tile body (staged_tile) over three sources.  A source is the one place that knows a format -- what a tile stages of it, where a
// tapped row lies in LDS and how a tapped pixel is decoded, and on the host the checks and the LDS sizes that go with them --:
// RawSource for U8 / FP32 images, Yuv420Source for YUV 4:2:0 frames (NV12, I420), which converts every tapped pixel to B, G, R in front of
// the interpolation, and PackedSource for frames of 4-byte units (packed YUV 4:2:2: YUY2, UYVY; four-byte pixels: BGRX, RGBX), which
// decodes every tapped pixel.  The three kernels -- preprocess_kernel, preprocess_yuv_kernel, preprocess_packed_kernel -- are the body
// over one source each; one launcher (launch_staged) plans and launches all of them, the form of a launch -- resize, table, fit, store
// form, literal colour rule -- becoming template arguments in one place (with_form).
// A workgroup owns a tile of `th` output rows x `tw` output columns of one image (normally whole rows; plan_tiles).  It
//   1. finds its tile and the source extent its taps see (tile_of);
//   2. tabulates the tile's column and row coordinates (x0, x1, fx), (y0, y1, fy) in LDS (fill_tables);
//   3. stages the source it reads -- for every row y0(first)..y1(last) the contiguous span of columns x0(first)..x1(last): per channel
//      plane (NCHW), for all channels at once (NHWC), or of the Y plane and of the chroma under it (YUV) -- into LDS with 16-byte loads
//      (stage_block); every span keeps its address modulo 16 in LDS (span_base), so any source alignment takes the wide loads, with
//      byte-wise head and tail;
//   4. has every lane produce 4 consecutive output pixels of one row, for every channel, stored as float4 nontemporal stores into each
//      channel plane, scalar stores when the destination rows are not 16-byte aligned (finish_quad).
//
// Regions of interest (the ROI entries): image b of the output is the rectangle rois[b] = (id, x, y, w, h) of frame id of m frames, cropped
// and then resized -- the taps clamp at the rectangle's edge, not the frame's.  Every kernel takes it as a template parameter: a workgroup
// reads its image's five ints, takes S = (h, w) for its taps and adds (id, y, x) to the addresses it stages from; a rectangle of exactly
// the destination's extent is copied (fp32 sources: no 0 * inf; bytes give the same bits either way).  The table is device data, so an image whose rectangle does not lie inside a frame, or
// exceeds the maxima the launch was sized for, is written as quiet NaN and nothing is read for it.  tests/roi_ref.py is the rule in numpy.
//
// An aspect-preserving fit (the _fit_ entries; preprocess_info.resize_fit 'LETTERBOX' / 'TOP_LEFT'): the source -- a whole image, or the
// rectangle of a table -- is scaled by ONE factor into the rectangle [dy, dy + ih) x [dx, dx + iw) of the destination (fit_rect: integers
// only, the short side rounded half up) by the rule above onto (ih, iw), and the rest of the destination is the pad value, which goes through
// the same mean / scale.  No new interpolation: every kernel takes it as one more template parameter beside ROI.  tile_of computes the
// rectangle per workgroup (a table is device data) and fills a tile that lies wholly in the padding without touching `src`; fill_tables
// runs the taps over (ih, iw) at d - dx, d - dy, clamped into the rectangle, so a tile stages what its intersection with the rectangle
// reads; the quad loop replaces the value of a pixel outside it by the pad (quads may straddle the edge: dx is any integer; the stores do
// not change).  The tiles are sized by a bound on the taps' step over every rectangle the launch may meet (Reach), and a workgroup whose
// tile would still not fit its slots writes NaN instead of staging.  tests/letterbox_ref.py is the rule in numpy.
//
// Affine warps (the warp entry; preprocess_warp_kernel): image b is frame id of m frames sampled through a 2 x 3 matrix in Q16,
// table[b] = (id, A00, A01, C0, A10, A11, C1) as int64.  For output pixel (y, x): SX = A00 x + A01 y + C0, SY = A10 x + A11 y + C1 in
// int64; ix = SX >> 16, fx = float(SX & 0xFFFF) 2^-16 (exact), iy and fy likewise; P(r, c) is the frame's pixel when 0 <= r < H and
// 0 <= c < W (64-bit compares), else the pad in every channel -- for the colour formats the B, G, R that yuv_to_bgr / packed_to_bgr
// give, with the chroma of the pixel's block of the FRAME --; top = fx == 0 ? P(iy, ix) : (1-fx) P(iy, ix) + fx P(iy, ix+1), bot the
// same on row iy + 1, v = fy == 0 ? top : (1-fy) top + fy bot, then the epilogue of the other kernels.  A zero fraction takes the one
// tap as it is, so an integer translation is a copy bit for bit.  tests/warp_ref.py is the rule in numpy.
// This kernel stages nothing: the source footprint of an output tile is a parallelogram, and at the rotations and downscales a warp is
// for, its bounding box is mostly pixels nobody reads (a 16 x 16 tile at scale 8 and 45 degrees spans about 180^2 source pixels, over
// kStageBudget).  It gathers its taps from global memory through the caches: a lane produces a quad of one row for every channel
// (finish_quad, as above), SX and SY advancing by A00 and A10 per pixel, and the format is a fetch functor (RawFetch, Yuv420Fetch,
// PackedFetch) over pixel<U8>, yuv_to_bgr and packed_to_bgr; the channels of a uint8 NHWC tap, a 4-byte unit and NV12's (U, V) pair
// are one load each.  Tile: 32 x 32 output pixels per workgroup, 8 quads x 32 rows, so a wave owns 32 x 8 pixels: the most compact
// footprint whose rows are still whole 128-byte lines of float4 stores per plane -- under a rotation a wave's taps then fall into
// about as few source lines as its pixel count allows, where the 64 x 16 alternative (a wave: 64 x 4) stretches them along one axis
// -- and 32 divides the 224 of the classifiers here, which 64 does not.  Measured (profiles/warp_input.md; 256 rows of 1080p frames
// -> 224 x 224, uint8 NHWC / NV12): 30 degrees at scale 3 313 / 156 us against 326 / 198 us for 64 x 16, upright at scale 3 48.6 /
// 55.5 us against 47.2 / 53.9 us -- and 174 / 141 us for the ROI launch on the same rectangles.
//
// Projective warps (the perspective entry; preprocess_perspective_kernel): image b is frame id sampled through a 3 x 3 homography,
// table[b] = (id, Q00 .. Q22) as int64, the matrix scaled on the host by a power of two of its own so that every linear form stays
// below 2^52 over the extent (the ratio does not see the scale).  For output pixel (y, x): NX = Q00 x + Q01 y + Q02, NY = Q10 x +
// Q11 y + Q12, D = Q20 x + Q21 y + Q22 in int64; TX = floor(double(NX) / double(D) * 65536), TY likewise -- binary64, one IEEE division
// each (the compiler's v_div_scale / v_rcp / v_div_fmas / v_div_fixup sequence: no reciprocal shared, nothing contracted), exact
// operands, so numpy's float64 gives the same bits --; the pixel is the pad unless D != 0 and |TX|, |TY| < 2^47; else SX = TX, SY = TY
// and the rule above from there on.  Only where the sample position comes from is new: the kernel has the tile, the fetch functors and
// the quad body (sample_quad) of the affine kernel, two divisions per pixel in place of two additions, and no whole-number form.
// tests/perspective_ref.py is the rule in numpy; include/pvhip.h states it in full.
#include "pvhip_common.h"
#include "pvhip_fit_rect.h"

#include <type_traits>

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

// What the _fit_ entries add to a launch; fit 0: none.  false: not a fit, or no finite pad.
struct Fit {
    int fit;
    float pad;
    bool ok() const { return (fit == 1 || fit == 2) && pad - pad == 0.0f; }
};

struct YuvRule;

// What an entry asks of its launcher (launch_staged, preprocess_warp_launch), as the caller gave it.  rois == NULL: image b is the whole
// of source image b, with m = n and (roi_h, roi_w) = (src_h, src_w); else image b is a rectangle of one of m frames, and the tiles and
// LDS slots are sized for the largest rectangle (roi_h, roi_w): extent() is monotone in S, so the budget holds for every image.
struct Job {
    const void* src;
    float* dst;
    const int* rois;
    int n, m, c;
    int src_h, src_w, dst_h, dst_w, roi_h, roi_w;
    int how;                  // raw: src_u8 | src_nhwc << 1; YUV 4:2:0: planar; 4-byte units: kind
    int reverse;
    const float *mean, *std_scale;
    Fit fit;                  // (the warp entries: fit 0 and their pad)
    const YuvRule* rule;      // NULL: BT.601 limited range, the LIT kernels
    const long long* table;   // the warp entries
};

// What a launch of any kernel is given; each kernel's own members follow it (PrepArgs, YuvArgs, PackedArgs, WarpArgs).
struct TileArgs {
    const unsigned char* src;
    float* dst;
    const float* mean;        // NULL: no mean
    const float* std_scale;   // NULL: no scale
    int hs, ws, hd, wd, tw, th;
    int reverse;
    unsigned stage_bytes;     // LDS bytes of the staging area (the coordinate tables follow it)
    const int* rois;          // ROI kernels: n x (id, x, y, w, h); hs, ws are then the extent of each of the m frames
    int m, mh, mw;            // ... the frame count and the largest h and w the launch was sized for
    int fit;                  // FIT kernels: 1 LETTERBOX (the fitted rectangle is centred), 2 TOP_LEFT
    float pad;                // ... the value outside the fitted rectangle, in source units (it goes through mean / scale)
};

// The tile of one workgroup: columns tx0.. (twv of them) of rows ty0.. (thv of them) of image n, whose taps see a source of hs x ws
// pixels: the whole of source image img = n, or (ROI kernels) the rectangle at column ox, row oy of frame img.
// FIT kernels: the taps run over the fitted rectangle [dy, dy + ih) x [dx, dx + iw) of the destination, everything outside it is `pad`;
// else that rectangle is the destination.
struct Tile {
    int n, tx0, ty0, twv, thv;
    int hs, ws, img, ox, oy;
    int dx, dy, iw, ih;
};

// Every pixel of the tile, in all c planes, becomes v (FIT: (v - mean) / std_scale, as finish_quad computes it).
template <bool EPILOGUE>
__device__ __forceinline__ void fill_tile(const TileArgs& a, int c, const Tile& t, float v) {
    const size_t plane_out = (size_t)a.hd * a.wd;
    float* out_n = a.dst + (size_t)t.n * c * plane_out;
    for (int oc = 0; oc < c; ++oc) {
        float w = v;
        if (EPILOGUE && a.mean != nullptr) w = w - a.mean[oc];
        if (EPILOGUE && a.std_scale != nullptr) w = w / a.std_scale[oc];
        for (int i = threadIdx.x; i < t.thv * t.twv; i += kBlock) {
            const int r = i / t.twv;
            out_n[oc * plane_out + (size_t)(t.ty0 + r) * a.wd + t.tx0 + (i - r * t.twv)] = w;
        }
    }
}

// grid (ceil(wd / tw), ceil(hd / th), n).  ROI: the image's rectangle (id, x, y, w, h) is read once per workgroup; false: it does not lie
// inside frame id or exceeds the launch's maxima, the tile is filled with quiet NaN in all c planes -- padding included -- and the
// workgroup is done.  FIT: the fitted rectangle follows from the extent the taps see (per workgroup: a table is device data); false too
// when the tile lies wholly in the padding: it is filled with the pad value and nothing of `src` is touched.
template <bool ROI, bool FIT>
__device__ __forceinline__ bool tile_of(const TileArgs& a, int c, Tile& t) {
    t.n = blockIdx.z; t.tx0 = blockIdx.x * a.tw; t.ty0 = blockIdx.y * a.th;
    t.twv = min(a.tw, a.wd - t.tx0); t.thv = min(a.th, a.hd - t.ty0);
    t.hs = a.hs; t.ws = a.ws; t.img = t.n; t.ox = 0; t.oy = 0;
    t.dx = 0; t.dy = 0; t.iw = a.wd; t.ih = a.hd;
    if (ROI) {
        const int* q = a.rois + 5 * (size_t)t.n;
        t.img = q[0]; t.ox = q[1]; t.oy = q[2]; t.ws = q[3]; t.hs = q[4];
        if (!(t.img >= 0 && t.img < a.m && t.ox >= 0 && t.oy >= 0 && t.ws >= 1 && t.hs >= 1 && t.ws <= a.mw && t.hs <= a.mh
              && (long long)t.ox + t.ws <= a.ws && (long long)t.oy + t.hs <= a.hs)) {
            fill_tile<false>(a, c, t, __builtin_nanf(""));
            return false;
        }
    }
    if (FIT) {
        const FitRect f = fit_rect(t.hs, t.ws, a.hd, a.wd, a.fit);
        t.dx = f.dx; t.dy = f.dy; t.iw = f.iw; t.ih = f.ih;
        if (t.tx0 >= t.dx + t.iw || t.tx0 + t.twv <= t.dx || t.ty0 >= t.dy + t.ih || t.ty0 + t.thv <= t.dy) {
            fill_tile<true>(a, c, t, a.pad);
            return false;
        }
    }
    return true;
}

// The coordinate tables of a tile, in dynamic LDS behind the staging area: (x0, x1, fx) of each of its tw columns, then (y0, y1, fy) of
// each of its th rows -- bytes(tw, th) in all --, and the source the tile reads (the taps are monotone in d): columns xs0..xs1 of rows
// ys0..ys1.
struct Tables {
    int *cx0, *cx1;
    float* cfx;
    int *ry0, *ry1;
    float* rfy;
    int xs0, xs1, ys0, ys1;
    static constexpr size_t bytes(int tw, int th) { return 3 * sizeof(int) * ((size_t)tw + (size_t)th); }
};

// taps(d, S, D): the Tap of destination index d.  Read the tables after a __syncthreads().  FIT: index d of the destination is index
// d - dx (d - dy) of the fitted rectangle, clamped into it -- a pixel of the padding gets the taps of the nearest inner column (row), which
// the tile stages anyway, and its value is replaced by the pad --, so the source the tile reads is that of its intersection with the
// fitted rectangle (not empty: tile_of).
template <bool FIT, class Taps>
__device__ __forceinline__ Tables fill_tables(unsigned char* lds, const TileArgs& a, const Tile& t, Taps taps) {
    auto col = [&](int d) { return FIT ? taps(min(max(d - t.dx, 0), t.iw - 1), t.ws, t.iw) : taps(d, t.ws, a.wd); };
    auto row = [&](int d) { return FIT ? taps(min(max(d - t.dy, 0), t.ih - 1), t.hs, t.ih) : taps(d, t.hs, a.hd); };
    Tables b;
    b.cx0 = reinterpret_cast<int*>(lds + a.stage_bytes);
    b.cx1 = b.cx0 + a.tw;
    b.cfx = reinterpret_cast<float*>(b.cx1 + a.tw);
    b.ry0 = reinterpret_cast<int*>(b.cfx + a.tw);
    b.ry1 = b.ry0 + a.th;
    b.rfy = reinterpret_cast<float*>(b.ry1 + a.th);
    for (int j = threadIdx.x; j < t.twv; j += kBlock) {
        const Tap p = col(t.tx0 + j);
        b.cx0[j] = p.i0; b.cx1[j] = p.i1; b.cfx[j] = p.f;
    }
    for (int j = threadIdx.x; j < t.thv; j += kBlock) {
        const Tap p = row(t.ty0 + j);
        b.ry0[j] = p.i0; b.ry1[j] = p.i1; b.rfy[j] = p.f;
    }
    b.xs0 = col(t.tx0).i0; b.xs1 = col(t.tx0 + t.twv - 1).i1;
    b.ys0 = row(t.ty0).i0; b.ys1 = row(t.ty0 + t.thv - 1).i1;
    return b;
}

// A span -- contiguous source bytes starting at g -- is staged into an LDS slot (16-byte aligned, at least span + 30 bytes rounded down
// to 16) at the source's address modulo 16: its byte j lies at span_base(slot, g) + j.
__device__ __forceinline__ int misalign(const unsigned char* g) { return (int)((uintptr_t)g & 15); }

__device__ __forceinline__ const unsigned char* span_base(const unsigned char* slot, const unsigned char* g) { return slot + misalign(g); }

// Block k of the slot: 16 aligned source bytes in one load, or those of them that belong to the span (its head and tail) byte by byte.
__device__ __forceinline__ void stage_block(const unsigned char* g, int span, unsigned char* slot, unsigned k) {
    const int lo = 16 * (int)k - misalign(g);                 // the block's first byte, relative to the span's
    const unsigned char* b = g + lo;
    unsigned char* l = slot + 16 * k;
    if (lo >= 0 && lo + 16 <= span) {
        *reinterpret_cast<u4v*>(l) = *reinterpret_cast<const u4v*>(b);
    } else {
        for (int t = lo < 0 ? -lo : 0; t < 16 && lo + t < span; ++t) l[t] = b[t];
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

// The quad v of output channel oc, destined for o[0..3] (columns j0.. of a tile of twv): mean, scale, store.
// VS: every tile's quads start 16-byte aligned in every output plane (dst aligned, wd and tw multiples of 4).
template <bool VS>
__device__ __forceinline__ void finish_quad(const TileArgs& a, int oc, float (&v)[4], float* o, int j0, int twv) {
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

// FIT: row r / column j of the tile lies in the fitted rectangle.
__device__ __forceinline__ bool row_inside(const Tile& t, int r) { return (unsigned)(t.ty0 + r - t.dy) < (unsigned)t.ih; }
__device__ __forceinline__ bool col_inside(const Tile& t, int j) { return (unsigned)(t.tx0 + j - t.dx) < (unsigned)t.iw; }

// A span of `span` bytes fits a slot of `slot` bytes as the launchers size them.
__device__ __forceinline__ bool span_fits(int span, unsigned slot) { return ((unsigned)span + 30) / 16 * 16 <= slot; }
// ... and the slot they give a span of at most `span` bytes.
size_t slot_for(size_t span) { return (span + 30) / 16 * 16; }

// ------------------------------------------------------------------------------------------------------------------- the sources
// A source is the one place that knows a format: RawSource<U8>, Yuv420Source<LIT>, PackedSource<KIND, LIT>.  staged_tile and
// launch_staged are written over what each of them declares:
//   Args                          the kernel's argument struct, TileArgs and the format's own members;
//   K                             the channels one decode yields; the c channels of the destination are c / K groups of K;
//   Lit<L>                        the source with the YuvRule as literals (L) or from the arguments; itself where it has no rule;
// on the host, beside the device code they bound (cols, rows: the source columns and rows a tile reads at most, Reach):
//   check(job, a)                 the format's argument checks; sets the format's members of a (a holds common_args' already);
//   stage_bytes(a, rows, cols)    the LDS bytes a tile stages;     set_slots(a, cols): the slot members of a;
// on the device, constructed for one tile from (a, t, tb, lds) once the coordinate tables are filled -- a source COPIES what it needs of
// the tile and the tables into members of its own (ox, ys0, ...) and keeps no reference to either: with references in the struct the
// 4:2:2 kernels came out a register and 0.3 - 1.0 us a launch worse (profiles/preprocess_source_refactor.md) --:
//   channels(a)                   the destination's channels;
//   kCopies, copies<CROP>(t)      where kCopies: (workgroup-uniform) the tile takes every pixel's one tap as it is.  A source that
//                                 never copies declares kCopies false and no copies(): its kernels then carry no trace of the rule;
//   groups(), kGroups, fits()     c / K (kGroups: 1 where that is known here, else 0); every span fits its slot and the slots fit
//                                 stage_bytes (FIT kernels check it);
//   blocks(), stage(i)            the 16-byte blocks the tile stages, and block i of them;
//   row(r, g)                     the handle (Row) of the r-th staged source row (tap row - ys0) for channel group g;
//   decode(row, x, o)             o[0..K) = the channels of group g of the pixel at column x of that row.
// x is a tap coordinate: relative to the image's rectangle, as the tables hold it.

// ------------------------------------------------------------------------------------------------------------ U8 / FP32 images
struct PrepArgs : TileArgs {
    int c, nhwc;
    unsigned slot;            // LDS bytes per staged span (a multiple of 16)
};

// One span per source row: of each channel plane (NCHW), or of all channels side by side (NHWC).  A group is one channel, whatever c.
template <bool U8>
struct RawSource {
    using Args = PrepArgs;
    template <bool>
    using Lit = RawSource;
    static constexpr int K = 1, ES = U8 ? 1 : 4;

    static int check(const Job& j, Args& a) {
        PVHIP_CHECK_ARG(j.c <= kMaxChannels);
        PVHIP_CHECK_ARG(U8 || (uintptr_t)j.src % 4 == 0);                            // fp32 sources are element-aligned
        a.c = j.c; a.nhwc = j.how >> 1;
        return PVHIP_OK;
    }
    static size_t slot_bytes(const Args& a, size_t cols) { return slot_for(cols * (a.nhwc ? (size_t)a.c : 1) * ES); }
    static size_t stage_bytes(const Args& a, size_t rows, size_t cols) { return (a.nhwc ? 1 : (size_t)a.c) * rows * slot_bytes(a, cols); }
    static void set_slots(Args& a, size_t cols) { a.slot = (unsigned)slot_bytes(a, cols); }

    const Args& a;
    int img, ox, oy, xs0, ys0;    // the frame and the rectangle's corner in it; the first staged column and row
    unsigned char* lds;
    int rows, cs, planes, span;   // staged rows; elements per pixel of a span, spans per row; bytes of one staged span
    unsigned bps;                 // 16-byte blocks a span touches at most

    __device__ __forceinline__ static int channels(const Args& a) { return a.c; }
    // the rectangle has the destination's extent (FIT: the source has the fitted rectangle's): fp32 sources are copied, identity weights
    // would turn an inf neighbour into NaN (bytes interpolate to the same bits: weight 0 on a finite value)
    static constexpr bool kCopies = true;
    template <bool CROP>
    __device__ __forceinline__ static bool copies(const Tile& t) { return CROP && !U8 && t.hs == t.ih && t.ws == t.iw; }

    __device__ __forceinline__ RawSource(const Args& a, const Tile& t, const Tables& tb, unsigned char* lds)
        : a(a), img(t.img), ox(t.ox), oy(t.oy), xs0(tb.xs0), ys0(tb.ys0), lds(lds), rows(tb.ys1 - tb.ys0 + 1), cs(a.nhwc ? a.c : 1), planes(a.nhwc ? 1 : a.c),
          span((tb.xs1 - tb.xs0 + 1) * cs * ES), bps((unsigned)span / 16 + 2) {}
    static constexpr int kGroups = 0;         // c of them
    __device__ __forceinline__ int groups() const { return a.c; }
    __device__ __forceinline__ bool fits() const { return span_fits(span, a.slot) && (size_t)planes * rows * a.slot <= a.stage_bytes; }
    // span s = plane * rows + row: its first byte in the source
    __device__ __forceinline__ const unsigned char* span_src(int s) const {
        const int p = s / rows, r = s - p * rows;
        const size_t e = a.nhwc ? ((size_t)img * a.hs + oy + ys0 + r) * a.ws * (size_t)a.c + (size_t)(ox + xs0) * a.c
                                : (((size_t)img * a.c + p) * a.hs + oy + ys0 + r) * a.ws + ox + xs0;
        return a.src + e * ES;
    }
    __device__ __forceinline__ unsigned blocks() const { return (unsigned)(planes * rows) * bps; }
    __device__ __forceinline__ void stage(unsigned i) const {
        const unsigned s = i / bps;
        stage_block(span_src((int)s), span, lds + s * a.slot, i - s * bps);
    }
    struct Row {
        const unsigned char* l;
        int ch;                   // the channel's element inside a pixel of the span
    };
    __device__ __forceinline__ Row row(int r, int g) const {
        const int s = (a.nhwc ? 0 : g) * rows + r;
        return Row{span_base(lds + (unsigned)s * a.slot, span_src(s)), a.nhwc ? g : 0};
    }
    __device__ __forceinline__ void decode(const Row& w, int x, float (&o)[K]) const { o[0] = pixel<U8>(w.l, (x - xs0) * cs + w.ch); }
};

// ---------------------------------------------------------------------------------------------------------------- YUV 4:2:0 sources
// A decoder's frame -- uint8, 3 h / 2 rows of w bytes per image: the Y plane, then NV12's h/2 rows of w/2 (U, V) pairs or I420's U plane
// and V plane of h/2 x w/2 bytes each -- converted to B, G, R by ONE rule in 20-bit fixed point, whose six ints (YuvRule) say which
// matrix and range the frames were encoded with (preprocess_info.color_standard / color_range; kYuvRules):
//   t = max(Y - yoff, 0) * CY + 2^19,  R = (t + CRV (V - 128)) >> 20,  G = (t - CGV (V - 128) - CGU (U - 128)) >> 20,
//   B = (t + CBU (U - 128)) >> 20  (arithmetic shifts), each clamped to [0, 255],
// BT.601 limited range -- yoff 16 and 1220542, 1673527, 852492, 409993, 2116026 -- where nothing is declared, with the (U, V) of the
// pixel's 2 x 2 block (no chroma interpolation); the uint8 image that gives is then resized, reversed and scaled exactly as a U8 NHWC
// source is above.  tests/yuv_ref.py is the BT.601 conversion in numpy and tests/colorimetry_ref.py all six; every intermediate stays
// within +-5.8e8.
//
// A tile stages the Y spans it reads and, behind them, the chroma spans under them: rows ys0/2..ys1/2, of each the pairs xs0/2..xs1/2 of
// the ABSOLUTE columns (a tile may start on an odd column) -- one span per row for NV12, one in each plane for I420.  A pixel is converted
// where it is tapped, so a downscale converts four pixels per output pixel however many it staged, and the three channels of a quad come
// from one pass over its taps.
//
// The rule of a launch.  It travels in the launch arguments, so the kernels read it from scalar registers: one yuv_to_bgr, and no
// kernel instantiation per rule -- but one more of each staged kernel, LIT, in which the rule is row [0][0] as literals: what every
// launch without a declared standard or range takes, instruction for instruction the code it was before rules were arguments.  From
// scalar registers the same conversion schedules 1.4 to 4 % slower (profiles/colorimetry.md), which a declared rule pays and the
// default does not.  The warp kernel gathers from global memory and showed no difference: it has the one form.
struct YuvRule {
    int yoff, cy, crv, cgv, cgu, cbu;
};

// kYuvRules[matrix][full_range]: matrix 0 BT.601, 1 BT.709, 2 BT.2020.  Row [0][0] is the three-decimal constants of cv2 (1.164, 1.596,
// 0.813, 0.391, 2.018); every other row is rint(x 2^20) of 2 (1 - Kr), 2 Kr (1 - Kr) / Kg, 2 Kb (1 - Kb) / Kg, 2 (1 - Kb) with
// (Kr, Kb) = (0.299, 0.114), (0.2126, 0.0722), (0.2627, 0.0593) and Kg = 1 - Kr - Kb, times 255/224 (and the luma gain 255/219) for
// limited range.  yoff = 0 makes the luma clamp the identity: full range is no second code path.
constexpr YuvRule kYuvRules[3][2] = {
    {{16, 1220542, 1673527, 852492, 409993, 2116026}, {0, 1048576, 1470104, 748826, 360853, 1858077}},
    {{16, 1220945, 1879825, 558796, 223607, 2215014}, {0, 1048576, 1651297, 490864, 196424, 1945738}},
    {{16, 1220945, 1760217, 682019, 196426, 2245811}, {0, 1048576, 1546230, 599107, 172546, 1972791}},
};

// What yuv_to_bgr's masks assume of every row: a byte for yoff, constants below 2^23.
constexpr bool yuv_rules_fit() {
    for (const auto& matrix : kYuvRules)
        for (const YuvRule& r : matrix)
            for (int c : {r.cy, r.crv, r.cgv, r.cgu, r.cbu})
                if (r.yoff < 0 || r.yoff > 255 || c < 0 || c >= (1 << 23)) return false;
    return true;
}
static_assert(yuv_rules_fit(), "a rule's constants are 23-bit: the products of yuv_to_bgr are 24-bit multiplies");

struct YuvArgs : TileArgs {
    int planar;
    unsigned yslot, cslot;    // LDS bytes per staged Y span and per staged chroma span (multiples of 16)
    YuvRule rule;
};

// B, G, R (in that order) of one pixel, as the floats of the converted bytes.  LIT: the rule is kYuvRules[0][0], whatever `k` holds.
// Else the constants come from scalar registers, where the compiler knows nothing of their range: the masks (scalar instructions,
// once per wave, and the identity on every row of the table) tell it they are 23-bit, so each product stays a full-rate 24-bit
// multiply.
template <bool LIT = false>
__device__ __forceinline__ void yuv_to_bgr(const YuvRule& k, int y, int u, int v, float (&o)[3]) {
    constexpr int kBits = (1 << 23) - 1;
    constexpr YuvRule d = kYuvRules[0][0];
    const int yoff = LIT ? d.yoff : k.yoff & 255, cy = LIT ? d.cy : k.cy & kBits, crv = LIT ? d.crv : k.crv & kBits;
    const int cgv = LIT ? d.cgv : k.cgv & kBits, cgu = LIT ? d.cgu : k.cgu & kBits, cbu = LIT ? d.cbu : k.cbu & kBits;
    y = max(y, yoff) - yoff;
    u -= 128; v -= 128;
    const int t = y * cy + (1 << 19);
    const int b = (t + cbu * u) >> 20;
    const int g = (t - cgv * v - cgu * u) >> 20;
    const int r = (t + crv * v) >> 20;
    o[0] = (float)min(max(b, 0), 255);
    o[1] = (float)min(max(g, 0), 255);
    o[2] = (float)min(max(r, 0), 255);
}

// ROI: the chroma of a pixel is that of its ABSOLUTE 2 x 2 block of the frame, so a rectangle may start on odd coordinates and have odd
// sizes.  (A rectangle of the destination's extent needs no copy path here: the converted pixels are bytes, and weight 0 on a finite
// value interpolates to the same bits.)
template <bool LIT = true>
struct Yuv420Source {
    using Args = YuvArgs;
    template <bool L>
    using Lit = Yuv420Source<L>;
    static constexpr int K = 3;

    static int check(const Job& j, Args& a) {
        PVHIP_CHECK_ARG(j.src_h % 2 == 0 && j.src_w % 2 == 0);                       // 4:2:0: one (U, V) per 2 x 2 block
        PVHIP_CHECK_ARG(j.how == 0 || j.how == 1);
        a.planar = j.how; a.rule = j.rule ? *j.rule : kYuvRules[0][0];
        return PVHIP_OK;
    }
    // e consecutive rows (columns) lie over at most e / 2 + 1 chroma rows (pairs): the first may be an odd one
    static size_t halves(size_t e, int S) { return e / 2 + 1 < (size_t)S / 2 ? e / 2 + 1 : (size_t)S / 2; }
    static size_t yslot_bytes(const Args&, size_t cols) { return slot_for(cols); }
    static size_t cslot_bytes(const Args& a, size_t cols) { return slot_for(halves(cols, a.ws) * (a.planar ? 1 : 2)); }
    static size_t stage_bytes(const Args& a, size_t rows, size_t cols) {
        return rows * yslot_bytes(a, cols) + halves(rows, a.hs) * (a.planar ? 2 : 1) * cslot_bytes(a, cols);
    }
    static void set_slots(Args& a, size_t cols) { a.yslot = (unsigned)yslot_bytes(a, cols); a.cslot = (unsigned)cslot_bytes(a, cols); }

    const Args& a;
    int ox, oy, xs0, ys0;         // the rectangle's corner in the frame; the first staged column and row
    unsigned char* lds;
    int rows, yspan;              // staged Y rows, bytes of one of them
    int ps0, cr0, crows;          // first chroma pair and row, chroma rows
    int cstep, cspan, hw;         // bytes from one U (V) to the next; bytes of one chroma span; a chroma plane's row
    const unsigned char *frame, *chroma;
    unsigned char* lds_c;         // the chroma slots, behind the Y slots
    unsigned ybps, cbps, yblk, cblk;

    __device__ __forceinline__ static int channels(const Args&) { return K; }
    static constexpr bool kCopies = false;

    __device__ __forceinline__ Yuv420Source(const Args& a, const Tile& t, const Tables& tb, unsigned char* lds)
        : a(a), ox(t.ox), oy(t.oy), xs0(tb.xs0), ys0(tb.ys0), lds(lds), rows(tb.ys1 - tb.ys0 + 1), yspan(tb.xs1 - tb.xs0 + 1), ps0((t.ox + tb.xs0) >> 1),
          cr0((t.oy + tb.ys0) >> 1), crows(((t.oy + tb.ys1) >> 1) - cr0 + 1), cstep(a.planar ? 1 : 2),
          cspan((((t.ox + tb.xs1) >> 1) - ps0 + 1) * cstep), hw(a.ws >> 1), frame(a.src + (size_t)t.img * ((size_t)a.hs * a.ws / 2 * 3)),
          chroma(frame + (size_t)a.hs * a.ws), lds_c(lds + (unsigned)rows * a.yslot), ybps((unsigned)yspan / 16 + 2),
          cbps((unsigned)cspan / 16 + 2), yblk((unsigned)rows * ybps), cblk((unsigned)(crows * (a.planar ? 2 : 1)) * cbps) {}
    static constexpr int kGroups = 1;
    __device__ __forceinline__ int groups() const { return 1; }
    __device__ __forceinline__ bool fits() const {
        return span_fits(yspan, a.yslot) && span_fits(cspan, a.cslot) &&
               (size_t)rows * a.yslot + (size_t)crows * (a.planar ? 2 : 1) * a.cslot <= a.stage_bytes;
    }
    __device__ __forceinline__ const unsigned char* y_src(int r) const { return frame + (size_t)(oy + ys0 + r) * a.ws + ox + xs0; }
    // chroma span s: NV12 row s of the pairs; I420 row s of U for s < crows, row s - crows of V after them
    __device__ __forceinline__ const unsigned char* c_src(int s) const {
        if (!a.planar) return chroma + (size_t)(cr0 + s) * a.ws + 2 * ps0;
        const int p = s >= crows ? 1 : 0;
        return chroma + ((size_t)p * (a.hs >> 1) + cr0 + s - p * crows) * hw + ps0;
    }
    __device__ __forceinline__ unsigned blocks() const { return yblk + cblk; }
    __device__ __forceinline__ void stage(unsigned i) const {
        if (i < yblk) {
            const unsigned s = i / ybps;
            stage_block(y_src((int)s), yspan, lds + s * a.yslot, i - s * ybps);
        } else {
            const unsigned s = (i - yblk) / cbps;
            stage_block(c_src((int)s), cspan, lds_c + s * a.cslot, i - yblk - s * cbps);
        }
    }
    // a tapped row: its Y span, and the U and V of the chroma row under it
    struct Row {
        const unsigned char *ly, *lu, *lv;
    };
    __device__ __forceinline__ Row row(int yr, int) const {
        const int cr = ((oy + ys0 + yr) >> 1) - cr0;
        Row w;
        w.ly = span_base(lds + (unsigned)yr * a.yslot, y_src(yr));
        w.lu = span_base(lds_c + (unsigned)cr * a.cslot, c_src(cr));
        w.lv = a.planar ? span_base(lds_c + (unsigned)(crows + cr) * a.cslot, c_src(crows + cr)) : w.lu + 1;
        return w;
    }
    __device__ __forceinline__ void decode(const Row& w, int x, float (&o)[K]) const {
        const int p = (((ox + x) >> 1) - ps0) * cstep;
        yuv_to_bgr<LIT>(a.rule, w.ly[x - xs0], w.lu[p], w.lv[p], o);
    }
};

// ------------------------------------------------------------------------------------------------------ packed 4-byte-unit sources
// Frames whose rows are 4-byte units, uint8, any alignment:
//   KIND 0 YUY2 (n, h, w, 2), w even: a row is w / 2 groups Y0 U Y1 V;   KIND 1 UYVY: groups U Y0 V Y1 -- a camera's or a capture card's
//          packed YUV 4:2:2: pixel (y, x) has luma Y[x & 1] of group x / 2 of row y and that group's (U, V) (no chroma interpolation) and
//          goes to B, G, R by yuv_to_bgr, the one integer rule of the 4:2:0 sources above; h may be odd;
//   KIND 2 BGRX (n, h, w, 4): B, G, R are bytes 0, 1, 2 of a pixel;      KIND 3 RGBX: bytes 2, 1, 0 -- a screen capture's or a read-back's
//          four-byte pixels; byte 3 is never read into the result; any h, w.
// The uint8 B, G, R image that gives is then resized, reversed and scaled exactly as a U8 NHWC source is above.  tests/packed_ref.py is
// the rule in numpy.
//
// A tile stages, for every source row ys0..ys1, ONE span of whole units: units (ox + xs0) >> 1 .. (ox + xs1) >> 1 of the ABSOLUTE columns
// for 4:2:2 (a tile or a rectangle may start on an odd column), units ox + xs0 .. ox + xs1 for the X kinds.  A pixel is decoded where it
// is tapped -- four decodes per output pixel under resize, one without --, the three channels of a quad come from one pass over its taps,
// and the byte positions inside a unit are compile-time constants of KIND.
struct PackedArgs : TileArgs {
    unsigned slot;            // LDS bytes per staged row span (a multiple of 16)
    YuvRule rule;             // kinds 0 and 1
};

// B, G, R of the pixel at column x of its rectangle (absolute column ox + x), from the row span `l` whose first unit is unit u0.
template <int KIND, bool LIT = false>
__device__ __forceinline__ void packed_to_bgr(const YuvRule& k, const unsigned char* l, int ox, int x, int u0, float (&o)[3]) {
    if (KIND < 2) {
        const int ax = ox + x;
        const unsigned char* g = l + 4 * ((ax >> 1) - u0);
        constexpr int Y = KIND == 0 ? 0 : 1, U = KIND == 0 ? 1 : 0, V = KIND == 0 ? 3 : 2;
        yuv_to_bgr<LIT>(k, g[Y + 2 * (ax & 1)], g[U], g[V], o);
    } else {
        const unsigned char* g = l + 4 * (ox + x - u0);
        o[0] = (float)g[KIND == 2 ? 0 : 2];
        o[1] = (float)g[1];
        o[2] = (float)g[KIND == 2 ? 2 : 0];
    }
}

// ROI: a 4:2:2 pixel keeps the chroma of its ABSOLUTE column pair, so a rectangle may start on an odd x and have an odd w.  (No copy
// path for a rectangle of the destination's extent: the pixels are bytes.)  Kinds 2 and 3 convert nothing: they have the LIT form only.
template <int KIND, bool LIT = true>
struct PackedSource {
    using Args = PackedArgs;
    template <bool L>
    using Lit = PackedSource<KIND, L || KIND >= 2>;
    static constexpr int K = 3;
    static constexpr bool YUV = KIND < 2;

    static int check(const Job& j, Args& a) {
        PVHIP_CHECK_ARG(!YUV || j.src_w % 2 == 0);                                   // 4:2:2: one (U, V) per column pair
        a.rule = j.rule ? *j.rule : kYuvRules[0][0];
        return PVHIP_OK;
    }
    // e consecutive columns lie in at most e / 2 + 1 groups of 4:2:2 (the first may be an odd one), and in e units of an X kind
    static size_t units(const Args& a, size_t e) { return !YUV ? e : (e / 2 + 1 < (size_t)a.ws / 2 ? e / 2 + 1 : (size_t)a.ws / 2); }
    static size_t slot_bytes(const Args& a, size_t cols) { return slot_for(units(a, cols) * 4); }
    static size_t stage_bytes(const Args& a, size_t rows, size_t cols) { return rows * slot_bytes(a, cols); }
    static void set_slots(Args& a, size_t cols) { a.slot = (unsigned)slot_bytes(a, cols); }

    const Args& a;
    int ox, oy, ys0;              // the rectangle's corner in the frame; the first staged row
    unsigned char* lds;
    int rows, u0, span;           // staged rows; the first unit of every one of them, and their bytes
    size_t row_bytes;
    const unsigned char* frame;
    unsigned bps;                 // 16-byte blocks a span touches at most

    __device__ __forceinline__ static int channels(const Args&) { return K; }
    static constexpr bool kCopies = false;

    __device__ __forceinline__ PackedSource(const Args& a, const Tile& t, const Tables& tb, unsigned char* lds)
        : a(a), ox(t.ox), oy(t.oy), ys0(tb.ys0), lds(lds), rows(tb.ys1 - tb.ys0 + 1), u0(YUV ? (t.ox + tb.xs0) >> 1 : t.ox + tb.xs0),
          span(((YUV ? (t.ox + tb.xs1) >> 1 : t.ox + tb.xs1) - u0 + 1) * 4), row_bytes((size_t)a.ws * (YUV ? 2 : 4)),
          frame(a.src + (size_t)t.img * ((size_t)a.hs * row_bytes)), bps((unsigned)span / 16 + 2) {}
    static constexpr int kGroups = 1;
    __device__ __forceinline__ int groups() const { return 1; }
    __device__ __forceinline__ bool fits() const { return span_fits(span, a.slot) && (size_t)rows * a.slot <= a.stage_bytes; }
    __device__ __forceinline__ const unsigned char* row_src(int r) const { return frame + (size_t)(oy + ys0 + r) * row_bytes + (size_t)u0 * 4; }
    __device__ __forceinline__ unsigned blocks() const { return (unsigned)rows * bps; }
    __device__ __forceinline__ void stage(unsigned i) const {
        const unsigned s = i / bps;
        stage_block(row_src((int)s), span, lds + s * a.slot, i - s * bps);
    }
    struct Row {
        const unsigned char* l;
    };
    __device__ __forceinline__ Row row(int r, int) const {
        return Row{span_base(lds + (unsigned)r * a.slot, row_src(r))};
    }
    __device__ __forceinline__ void decode(const Row& w, int x, float (&o)[K]) const { packed_to_bgr<KIND, LIT>(a.rule, w.l, ox, x, u0, o); }
};

// ---------------------------------------------------------------------------------------------------- the tile body, the kernels
// One workgroup's tile, steps 1 to 4 of the file comment, for any source.  dynamic LDS: stage_bytes + Tables::bytes(tw, th).
// ROI (with RESIZE): image n is a rectangle of a frame; FIT (with RESIZE): the source is fitted into the destination and padded (see
// the file comment).  VS: finish_quad.  The interpolation is the file comment's, in its order; a tile without resize, and one that
// copies(), takes the one tap as it is.
template <class Source, bool CROP>
__device__ __forceinline__ bool copies_of(const Tile& t) {
    if constexpr (Source::kCopies) return Source::template copies<CROP>(t);
    else return false;
}

template <class Source, bool RESIZE, bool VS, bool ROI, bool FIT>
__device__ __forceinline__ void staged_tile(const typename Source::Args& a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int K = Source::K;
    const int c = Source::channels(a);
    Tile t;
    if (!tile_of<ROI, FIT>(a, c, t)) return;
    const bool one_tap = !RESIZE || copies_of<Source, ROI || FIT>(t);      // (workgroup-uniform)
    const Tables tb = fill_tables<FIT>(lds, a, t, [&](int d, int S, int D) {
        if constexpr (Source::kCopies) return one_tap ? tap<false>(d, S, D) : tap<RESIZE>(d, S, D);
        else return tap<RESIZE>(d, S, D);
    });
    const Source src(a, t, tb, lds);
    if (FIT && !src.fits()) {                                 // (never, by Reach's bound)
        fill_tile<false>(a, c, t, __builtin_nanf(""));
        return;
    }
    for (unsigned i = threadIdx.x; i < src.blocks(); i += kBlock) src.stage(i);
    __syncthreads();

    const int nq = (t.twv + 3) >> 2;
    const size_t plane_out = (size_t)a.hd * a.wd;
    float* out_n = a.dst + (size_t)t.n * c * plane_out;
    for (int i = threadIdx.x; i < t.thv * nq; i += kBlock) {
        const int r = i / nq, j0 = 4 * (i - r * nq);
        const float fy = tb.rfy[r], gy = 1.0f - fy;
        const bool rin = !FIT || row_inside(t, r);
        const int r0 = tb.ry0[r] - tb.ys0, r1 = tb.ry1[r] - tb.ys0;   // the two tapped rows, among the staged ones
        float* o = out_n + (size_t)(t.ty0 + r) * a.wd + t.tx0 + j0;
        // output channels g K .. g K + K - 1 read source group g, under reversal the last group first and its channels backwards
        int g = 0;
        do {                                                  // (kGroups == 1: no loop is emitted at all, the colour kernels' form)
            const int sg = a.reverse ? src.groups() - 1 - g : g;
            const typename Source::Row w0 = src.row(r0, sg), w1 = src.row(r1, sg);
            float v[K][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u < t.twv ? j0 + u : j0;   // (a pixel past the tile computes column j0 again and is not stored)
                const int xa = tb.cx0[j], xb = tb.cx1[j];
                float p00[K];
                src.decode(w0, xa, p00);
                if (Source::kCopies ? !one_tap : RESIZE) {
                    const float fx = tb.cfx[j], gx = 1.0f - fx;
                    float p01[K], p10[K], p11[K];
                    src.decode(w0, xb, p01);
                    src.decode(w1, xa, p10);
                    src.decode(w1, xb, p11);
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const float top = gx * p00[k] + fx * p01[k];
                        const float bot = gx * p10[k] + fx * p11[k];
                        v[k][u] = gy * top + fy * bot;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < K; ++k) v[k][u] = p00[k];
                }
                if (FIT && !(rin && col_inside(t, j0 + u))) {
#pragma unroll
                    for (int k = 0; k < K; ++k) v[k][u] = a.pad;
                }
            }
#pragma unroll
            for (int k = 0; k < K; ++k, o += plane_out) {
                float w[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) w[u] = a.reverse ? v[K - 1 - k][u] : v[k][u];
                finish_quad<VS>(a, g * K + k, w, o, j0, t.twv);
            }
        } while (Source::kGroups != 1 && ++g < src.groups());
    }
}

// The kernels: the body over each source, and kernel_of: the kernel of a source's form.
template <class>
struct Type {};

template <bool U8, bool RESIZE, bool VS, bool ROI, bool FIT = false>
__global__ __launch_bounds__(kBlock) void preprocess_kernel(PrepArgs a) {
    staged_tile<RawSource<U8>, RESIZE, VS, ROI, FIT>(a);
}

template <bool RESIZE, bool VS, bool ROI, bool FIT = false, bool LIT = true>
__global__ __launch_bounds__(kBlock) void preprocess_yuv_kernel(YuvArgs a) {
    staged_tile<Yuv420Source<LIT>, RESIZE, VS, ROI, FIT>(a);
}

template <int KIND, bool RESIZE, bool VS, bool ROI, bool FIT = false, bool LIT = true>
__global__ __launch_bounds__(kBlock) void preprocess_packed_kernel(PackedArgs a) {
    staged_tile<PackedSource<KIND, LIT>, RESIZE, VS, ROI, FIT>(a);
}

template <bool RESIZE, bool VS, bool ROI, bool FIT, bool U8>
constexpr auto kernel_of(Type<RawSource<U8>>) { return preprocess_kernel<U8, RESIZE, VS, ROI, FIT>; }
template <bool RESIZE, bool VS, bool ROI, bool FIT, bool LIT>
constexpr auto kernel_of(Type<Yuv420Source<LIT>>) { return preprocess_yuv_kernel<RESIZE, VS, ROI, FIT, LIT>; }
template <bool RESIZE, bool VS, bool ROI, bool FIT, int KIND, bool LIT>
constexpr auto kernel_of(Type<PackedSource<KIND, LIT>>) { return preprocess_packed_kernel<KIND, RESIZE, VS, ROI, FIT, LIT>; }

// ------------------------------------------------------------------------------------------------------------------ affine warps
// Image b is frame id of m frames sampled through the 2 x 3 matrix of row b of `table` = n x (id, A00, A01, C0, A10, A11, C1), int64,
// the coefficients in Q16 (the warp entry; the rule is in the file comment and, in numpy, in tests/warp_ref.py).
struct WarpArgs : TileArgs {
    const long long* table;
    int c;
    YuvRule rule;             // the colour formats
};

// The tile of a workgroup: kWarpTileW x kWarpTileH output pixels of one image, a quad of one row per lane (kBlock quads).  See the
// file comment for the choice; -DPVHIP_WARP_TILE_W=64 builds the 64 x 16 alternative scripts/bench_warp_input.py compares it with.
#ifndef PVHIP_WARP_TILE_W
#define PVHIP_WARP_TILE_W 32
#endif
constexpr int kWarpTileW = PVHIP_WARP_TILE_W, kWarpQuads = kWarpTileW / 4, kWarpTileH = kBlock / kWarpQuads;
static_assert(kWarpTileW % 4 == 0 && kBlock % kWarpQuads == 0, "a tile is whole quads, one per lane");

// The fetch functors: one frame of the launch's format.  f(r, col, s0, step, kn, p): p[k] = source channel s0 + k step of the pixel at
// row r, column col of the frame, k < kn <= K (K output channels are produced per pass over the taps; colour formats have K = c = 3).
// (r, col) is inside the frame.
template <bool U8, bool NHWC>
struct RawFetch {
    static constexpr int K = 4;
    const unsigned char *frame, *end4;                        // end4: where the last 4 bytes of the m frames start (NULL: fewer than 4)
    int hs, ws, c;
    __device__ RawFetch(const WarpArgs& a, int id)
        : frame(a.src + (size_t)id * ((size_t)a.c * a.hs * a.ws) * (U8 ? 1 : 4)),
          end4((size_t)a.m * a.c * a.hs * a.ws >= 4 ? a.src + (size_t)a.m * a.c * a.hs * a.ws - 4 : nullptr), hs(a.hs), ws(a.ws), c(a.c) {}
    __device__ __forceinline__ void operator()(int r, int col, int s0, int step, int kn, float (&p)[K]) const {
        // NHWC: the channels of a tap lie side by side
        const int e = NHWC ? (r * ws + col) * c + s0 : (s0 * hs + r) * ws + col, ke = NHWC ? step : step * hs * ws;
        if (U8 && NHWC && end4 != nullptr) {
            // ... for bytes within 4 consecutive ones: ONE 32-bit load at any alignment, moved back where it would pass the frames' end
            const unsigned char* lo = frame + e + (step < 0 ? 1 - kn : 0);
            const unsigned char* at = lo < end4 ? lo : end4;
            unsigned w;
            __builtin_memcpy(&w, at, 4);
            const int first = (int)(lo - at);
#pragma unroll
            for (int k = 0; k < K; ++k) p[k] = k < kn ? (float)((w >> (8 * (first + (step < 0 ? kn - 1 - k : k)))) & 255u) : 0.0f;
            return;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) p[k] = k < kn ? pixel<U8>(frame, e + k * ke) : 0.0f;
    }
};

// B, G, R in the order the output channels take them.
__device__ __forceinline__ void bgr_in_order(const float (&o)[3], int step, float (&p)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = step < 0 ? o[2 - k] : o[k];
}

template <bool PLANAR>
struct Yuv420Fetch {
    static constexpr int K = 3;
    const unsigned char *frame, *chroma;
    int ws, hw, vplane;
    const YuvRule& rule;
    __device__ Yuv420Fetch(const WarpArgs& a, int id)
        : frame(a.src + (size_t)id * ((size_t)a.hs * a.ws / 2 * 3)), chroma(frame + (size_t)a.hs * a.ws), ws(a.ws), hw(a.ws >> 1),
          vplane((a.hs >> 1) * (a.ws >> 1)), rule(a.rule) {}
    __device__ __forceinline__ void operator()(int r, int col, int, int step, int, float (&p)[K]) const {
        const unsigned char* cp = PLANAR ? chroma + (r >> 1) * hw + (col >> 1) : chroma + (r >> 1) * ws + 2 * (col >> 1);
        float o[3];
        if (PLANAR) {
            yuv_to_bgr(rule, frame[r * ws + col], cp[0], cp[vplane], o);
        } else {
            unsigned short uv;                                // NV12's (U, V) pair: one 16-bit load at any alignment
            __builtin_memcpy(&uv, cp, 2);
            yuv_to_bgr(rule, frame[r * ws + col], uv & 255, uv >> 8, o);
        }
        bgr_in_order(o, step, p);
    }
};

// A4: the frames are 4-byte aligned, so a unit is one 32-bit load (a frame and a row are whole units); else its bytes one by one.
template <int KIND, bool A4>
struct PackedFetch {
    static constexpr int K = 3;
    const unsigned char* frame;
    int row_bytes;
    const YuvRule& rule;
    __device__ PackedFetch(const WarpArgs& a, int id)
        : frame(a.src + (size_t)id * ((size_t)a.hs * a.ws * (KIND < 2 ? 2 : 4))), row_bytes(a.ws * (KIND < 2 ? 2 : 4)), rule(a.rule) {}
    __device__ __forceinline__ void operator()(int r, int col, int, int step, int, float (&p)[K]) const {
        const int unit = KIND < 2 ? col >> 1 : col;
        const unsigned char* g = frame + (size_t)r * row_bytes + (size_t)unit * 4;
        float o[3];
        if (A4) {
            const unsigned w = *reinterpret_cast<const unsigned*>(g);
            const unsigned char b[4] = {(unsigned char)w, (unsigned char)(w >> 8), (unsigned char)(w >> 16), (unsigned char)(w >> 24)};
            packed_to_bgr<KIND>(rule, b, 0, col, unit, o);
        } else {
            packed_to_bgr<KIND>(rule, g, 0, col, unit, o);
        }
        bgr_in_order(o, step, p);
    }
};

// The taps of one output pixel along one axis: i0 = S >> 16 and i0 + 1 where they lie inside [0, extent) -- compared in 64 bits --,
// else index 0 (a load that is always legal, its value replaced by the pad) with in = false; f the fraction, f == 0 exactly when q == 0.
struct WarpTap {
    int i0, i1, q;
    bool in0, in1;
    float f;
};

__device__ __forceinline__ WarpTap warp_tap(long long s, int extent) {
    const long long i = s >> 16;
    WarpTap t;
    t.in0 = i >= 0 && i < extent;
    t.in1 = i + 1 >= 0 && i + 1 < extent;
    t.i0 = t.in0 ? (int)i : 0;
    t.i1 = t.in1 ? (int)(i + 1) : 0;
    t.q = (int)(s & 0xFFFF);
    t.f = (float)t.q * (1.0f / 65536.0f);
    return t;
}

// The quad of one lane behind its taps (both warp kernels): output columns t.tx0 + j0.. of row t.ty0 + r of image t.n, for every
// channel, pixel u sampled at (ty[u], tx[u]).  WHOLE: no pixel has a second tap (workgroup-uniform): the one tap is copied.
template <class Fetch, bool VS, bool WHOLE>
__device__ __forceinline__ void sample_quad(const WarpArgs& a, const Tile& t, const Fetch& fetch, int r, int j0, const WarpTap (&tx)[4],
                                            const WarpTap (&ty)[4]) {
    constexpr int K = Fetch::K;
    const size_t plane_out = (size_t)a.hd * a.wd;
    float* o = a.dst + (size_t)t.n * a.c * plane_out + (size_t)(t.ty0 + r) * a.wd + t.tx0 + j0;
    for (int oc0 = 0; oc0 < a.c; oc0 += K) {
        const int kn = min(K, a.c - oc0);
        const int s0 = a.reverse ? a.c - 1 - oc0 : oc0, step = a.reverse ? -1 : 1;
        float v[K][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (j0 + u >= t.twv) {                            // (a pixel past the tile is neither fetched nor stored)
#pragma unroll
                for (int k = 0; k < K; ++k) v[k][u] = 0.0f;
                continue;
            }
            const WarpTap &cx = tx[u], &cy = ty[u];
            float p00[K], p01[K], p10[K], p11[K];
            fetch(cy.i0, cx.i0, s0, step, kn, p00);
            if (!WHOLE) {
                fetch(cy.i0, cx.i1, s0, step, kn, p01);
                fetch(cy.i1, cx.i0, s0, step, kn, p10);
                fetch(cy.i1, cx.i1, s0, step, kn, p11);
            }
            const float gx = 1.0f - cx.f, gy = 1.0f - cy.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float q00 = cy.in0 && cx.in0 ? p00[k] : a.pad;
                if (WHOLE) {
                    v[k][u] = q00;
                    continue;
                }
                const float q01 = cy.in0 && cx.in1 ? p01[k] : a.pad, q10 = cy.in1 && cx.in0 ? p10[k] : a.pad;
                const float q11 = cy.in1 && cx.in1 ? p11[k] : a.pad;
                const float top = cx.q == 0 ? q00 : gx * q00 + cx.f * q01;
                const float bot = cx.q == 0 ? q10 : gx * q10 + cx.f * q11;
                v[k][u] = cy.q == 0 ? top : gy * top + cy.f * bot;
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (k < kn) finish_quad<VS>(a, oc0 + k, v[k], o + (size_t)(oc0 + k) * plane_out, j0, t.twv);
    }
}

// The affine front end of a quad: SX, SY of its first pixel, advancing by A00, A10 per pixel.
template <class Fetch, bool VS, bool WHOLE>
__device__ __forceinline__ void warp_quad(const WarpArgs& a, const Tile& t, const Fetch& fetch, int r, int j0, long long sx, long long sy,
                                          long long ax, long long ay) {
    WarpTap tx[4], ty[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        tx[u] = warp_tap(sx + u * ax, a.ws);
        ty[u] = warp_tap(sy + u * ay, a.hs);
    }
    sample_quad<Fetch, VS, WHOLE>(a, t, fetch, r, j0, tx, ty);
}

// The tile of this workgroup and the row of its image in a table of `columns` int64 per image (both warp kernels).  The row is read
// once per workgroup (uniform loads); NULL: the image's id is no frame, the tile is filled with quiet NaN and the workgroup is done.
__device__ __forceinline__ const long long* warp_tile_of(const WarpArgs& a, int columns, Tile& t) {
    t.n = blockIdx.z; t.tx0 = blockIdx.x * kWarpTileW; t.ty0 = blockIdx.y * kWarpTileH;
    t.twv = min(kWarpTileW, a.wd - t.tx0); t.thv = min(kWarpTileH, a.hd - t.ty0);
    const long long* q = a.table + columns * (size_t)t.n;
    if (!(q[0] >= 0 && q[0] < a.m)) {
        fill_tile<false>(a, a.c, t, __builtin_nanf(""));
        return nullptr;
    }
    return q;
}

// grid (ceil(wd / kWarpTileW), ceil(hd / kWarpTileH), n); no LDS.  An image whose id is no frame is filled with quiet NaN and nothing
// of `src` is read for it.
template <class Fetch, bool VS>
__global__ __launch_bounds__(kBlock) void preprocess_warp_kernel(WarpArgs a) {
    Tile t;
    const long long* q = warp_tile_of(a, 7, t);
    if (q == nullptr) return;
    const long long a00 = q[1], a01 = q[2], c0 = q[3], a10 = q[4], a11 = q[5], c1 = q[6];
    const int r = threadIdx.x / kWarpQuads, j0 = 4 * (threadIdx.x % kWarpQuads);
    if (r >= t.thv || j0 >= t.twv) return;
    const long long x = t.tx0 + j0, y = t.ty0 + r;            // (|A| <= 2^26, |C| <= 2^40, x, y < 2^31: below 2^59)
    const long long sx = a00 * x + a01 * y + c0, sy = a10 * x + a11 * y + c1;
    const Fetch fetch(a, (int)q[0]);
    if (((a00 | a01 | c0 | a10 | a11 | c1) & 0xFFFF) == 0) warp_quad<Fetch, VS, true>(a, t, fetch, r, j0, sx, sy, a00, a10);
    else                                                   warp_quad<Fetch, VS, false>(a, t, fetch, r, j0, sx, sy, a00, a10);
}

// ------------------------------------------------------------------------------------------------------------- projective warps
// Image b is frame id of m frames sampled through the homography of row b of `table` = n x (id, Q00 .. Q22), int64, the matrix scaled
// by a power of two of its own (the perspective entry; the rule is in the file comment and, in numpy, in tests/perspective_ref.py).
// The taps of one output pixel whose linear forms are nx, ny and d: SX = floor(nx / d * 65536), SY likewise, in binary64 -- one IEEE
// division each --; a pixel with d == 0 or a position beyond 2^47 (a NaN fails the compares) has no tap inside the frame and no
// fraction: it is the pad.  The conversion to int64 stands behind the range test, so it is defined for every table.
__device__ __forceinline__ void perspective_taps(const WarpArgs& a, long long nx, long long ny, long long d, WarpTap& tx, WarpTap& ty) {
    constexpr double kLimit = 140737488355328.0;              // 2^47: ix, iy below 2^31
    const double den = (double)d;
    const double px = __builtin_floor((double)nx / den * 65536.0), py = __builtin_floor((double)ny / den * 65536.0);
    const bool ok = d != 0 && __builtin_fabs(px) < kLimit && __builtin_fabs(py) < kLimit;
    tx = warp_tap((long long)(ok ? px : 0.0), a.ws);
    ty = warp_tap((long long)(ok ? py : 0.0), a.hs);
    if (!ok) {                                                // (index 0: the load that is always legal)
        tx.in0 = tx.in1 = ty.in0 = ty.in1 = false;
        tx.i1 = ty.i1 = 0;
    }
}

// The grid and the tile of preprocess_warp_kernel.  NX, NY and D advance by Q00, Q10 and Q20 per pixel; there is no WHOLE form.  The
// device cannot check the table's limit: the forms are computed in unsigned arithmetic, which wraps, so a table beyond it gives other
// pixels and nothing undefined; every index still passes warp_tap's 64-bit range test.
template <class Fetch, bool VS>
__global__ __launch_bounds__(kBlock) void preprocess_perspective_kernel(WarpArgs a) {
    typedef unsigned long long u64;
    Tile t;
    const long long* q = warp_tile_of(a, 10, t);
    if (q == nullptr) return;
    const u64 q00 = q[1], q01 = q[2], q02 = q[3], q10 = q[4], q11 = q[5], q12 = q[6], q20 = q[7], q21 = q[8], q22 = q[9];
    const int r = threadIdx.x / kWarpQuads, j0 = 4 * (threadIdx.x % kWarpQuads);
    if (r >= t.thv || j0 >= t.twv) return;
    const u64 x = t.tx0 + j0, y = t.ty0 + r;
    const u64 nx = q00 * x + q01 * y + q02, ny = q10 * x + q11 * y + q12, d = q20 * x + q21 * y + q22;
    WarpTap tx[4], ty[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) perspective_taps(a, (long long)(nx + u * q00), (long long)(ny + u * q10), (long long)(d + u * q20), tx[u], ty[u]);
    const Fetch fetch(a, (int)q[0]);
    sample_quad<Fetch, VS, false>(a, t, fetch, r, j0, tx, ty);
}

template <class Fetch>
void launch_warp(const WarpArgs& a, dim3 grid, bool vs, bool perspective, hipStream_t st) {
    if (perspective) {
        if (vs) hipLaunchKernelGGL((preprocess_perspective_kernel<Fetch, true>), grid, dim3(kBlock), 0, st, a);
        else    hipLaunchKernelGGL((preprocess_perspective_kernel<Fetch, false>), grid, dim3(kBlock), 0, st, a);
        return;
    }
    if (vs) hipLaunchKernelGGL((preprocess_warp_kernel<Fetch, true>), grid, dim3(kBlock), 0, st, a);
    else    hipLaunchKernelGGL((preprocess_warp_kernel<Fetch, false>), grid, dim3(kBlock), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------------------- launchers
// What every launcher checks of a Job, and the members of `a` that follow from it alone.
int common_args(TileArgs& a, const Job& j) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(j.src != nullptr && j.dst != nullptr);
    PVHIP_CHECK_ARG(j.n > 0 && j.n <= 65535 && j.c > 0 && j.src_h > 0 && j.src_w > 0 && j.dst_h > 0 && j.dst_w > 0);
    PVHIP_CHECK_ARG((size_t)j.src_h * (size_t)j.src_w * (size_t)j.c < ((size_t)1 << 31));   // one image's elements index in 32 bits
    PVHIP_CHECK_ARG((size_t)j.dst_h * (size_t)j.dst_w * (size_t)j.c < ((size_t)1 << 31));
    PVHIP_CHECK_ARG(j.m >= 1 && j.roi_h >= 1 && j.roi_h <= j.src_h && j.roi_w >= 1 && j.roi_w <= j.src_w);
    a.src = (const unsigned char*)j.src; a.dst = j.dst; a.mean = j.mean; a.std_scale = j.std_scale;
    a.hs = j.src_h; a.ws = j.src_w; a.hd = j.dst_h; a.wd = j.dst_w; a.reverse = j.reverse ? 1 : 0;
    a.rois = j.rois; a.m = j.m; a.mh = j.roi_h; a.mw = j.roi_w; a.fit = j.fit.fit; a.pad = j.fit.pad;
    return PVHIP_OK;
}

// Source rows (columns) a tile of t destination rows (columns) reads at most, of S onto D: the taps advance by S/D per step.
size_t extent(bool resize, int t, int S, int D) {
    if (!resize) return (size_t)t;
    const size_t e = ((size_t)(t - 1) * (size_t)S + (size_t)D - 1) / (size_t)D + 2;
    return e < (size_t)S ? e : (size_t)S;
}

// What a tile reads along both axes: rows(t) / cols(t) source rows (columns) at most for t destination rows (columns).  Without a fit
// that is extent() of the launch's largest source onto the destination.  With one, the taps of an image run over its own fitted
// rectangle (ih, iw), and a tile of t rows holds t' <= min(t, ih) rows of it, which read at most min(hs, ceil((t' - 1) hs / ih) + 2)
// source rows (extent()'s argument: i0 advances by at most ceil(k hs / ih) over k steps, i1 <= i0 + 1); so a bound on the step hs / ih
// of every image of the launch bounds the tile:
//   whole images  (ih, iw) is known here: the steps are src_h / ih and src_w / iw exactly;
//   ROI           the rectangle (hs, ws) <= (mh, mw) is device data.  Let r = hs wd / ws.  Wide (ws hd >= hs wd, so r <= hd): iw = wd, the
//                 column step is ws / wd <= mw / wd; ih = floor(r + 1/2) unclamped from above, and either ih = 1 -- then t' = 1 and the tile
//                 reads 2 rows at most, below any bound of this form -- or r >= 3/2 and ih >= r - 1/2 >= r / 2, so hs / ih <= 2 hs / r =
//                 2 ws / wd <= 2 mw / wd.  Tall: the same with the axes swapped: row step hs / hd <= mh / hd, column step <= 2 mh / hd.
//                 Hence rows step <= max(mh / hd, 2 mw / wd), columns step <= max(mw / wd, 2 mh / hd), each capped by (mh, mw).
// The kernels check the slots they were given all the same and write NaN rather than stage past them.
struct Reach {
    bool fit, resize;
    int S_h, S_w, D_h, D_w;                // !fit: extent()'s arguments
    size_t rn, rd, cn, cd;                 // fit: the row and column steps rn / rd, cn / cd
    static size_t by(int t, size_t num, size_t den, int cap) {
        const size_t e = ((size_t)(t - 1) * num + den - 1) / den + 2;      // (t < 2^31, num < 2^33)
        return e < (size_t)cap ? e : (size_t)cap;
    }
    size_t rows(int t) const { return fit ? by(t, rn, rd, S_h) : extent(resize, t, S_h, D_h); }
    size_t cols(int t) const { return fit ? by(t, cn, cd, S_w) : extent(resize, t, S_w, D_w); }
};

Reach reach_of(const TileArgs& a, bool roi, bool resize) {
    Reach r{a.fit != 0, resize, a.mh, a.mw, a.hd, a.wd, 0, 1, 0, 1};
    if (!r.fit) return r;
    if (!roi) {
        const FitRect f = fit_rect(a.hs, a.ws, a.hd, a.wd, a.fit);
        r.rn = (size_t)a.hs; r.rd = (size_t)f.ih; r.cn = (size_t)a.ws; r.cd = (size_t)f.iw;
        return r;
    }
    const size_t mh = (size_t)a.mh, mw = (size_t)a.mw, hd = (size_t)a.hd, wd = (size_t)a.wd;
    if (mh * wd >= 2 * mw * hd) { r.rn = mh; r.rd = hd; } else { r.rn = 2 * mw; r.rd = wd; }
    if (mw * hd >= 2 * mh * wd) { r.cn = mw; r.cd = wd; } else { r.cn = 2 * mh; r.cd = hd; }
    return r;
}

struct TilePlan {
    dim3 grid;
    size_t lds;
    bool vs;
};

// The tiles of a launch of n images: a.tw, a.th, a.stage_bytes and the launch's grid, LDS bytes and store form.  stage_of(tw, th): the
// bytes a tile of that size stages; with its coordinate tables it has to fit the budget.
template <class StageOf>
int plan_tiles(TileArgs& a, int n, StageOf stage_of, TilePlan& p) {
    auto lds_of = [&](int tw, int th) { return stage_of(tw, th) + Tables::bytes(tw, th); };
    int tw = a.wd;                         // whole rows, unless one row's sources do not fit
    while (tw > 1 && lds_of(tw, 1) > kStageBudget) tw = tw > 4 ? (((tw + 1) / 2 + 3) & ~3) : tw - 1;
    int th = 2 * kBlock / ((tw + 3) / 4);  // about two quads per lane
    th = th < 1 ? 1 : (th > a.hd ? a.hd : th);
    while (th > 1 && lds_of(tw, th) > kStageBudget) th = (th + 1) / 2;
    PVHIP_CHECK_ARG(lds_of(tw, th) <= kStageBudget);
    p.grid = dim3((unsigned)((a.wd + tw - 1) / tw), (unsigned)((a.hd + th - 1) / th), (unsigned)n);
    PVHIP_CHECK_ARG(p.grid.y <= 65535);
    p.lds = lds_of(tw, th);
    p.vs = (uintptr_t)a.dst % 16 == 0 && a.wd % 4 == 0 && tw % 4 == 0;
    a.tw = tw; a.th = th; a.stage_bytes = (unsigned)stage_of(tw, th);
    return PVHIP_OK;
}

template <bool B>
using Flag = std::integral_constant<bool, B>;

// The form of a staged launch as compile-time flags: f(RESIZE, VS, ROI, FIT, LIT), over the five (RESIZE, ROI, FIT) that exist.
template <class F>
void with_form(bool resize, bool roi, bool fit, bool vs, bool lit, F f) {
    constexpr Flag<true> yes{};
    constexpr Flag<false> no{};
    auto rest = [&](auto R, auto O, auto T) {
        if (lit) { if (vs) f(R, yes, O, T, yes); else f(R, no, O, T, yes); }
        else     { if (vs) f(R, yes, O, T, no); else f(R, no, O, T, no); }
    };
    if (fit)         { if (roi) rest(yes, yes, yes); else rest(yes, no, yes); }
    else if (roi)    rest(yes, yes, no);
    else if (resize) rest(yes, no, no);
    else             rest(no, no, no);
}

bool resizes(const Job& j) { return j.rois != nullptr || j.fit.fit || j.src_h != j.dst_h || j.src_w != j.dst_w; }

// What a launch of `Source` checks of its Job, in this order, and the members of `a` that follow from the Job alone.
template <class Source>
int checked_args(typename Source::Args& a, const Job& j) {
    const int rc = common_args(a, j);
    return rc != PVHIP_OK ? rc : Source::check(j, a);
}

// The one launcher of the staged kernels.  No declared rule: the LIT kernels (with_form also hands a source without a rule, and kinds
// 2 and 3, the flag: their Lit<> is the one form they have).
template <class Source>
int launch_staged(const Job& j) {
    typename Source::Args a;
    int rc = checked_args<Source>(a, j);
    if (rc != PVHIP_OK) return rc;
    const bool roi = j.rois != nullptr, resize = resizes(j);
    const Reach reach = reach_of(a, roi, resize);
    TilePlan p;
    rc = plan_tiles(a, j.n, [&](int tw, int th) { return Source::stage_bytes(a, reach.rows(th), reach.cols(tw)); }, p);
    if (rc != PVHIP_OK) return rc;
    Source::set_slots(a, reach.cols(a.tw));
    hipStream_t st = state().stream;
    with_form(resize, roi, a.fit != 0, p.vs, j.rule == nullptr, [&](auto R, auto V, auto O, auto T, auto L) {
        using Form = typename Source::template Lit<decltype(L)::value>;
        constexpr auto kernel = kernel_of<decltype(R)::value, decltype(V)::value, decltype(O)::value, decltype(T)::value>(Type<Form>{});
        hipLaunchKernelGGL(kernel, p.grid, dim3(kBlock), p.lds, st, a);
    });
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

// U8 / FP32 images.  The format alone is no launch of these kernels: the same bits as the path without preprocessing, after the
// checks of a launch.
template <bool U8>
int launch_raw(const Job& j) {
    if (resizes(j) || j.reverse || j.mean != nullptr || j.std_scale != nullptr) return launch_staged<RawSource<U8>>(j);
    PrepArgs a;
    const int rc = checked_args<RawSource<U8>>(a, j);
    return rc != PVHIP_OK ? rc : pvhip_input_to_nchw_f32(j.src, j.dst, j.n, j.c, j.dst_h, j.dst_w, U8, j.how >> 1);
}

int launch_packed(const Job& j) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(j.how >= 0 && j.how <= 3);   // 0 YUY2, 1 UYVY, 2 BGRX, 3 RGBX
    switch (j.how) {
        case 0:  return launch_staged<PackedSource<0>>(j);
        case 1:  return launch_staged<PackedSource<1>>(j);
        case 2:  return launch_staged<PackedSource<2>>(j);
        default: return launch_staged<PackedSource<3>>(j);
    }
}

// The one launcher of preprocess_warp_kernel and (`perspective`: j.table has ten columns) of preprocess_perspective_kernel: the same
// checks, grid and fetch forms.  format 0 raw, 1 YUV 4:2:0, 2 frames of 4-byte units, with the `how` and the limits of that format's
// source above; the pad is j.fit.pad.
int preprocess_warp_launch(const Job& j, int format, bool perspective) {
    WarpArgs a;
    int rc = common_args(a, j);
    if (rc != PVHIP_OK) return rc;
    const int how = j.how;
    PVHIP_CHECK_ARG(j.table != nullptr);
    PVHIP_CHECK_ARG(j.fit.pad - j.fit.pad == 0.0f);
    PVHIP_CHECK_ARG(format >= 0 && format <= 2);
    PVHIP_CHECK_ARG(format == 0 || j.c == 3);
    PVHIP_CHECK_ARG(how >= 0 && how <= (format == 1 ? 1 : 3));
    if (format == 0) {
        PVHIP_CHECK_ARG(j.c <= kMaxChannels);
        PVHIP_CHECK_ARG((how & 1) || (uintptr_t)j.src % 4 == 0);                     // fp32 sources are element-aligned
    } else if (format == 1) {
        PVHIP_CHECK_ARG(j.src_h % 2 == 0 && j.src_w % 2 == 0);                       // 4:2:0: one (U, V) per 2 x 2 block
    } else {
        PVHIP_CHECK_ARG(how >= 2 || j.src_w % 2 == 0);                               // 4:2:2: one (U, V) per column pair
    }
    const dim3 grid((unsigned)((j.dst_w + kWarpTileW - 1) / kWarpTileW), (unsigned)((j.dst_h + kWarpTileH - 1) / kWarpTileH), (unsigned)j.n);
    PVHIP_CHECK_ARG(grid.y <= 65535);
    a.table = j.table; a.c = j.c; a.rule = j.rule ? *j.rule : kYuvRules[0][0];
    const bool vs = (uintptr_t)j.dst % 16 == 0 && j.dst_w % 4 == 0;
    const bool a4 = (uintptr_t)j.src % 4 == 0;
    hipStream_t st = state().stream;
    switch (format * 8 + how * 2 + (format == 2 && a4 ? 1 : 0)) {
        case 0:  launch_warp<RawFetch<false, false>>(a, grid, vs, perspective, st); break;
        case 2:  launch_warp<RawFetch<true, false>>(a, grid, vs, perspective, st); break;
        case 4:  launch_warp<RawFetch<false, true>>(a, grid, vs, perspective, st); break;
        case 6:  launch_warp<RawFetch<true, true>>(a, grid, vs, perspective, st); break;
        case 8:  launch_warp<Yuv420Fetch<false>>(a, grid, vs, perspective, st); break;
        case 10: launch_warp<Yuv420Fetch<true>>(a, grid, vs, perspective, st); break;
        case 16: launch_warp<PackedFetch<0, false>>(a, grid, vs, perspective, st); break;
        case 17: launch_warp<PackedFetch<0, true>>(a, grid, vs, perspective, st); break;
        case 18: launch_warp<PackedFetch<1, false>>(a, grid, vs, perspective, st); break;
        case 19: launch_warp<PackedFetch<1, true>>(a, grid, vs, perspective, st); break;
        case 20: launch_warp<PackedFetch<2, false>>(a, grid, vs, perspective, st); break;
        case 21: launch_warp<PackedFetch<2, true>>(a, grid, vs, perspective, st); break;
        case 22: launch_warp<PackedFetch<3, false>>(a, grid, vs, perspective, st); break;
        default: launch_warp<PackedFetch<3, true>>(a, grid, vs, perspective, st); break;
    }
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

// The entries' Jobs: whole images (rois NULL: m = n and the maxima are the frame's) or a table's rectangles.
Job job_of(const void* src, float* dst, const int* rois, int n, int m, int c, int src_h, int src_w, int dst_h, int dst_w, int roi_h,
           int roi_w, int how, int reverse_channels, const float* mean, const float* std_scale) {
    return Job{src, dst, rois, n, m, c, src_h, src_w, dst_h, dst_w, roi_h, roi_w, how, reverse_channels, mean, std_scale, Fit{0, 0.0f},
               nullptr, nullptr};
}

int raw_how(int src_u8, int src_nhwc) { return (src_u8 ? 1 : 0) | (src_nhwc ? 2 : 0); }

int launch_raw(const Job& j) { return j.how & 1 ? launch_raw<true>(j) : launch_raw<false>(j); }

// The fitted forms: rois == NULL means whole images.  A fit of whole images that fills the destination is the launch without a fit.
// stretch (the _color_ entries): fit 0 is taken too, and is the launch without a fit whatever pad_value holds.
int set_fit(Job& j, int fit, float pad_value, bool stretch) {
    PVHIP_REQUIRE_INIT();
    const Fit f{fit, pad_value};
    PVHIP_CHECK_ARG(f.ok() || (stretch && fit == 0));
    PVHIP_CHECK_ARG(j.src_h > 0 && j.src_w > 0 && j.dst_h > 0 && j.dst_w > 0);
    if (j.rois == nullptr) { j.m = j.n; j.roi_h = j.src_h; j.roi_w = j.src_w; }
    const FitRect g = fit_rect(j.src_h, j.src_w, j.dst_h, j.dst_w, fit);
    if (fit != 0 && !(j.rois == nullptr && g.iw == j.dst_w && g.ih == j.dst_h)) j.fit = f;
    return PVHIP_OK;
}

// The _color_ entries: the rule kYuvRules[matrix][full_range] in place of BT.601 limited range, which (0, 0) is.
int set_rule(Job& j, int matrix, int full_range) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(matrix >= 0 && matrix <= 2 && (full_range == 0 || full_range == 1));
    j.rule = matrix || full_range ? &kYuvRules[matrix][full_range] : nullptr;
    return PVHIP_OK;
}

// ... of the warp entries: raw frames and four-byte pixels hold nothing to convert.
int set_warp_rule(Job& j, int format, int matrix, int full_range) {
    const int rc = set_rule(j, matrix, full_range);
    if (rc != PVHIP_OK) return rc;
    PVHIP_CHECK_ARG((format != 0 && !(format == 2 && j.how >= 2)) || (matrix == 0 && full_range == 0));
    return PVHIP_OK;
}

}  // namespace

extern "C" {

int pvhip_input_preprocess_f32(const void* src, float* dst, int n, int c, int src_h, int src_w, int dst_h, int dst_w,
                               int src_u8, int src_nhwc, int reverse_channels, const float* mean, const float* std_scale) {
    return launch_raw(job_of(src, dst, nullptr, n, n, c, src_h, src_w, dst_h, dst_w, src_h, src_w, raw_how(src_u8, src_nhwc),
                             reverse_channels, mean, std_scale));
}

int pvhip_input_preprocess_yuv_f32(const void* src, float* dst, int n, int src_h, int src_w, int dst_h, int dst_w, int planar,
                                   int reverse_channels, const float* mean, const float* std_scale) {
    return launch_staged<Yuv420Source<>>(job_of(src, dst, nullptr, n, n, 3, src_h, src_w, dst_h, dst_w, src_h, src_w, planar,
                                                reverse_channels, mean, std_scale));
}

int pvhip_input_preprocess_roi_f32(const void* src, float* dst, const int* rois, int n, int m, int c, int src_h, int src_w, int dst_h,
                                   int dst_w, int max_roi_h, int max_roi_w, int src_u8, int src_nhwc, int reverse_channels,
                                   const float* mean, const float* std_scale) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(rois != nullptr);
    return launch_raw(job_of(src, dst, rois, n, m, c, src_h, src_w, dst_h, dst_w, max_roi_h, max_roi_w, raw_how(src_u8, src_nhwc),
                             reverse_channels, mean, std_scale));
}

int pvhip_input_preprocess_yuv_roi_f32(const void* src, float* dst, const int* rois, int n, int m, int src_h, int src_w, int dst_h,
                                       int dst_w, int max_roi_h, int max_roi_w, int planar, int reverse_channels, const float* mean,
                                       const float* std_scale) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(rois != nullptr);
    return launch_staged<Yuv420Source<>>(job_of(src, dst, rois, n, m, 3, src_h, src_w, dst_h, dst_w, max_roi_h, max_roi_w, planar,
                                                reverse_channels, mean, std_scale));
}

int pvhip_input_preprocess_packed_f32(const void* src, float* dst, int n, int src_h, int src_w, int dst_h, int dst_w, int kind,
                                      int reverse_channels, const float* mean, const float* std_scale) {
    return launch_packed(job_of(src, dst, nullptr, n, n, 3, src_h, src_w, dst_h, dst_w, src_h, src_w, kind, reverse_channels, mean,
                                std_scale));
}

int pvhip_input_preprocess_packed_roi_f32(const void* src, float* dst, const int* rois, int n, int m, int src_h, int src_w, int dst_h,
                                          int dst_w, int max_roi_h, int max_roi_w, int kind, int reverse_channels, const float* mean,
                                          const float* std_scale) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(rois != nullptr);
    return launch_packed(job_of(src, dst, rois, n, m, 3, src_h, src_w, dst_h, dst_w, max_roi_h, max_roi_w, kind, reverse_channels, mean,
                                std_scale));
}

int pvhip_input_preprocess_fit_f32(const void* src, float* dst, const int* rois, int n, int m, int c, int src_h, int src_w, int dst_h,
                                   int dst_w, int max_roi_h, int max_roi_w, int src_u8, int src_nhwc, int reverse_channels,
                                   const float* mean, const float* std_scale, int fit, float pad_value) {
    Job j = job_of(src, dst, rois, n, m, c, src_h, src_w, dst_h, dst_w, max_roi_h, max_roi_w, raw_how(src_u8, src_nhwc), reverse_channels,
                   mean, std_scale);
    const int rc = set_fit(j, fit, pad_value, false);
    return rc != PVHIP_OK ? rc : launch_raw(j);
}

int pvhip_input_preprocess_yuv_fit_f32(const void* src, float* dst, const int* rois, int n, int m, int src_h, int src_w, int dst_h,
                                       int dst_w, int max_roi_h, int max_roi_w, int planar, int reverse_channels, const float* mean,
                                       const float* std_scale, int fit, float pad_value) {
    Job j = job_of(src, dst, rois, n, m, 3, src_h, src_w, dst_h, dst_w, max_roi_h, max_roi_w, planar, reverse_channels, mean, std_scale);
    const int rc = set_fit(j, fit, pad_value, false);
    return rc != PVHIP_OK ? rc : launch_staged<Yuv420Source<>>(j);
}

int pvhip_input_preprocess_packed_fit_f32(const void* src, float* dst, const int* rois, int n, int m, int src_h, int src_w, int dst_h,
                                          int dst_w, int max_roi_h, int max_roi_w, int kind, int reverse_channels, const float* mean,
                                          const float* std_scale, int fit, float pad_value) {
    Job j = job_of(src, dst, rois, n, m, 3, src_h, src_w, dst_h, dst_w, max_roi_h, max_roi_w, kind, reverse_channels, mean, std_scale);
    const int rc = set_fit(j, fit, pad_value, false);
    return rc != PVHIP_OK ? rc : launch_packed(j);
}

int pvhip_input_preprocess_yuv_color_f32(const void* src, float* dst, const int* rois, int n, int m, int src_h, int src_w, int dst_h,
                                         int dst_w, int max_roi_h, int max_roi_w, int planar, int reverse_channels, const float* mean,
                                         const float* std_scale, int fit, float pad_value, int matrix, int full_range) {
    Job j = job_of(src, dst, rois, n, m, 3, src_h, src_w, dst_h, dst_w, max_roi_h, max_roi_w, planar, reverse_channels, mean, std_scale);
    int rc = set_rule(j, matrix, full_range);
    if (rc == PVHIP_OK) rc = set_fit(j, fit, pad_value, true);
    return rc != PVHIP_OK ? rc : launch_staged<Yuv420Source<>>(j);
}

int pvhip_input_preprocess_packed_color_f32(const void* src, float* dst, const int* rois, int n, int m, int src_h, int src_w, int dst_h,
                                            int dst_w, int max_roi_h, int max_roi_w, int kind, int reverse_channels, const float* mean,
                                            const float* std_scale, int fit, float pad_value, int matrix, int full_range) {
    Job j = job_of(src, dst, rois, n, m, 3, src_h, src_w, dst_h, dst_w, max_roi_h, max_roi_w, kind, reverse_channels, mean, std_scale);
    int rc = set_rule(j, matrix, full_range);
    if (rc != PVHIP_OK) return rc;
    PVHIP_CHECK_ARG(kind < 2 || (matrix == 0 && full_range == 0));                   // four-byte pixels: nothing to convert
    rc = set_fit(j, fit, pad_value, true);
    return rc != PVHIP_OK ? rc : launch_packed(j);
}

int pvhip_input_preprocess_warp_f32(const void* src, float* dst, const long long* table, int n, int m, int c, int src_h, int src_w,
                                    int dst_h, int dst_w, int format, int how, int reverse_channels, const float* mean,
                                    const float* std_scale, float pad_value) {
    Job j = job_of(src, dst, nullptr, n, m, c, src_h, src_w, dst_h, dst_w, src_h, src_w, how, reverse_channels, mean, std_scale);
    j.table = table; j.fit.pad = pad_value;
    return preprocess_warp_launch(j, format, false);
}

int pvhip_input_preprocess_warp_color_f32(const void* src, float* dst, const long long* table, int n, int m, int c, int src_h, int src_w,
                                          int dst_h, int dst_w, int format, int how, int reverse_channels, const float* mean,
                                          const float* std_scale, float pad_value, int matrix, int full_range) {
    Job j = job_of(src, dst, nullptr, n, m, c, src_h, src_w, dst_h, dst_w, src_h, src_w, how, reverse_channels, mean, std_scale);
    j.table = table; j.fit.pad = pad_value;
    const int rc = set_warp_rule(j, format, matrix, full_range);
    return rc != PVHIP_OK ? rc : preprocess_warp_launch(j, format, false);
}

int pvhip_input_preprocess_perspective_f32(const void* src, float* dst, const long long* table, int n, int m, int c, int src_h, int src_w,
                                           int dst_h, int dst_w, int format, int how, int reverse_channels, const float* mean,
                                           const float* std_scale, float pad_value) {
    Job j = job_of(src, dst, nullptr, n, m, c, src_h, src_w, dst_h, dst_w, src_h, src_w, how, reverse_channels, mean, std_scale);
    j.table = table; j.fit.pad = pad_value;
    return preprocess_warp_launch(j, format, true);
}

int pvhip_input_preprocess_perspective_color_f32(const void* src, float* dst, const long long* table, int n, int m, int c, int src_h,
                                                 int src_w, int dst_h, int dst_w, int format, int how, int reverse_channels,
                                                 const float* mean, const float* std_scale, float pad_value, int matrix, int full_range) {
    Job j = job_of(src, dst, nullptr, n, m, c, src_h, src_w, dst_h, dst_w, src_h, src_w, how, reverse_channels, mean, std_scale);
    j.table = table; j.fit.pad = pad_value;
    const int rc = set_warp_rule(j, format, matrix, full_range);
    return rc != PVHIP_OK ? rc : preprocess_warp_launch(j, format, true);
}

}  // extern "C"
