// Pooling kernels (HBM-bound).  NCHW fp32; lanes run along the output row so the window loads of a
// wave are contiguous (stride sw) segments of input rows and the stores are fully coalesced.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "pvhip_common.h"

using namespace pvhip;

namespace {

struct PoolArgs {
    int n_planes;  // N*C
    int h, w, oh, ow;
    int kh, kw, sh, sw;
    int pt, pl;    // pad top / left
    int hp, wp;    // padded extents (h + pt + pb, w + pl + pr)
};

// MaxPool over the zero-padded input, window clipped at the padded extent (MaxPool.py:41-72):
// a pad cell is a candidate with value 0.0; np.max semantics (NaN wins).
__global__ __launch_bounds__(kBlock) void maxpool2d_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            PoolArgs a, unsigned total) {
    const unsigned stride = gridDim.x * blockDim.x;
    const unsigned ohw    = (unsigned)(a.oh * a.ow);
    for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const unsigned plane = e / ohw;
        const unsigned rem   = e - plane * ohw;
        const int      oy    = (int)(rem / (unsigned)a.ow);
        const int      ox    = (int)(rem - (unsigned)oy * (unsigned)a.ow);
        const float* __restrict__ xp = x + (size_t)plane * (size_t)(a.h * a.w);
        const int py0 = oy * a.sh, px0 = ox * a.sw;  // window origin in padded coordinates
        float     m   = -INFINITY;
        for (int ky = 0; ky < a.kh; ++ky) {
            const int py = py0 + ky;
            if (py >= a.hp) break;
            const int  iy    = py - a.pt;
            const bool row_in = (unsigned)iy < (unsigned)a.h;
            for (int kx = 0; kx < a.kw; ++kx) {
                const int px = px0 + kx;
                if (px >= a.wp) break;
                const int ix = px - a.pl;
                float     v  = 0.0f;
                if (row_in && (unsigned)ix < (unsigned)a.w) v = xp[iy * a.w + ix];
                m = (v > m || v != v) ? v : m;
            }
        }
        y[e] = m;
    }
}

struct PoolDivs {
    FastDiv hw, w, ohw, ow;
};

// First input float of the workgroup that owns the planes from g0 on and the output rows from oy0 on (a one-shot LDS kernel reads
// from there), and whether it lies on a 16-byte boundary.  The kernels and the form queries both ask here.
__host__ __device__ inline size_t band_in_off(int h, int w, int pt, int sh, int g0, int oy0) {
    const int iy_lo = oy0 * sh - pt > 0 ? oy0 * sh - pt : 0;
    return (size_t)g0 * h * w + (size_t)iy_lo * w;
}
__host__ __device__ inline bool start_aligned(int h, int w, int pt, int sh, int g0, int oy0) {
    return (band_in_off(h, w, pt, sh, g0, oy0) & 3) == 0;
}

// What a workgroup of a one-shot LDS kernel owns: the group blockIdx.x of G planes, and of them band `band` of `band_rows` output
// rows (blockIdx.y; bands > 1 only with G == 1, for planes too large to stage whole; `whole`: there is one band).  The LDS image
// holds the PADDED rows [py_lo, py_hi) the band needs.
struct BandGeom {
    int    g0, gn, oy0, oy1;
    bool   whole;             // whole planes: the dense run spans planes, so every row is staged
    int    py_lo, py_hi;
    int    iy_lo, hb;         // input rows [iy_lo, iy_lo + hb) of this band are actually present in the tensor
    int    hwb, obw;          // input / output floats per plane of this band
    int    plane_l;           // floats between padded plane images in LDS
    int    n_in, n_out;
    int    row_shift;         // LDS row of input row iy_lo (0 unless the band starts in the top pad)
    bool   aligned;
    size_t in_off, out_off;
};
__device__ __forceinline__ BandGeom band_geom(const PoolArgs& a, int G, int band_rows, int kh, int band, bool whole) {
    BandGeom b;
    b.g0 = blockIdx.x * G;
    b.gn = min(G, a.n_planes - b.g0);
    b.oy0 = band * band_rows;
    b.oy1 = min(a.oh, b.oy0 + band_rows);
    b.whole = whole;
    b.py_lo = b.oy0 * a.sh;
    b.py_hi = b.whole ? a.hp : min(a.hp, (b.oy1 - 1) * a.sh + kh);
    b.iy_lo = max(0, b.py_lo - a.pt);
    b.hb    = min(a.h, b.py_hi - a.pt) - b.iy_lo;
    b.hwb = b.hb * a.w; b.obw = (b.oy1 - b.oy0) * a.ow;
    b.plane_l = (b.py_hi - b.py_lo) * a.wp;
    b.n_in = b.gn * b.hwb; b.n_out = b.gn * b.obw;
    b.row_shift = b.iy_lo + a.pt - b.py_lo;
    b.in_off  = band_in_off(a.h, a.w, a.pt, a.sh, b.g0, b.oy0);
    b.aligned = start_aligned(a.h, a.w, a.pt, a.sh, b.g0, b.oy0);
    b.out_off = (size_t)b.g0 * a.oh * a.ow + (size_t)b.oy0 * a.ow;
    return b;
}

// A dense run of n floats -> LDS as it is: 16-byte loads where the run starts on a 16-byte boundary, the scalar loop where not.
__device__ __forceinline__ void stage_dense_run(float* tile, const float* __restrict__ xin, int n, bool aligned) {
    if (aligned) {
        const float4* __restrict__ x4 = reinterpret_cast<const float4*>(xin);
        float4* t4 = reinterpret_cast<float4*>(tile);
        const int n4 = n >> 2;
        for (int i = threadIdx.x; i < n4; i += kBlock) t4[i] = x4[i];
        for (int i = (n4 << 2) + threadIdx.x; i < n; i += kBlock) tile[i] = xin[i];
    } else {
        for (int i = threadIdx.x; i < n; i += kBlock) tile[i] = xin[i];
    }
}

// The dense run of a workgroup -> zero-PADDED plane images [py_hi - py_lo][wp] in LDS: zero fill, barrier, then each float to its
// place (16 bytes per load where the run is aligned: one decode per load, running (g, iy, ix) counters for its four floats).
__device__ __forceinline__ void stage_padded_images(float* tile, const float* __restrict__ xin, const PoolArgs& a, const BandGeom& b,
                                                    const PoolDivs& dv) {
    {
        float4* t4 = reinterpret_cast<float4*>(tile);
        const int n4 = (b.gn * b.plane_l + 3) >> 2;   // the allocation is rounded up to 16 bytes
        for (int i = threadIdx.x; i < n4; i += kBlock) t4[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();
    const int wl = a.wp;
    const int n4 = b.aligned ? (b.n_in >> 2) : 0;
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(xin);
    for (int i = threadIdx.x; i < n4; i += kBlock) {
        const float4   v = x4[i];
        const unsigned e = (unsigned)i * 4u;
        unsigned g  = b.whole ? fdiv(e, dv.hw) : 0u;
        unsigned r  = e - g * (unsigned)b.hwb;
        unsigned iy = fdiv(r, dv.w);
        unsigned ix = r - iy * (unsigned)a.w;
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            tile[g * b.plane_l + (iy + b.row_shift) * wl + ix + a.pl] = vv[q];
            if (++ix == (unsigned)a.w) { ix = 0; if (++iy == (unsigned)b.hb) { iy = 0; ++g; } }
        }
    }
    for (int e = (n4 << 2) + threadIdx.x; e < b.n_in; e += kBlock) {
        const unsigned g = b.whole ? fdiv((unsigned)e, dv.hw) : 0u, r = (unsigned)e - g * (unsigned)b.hwb;
        const unsigned iy = fdiv(r, dv.w), ix = r - iy * (unsigned)a.w;
        tile[g * b.plane_l + (iy + b.row_shift) * wl + ix + a.pl] = xin[e];
    }
}

// LDS-staged MaxPool: a workgroup owns G consecutive (n, c) planes.  Planes are contiguous in NCHW, so
// the input of a group is ONE dense run of G*H*W floats: it is read from HBM exactly once with 16-byte
// loads and laid out in LDS as G zero-PADDED planes [hp][wp] (the pad cells hold the 0.0 that takes part
// in the reference's max), so a window is kh*kw unconditional LDS reads.  Lanes own consecutive outputs
// (conflict-free LDS reads at stride 1, 2-way at stride 2); the outputs of a group are again one dense
// run, written coalesced.  CLIP handles ceil-mode windows that overhang the padded extent (those cells
// are excluded from the max, MaxPool.py:69).  np.max semantics: a NaN in the window wins.
template <int KH, int KW, bool CLIP>   // KH == 0: run-time window extent
__global__ __launch_bounds__(kBlock) void maxpool2d_lds_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                PoolArgs a, int G, int band_rows, PoolDivs dv) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int kh = KH ? KH : a.kh, kw = KW ? KW : a.kw;
    const BandGeom b = band_geom(a, G, band_rows, kh, blockIdx.y, gridDim.y == 1);
    const int wl = a.wp;
    float* __restrict__ yout = y + b.out_off;
    if (b.plane_l == b.hwb) stage_dense_run(tile, x + b.in_off, b.n_in, b.aligned);   // no pad cells
    else stage_padded_images(tile, x + b.in_off, a, b, dv);
    __syncthreads();

    for (int o = threadIdx.x; o < b.n_out; o += kBlock) {
        const unsigned g   = b.whole ? fdiv((unsigned)o, dv.ohw) : 0u;
        const unsigned rem = (unsigned)o - g * (unsigned)b.obw;
        const unsigned oyl = fdiv(rem, dv.ow);
        const unsigned ox  = rem - oyl * (unsigned)a.ow;
        const int py0 = (int)(b.oy0 + oyl) * a.sh, px0 = (int)ox * a.sw;
        const float* __restrict__ tp = tile + g * b.plane_l + (py0 - b.py_lo) * wl + px0;
        float m = -INFINITY;             // max3_nan: a NaN in the window IS its maximum
        if (KH != 0) {
#pragma unroll
            for (int ky = 0; ky < (KH ? KH : 1); ++ky) {
                const bool row_ok = !CLIP || (py0 + ky < a.hp);
#pragma unroll
                for (int kx = 0; kx < (KW ? KW : 1); ++kx) {
                    if (row_ok && (!CLIP || (px0 + kx < a.wp))) {
                        const float v = tp[ky * wl + kx];
                        m = max3_nan(m, v, v);
                    }
                }
            }
        } else {
            for (int ky = 0; ky < kh && py0 + ky < a.hp; ++ky)
                for (int kx = 0; kx < kw && px0 + kx < a.wp; ++kx) {
                    const float v = tp[ky * wl + kx];
                    m = max3_nan(m, v, v);
                }
        }
        yout[o] = m;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// 3x3 MaxPool, stride 1 or 2, as a persistent double-buffered pipeline (the GoogLeNet pools: 3x3/s2 ceil and
// 3x3/s1/p1).  Same semantics as maxpool2d_lds_kernel (MaxPool.py:41-72: zero pad cells take part in the max,
// windows are clipped at the padded extent, NaN wins).
//
// A tile is G planes x a band of output rows.  Its input (whole planes: one dense run; bands: one dense run per
// plane) goes global -> LDS by LDS-DMA (16 bytes per lane, no staging registers), and the DMA of tile t+1 is in
// flight while tile t is computed and stored.  The LDS image is the DENSE input (no pad cells): a lane owns one
// output COLUMN of a segment of rows and slides down it, so every input row costs it 3 LDS reads and one
// horizontal max, and an output is the max of three of those row values (3 instead of 9 LDS reads per output at
// stride 1, 6 at stride 2).  Taps outside the tensor are clamped onto a tap of the same window that is inside (a
// duplicate changes no max); a window that touches pad cells inside the padded extent gets max(m, 0) -- the value
// those cells hold in the reference.  The outputs of a tile are collected in LDS and leave as dense 16-byte runs.
struct Pool3Args {
    const float* x;
    float*       y;
    unsigned long long x_bytes;
    int n_planes, h, w, oh, ow;
    int pt, pl, hp, wp;
    int G, S, band_rows, n_bands;   // tile = G planes x band_rows output rows, split over S row segments per column
    int dense;                      // 1: bands == 1, a tile's input is ONE dense run of G*h*w floats
    int plane_l;                    // floats between plane images in LDS (dense: h*w; bands: a multiple of 256)
    int in_floats;                  // floats per input buffer (whole 1-KiB pieces)
    int out_plane_l;                // floats between plane images of the output stage
    int n_tiles;
    int vec_out;                    // 16-byte stores are aligned for every tile
};

template <bool NT>
__device__ __forceinline__ void pool_st4(float* dst, const float* src_lds) {
    const pv_f4v v = *reinterpret_cast<const pv_f4v*>(src_lds);
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<pv_f4v*>(dst));
    else *reinterpret_cast<pv_f4v*>(dst) = v;
}
template <bool NT>
__device__ __forceinline__ void pool_st1(float* dst, float v) {
    if (NT) __builtin_nontemporal_store(v, dst);
    else *dst = v;
}

struct Pool3Divs {
    FastDiv bands, sow, ow;
};

// The column pipeline, shared by maxpool3x3_cols_kernel and dwconv3x3_cols_kernel.  cols_pipeline<Op, ST, STAGE, NT> owns the tile
// decode, the LDS-DMA issue, the wait / barrier / prefetch loop, the item -> (plane, segment, column) decode, the walk down a row
// segment with the last rows in registers, and the output stage.  What a kernel computes is its Op:
//   Op::kAnyAlign                          whether a copy may start off a 16-byte boundary (the LDS image is then shifted)
//   Op::Item  op.item(a, plane, c)         per-item setup (held in registers down the segment)
//   Op::Row   op.row(a, item, L, iy, c)    what a lane keeps of input row iy (row iy of its plane is at L + iy * w; iy may be outside)
//   float     op.finish(a, item, rA, rB, rC, py0)   the output whose window starts at padded row py0, from its three rows
struct ColsTile {
    int g0, gn;          // planes [g0, g0 + gn)
    int oy0, oy1;        // output rows [oy0, oy1)
    int iy_lo, iy_hi;    // input rows [iy_lo, iy_hi) are in the tile's LDS image
};
template <int ST>
__device__ __forceinline__ ColsTile cols_tile(const Pool3Args& a, const Pool3Divs& dv, int t) {
    ColsTile T;
    const int pg = (int)fdiv((unsigned)t, dv.bands), b = t - pg * a.n_bands;
    T.g0 = pg * a.G; T.gn = min(a.G, a.n_planes - T.g0);
    T.oy0 = b * a.band_rows; T.oy1 = min(a.oh, T.oy0 + a.band_rows);
    T.iy_lo = max(0, T.oy0 * ST - a.pt); T.iy_hi = min(a.h, (T.oy1 - 1) * ST + 3 - a.pt);
    return T;
}
// first float of run p of a tile (whole planes: ONE run from plane g0 on, iy_lo is 0; bands: one run per plane); the entries admit
// tensors below 2^31 elements (check_pool_dims), so element indices are 32-bit and only byte counts need more
__device__ __forceinline__ unsigned cols_run_src(const Pool3Args& a, const ColsTile& T, int p) {
    return (unsigned)(T.g0 + p) * (unsigned)(a.h * a.w) + (unsigned)(T.iy_lo * a.w);
}

// Input of tile t -> buffer `dst`: each run in 1-KiB pieces dealt to the four waves.  Each run gets a buffer resource of its own, based at
// the 16-byte boundary at or below its first float (ANY_ALIGN: a 150- or 75-wide row, a 5625-float plane do not start on one; the
// image in LDS is then shifted by the remainder, which the reads add back.  Without ANY_ALIGN the planner admits aligned starts
// only and the shift is a compile-time zero) and as long as the bytes of the tensor left from there.  Only the offset inside the run
// rides in the VECTOR offset, the one that is range-checked (the scalar one is not): the last pieces of the last tile reach past the
// tensor and must read zeros, not the bytes behind the allocation.  The base is a 64-bit address, so nothing here wraps for a tensor
// above 4 GiB (a resource over the whole tensor with the run's start in the 32-bit offset would).
template <bool NT, bool ANY_ALIGN>
__device__ __forceinline__ void cols_issue_run(const Pool3Args& a, unsigned src, int run_f, float* dst) {
    const int      wave   = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned lane16 = (unsigned)(threadIdx.x & 63) * 16u;
    const int      sh     = ANY_ALIGN ? (int)(src & 3) : 0;
    const unsigned left   = (unsigned)(a.x_bytes >> 2) - (src - sh);                     // floats of the tensor from the base on
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.x + (src - sh)), 0, (int)(left > 0x3FFFFFFFu ? 0xFFFFFFFFu : left * 4u), 0x00020000);
    const int pieces = (run_f + sh + 255) >> 8;
    for (int q = wave; q < pieces; q += 4) lds_dma_b128<NT>(r, dst + q * 256, lane16 + (unsigned)q * 1024u, 0u);
}
template <int ST, bool NT, bool ANY_ALIGN>
__device__ __forceinline__ void cols_issue(const Pool3Args& a, const Pool3Divs& dv, int t, float* dst) {
    const ColsTile T = cols_tile<ST>(a, dv, t);
    if (a.dense) {
        cols_issue_run<NT, ANY_ALIGN>(a, cols_run_src(a, T, 0), T.gn * a.h * a.w, dst);
    } else {
        for (int p = 0; p < T.gn; ++p)
            cols_issue_run<NT, ANY_ALIGN>(a, cols_run_src(a, T, p), (T.iy_hi - T.iy_lo) * a.w, dst + p * a.plane_l);
    }
}

// The outputs of a tile, collected in LDS at outb, leave as dense runs (16-byte stores where every tile's runs are aligned).
// (Whole planes take a branch of their own here and in cols_issue, not a loop of one run: as one loop the store loops were no
// longer unrolled and the GoogLeNet pools ran 3 % slower, profiles/pool_refactor.md)
template <bool NT>
__device__ __forceinline__ void cols_store_run(float* yd, const float* so, int run, bool vec, int tid) {
    if (vec) {
        const int n4 = run >> 2;
        for (int i = tid; i < n4; i += kBlock) pool_st4<NT>(yd + 4 * i, so + 4 * i);
        for (int i = (n4 << 2) + tid; i < run; i += kBlock) pool_st1<NT>(yd + i, so[i]);
    } else {
        for (int i = tid; i < run; i += kBlock) pool_st1<NT>(yd + i, so[i]);
    }
}
template <bool NT>
__device__ __forceinline__ void cols_store_stage(const Pool3Args& a, const ColsTile& T, const float* outb, int tid) {
    const int ohw = a.oh * a.ow;
    if (a.dense) {
        cols_store_run<NT>(a.y + (size_t)T.g0 * ohw, outb, T.gn * ohw, a.vec_out, tid);
    } else {
        for (int p = 0; p < T.gn; ++p)
            cols_store_run<NT>(a.y + (size_t)(T.g0 + p) * ohw + (size_t)T.oy0 * a.ow, outb + p * a.out_plane_l, (T.oy1 - T.oy0) * a.ow, a.vec_out, tid);
    }
}

struct Cols3 {
    int px0;           // leftmost tap column of the lane's windows (in the left padding when negative)
    int c0, c1, c2;    // the three tap columns clamped onto the tensor
};

template <class Op, int ST, bool STAGE, bool NT>
__device__ __forceinline__ void cols_pipeline(const Pool3Args& a, const Pool3Divs& dv, const Op& op) {
    extern __shared__ __attribute__((aligned(1024))) float lds3[];
    float* const outb = lds3 + 2 * a.in_floats;
    const int tid = threadIdx.x;
    const int ohw = a.oh * a.ow;

    int t = blockIdx.x, cur = 0;
    if (t < a.n_tiles) cols_issue<ST, NT, Op::kAnyAlign>(a, dv, t, lds3);
    for (; t < a.n_tiles; t += gridDim.x) {
        lds_dma_wait_all();
        __syncthreads();          // tile t has landed; every wave is done with the other buffer and with the output stage
        {
            const int tn = t + (int)gridDim.x;
            if (tn < a.n_tiles) cols_issue<ST, NT, Op::kAnyAlign>(a, dv, tn, lds3 + (cur ^ 1) * a.in_floats);
        }
        const float* const in = lds3 + cur * a.in_floats;
        const ColsTile T = cols_tile<ST>(a, dv, t);
        const int seg_rows = (T.oy1 - T.oy0 + a.S - 1) / a.S;
        const int n_items = T.gn * a.S * a.ow;
        const int sow = a.S * a.ow;
        for (int it = tid; it < n_items; it += kBlock) {
            const unsigned p = fdiv((unsigned)it, dv.sow), rem = (unsigned)it - p * (unsigned)sow;
            const unsigned seg = fdiv(rem, dv.ow), ox = rem - seg * (unsigned)a.ow;
            const int ys = T.oy0 + (int)seg * seg_rows, ye = min(T.oy1, ys + seg_rows);
            if (ys >= T.oy1) continue;                                        // trailing segment of a short band
            Cols3 c;
            c.px0 = (int)ox * ST - a.pl;
            c.c0 = min(max(c.px0, 0), a.w - 1); c.c1 = min(max(c.px0 + 1, 0), a.w - 1); c.c2 = min(max(c.px0 + 2, 0), a.w - 1);
            const typename Op::Item item = op.item(a, T.g0 + (int)p, c);
            // input row iy of this plane at L + iy * w (the copy started `shift` floats below the run)
            const int shift = Op::kAnyAlign ? (int)(cols_run_src(a, T, a.dense ? 0 : (int)p) & 3) : 0;
            const float* const L = in + (int)p * a.plane_l + shift - T.iy_lo * a.w;
            typename Op::Row rA, rB, rC;
            rA = op.row(a, item, L, ys * ST - a.pt, c);
            if (ST == 1) rB = op.row(a, item, L, ys - a.pt + 1, c);
            float* const yo = STAGE ? outb + (int)p * a.out_plane_l + (ys - T.oy0) * a.ow + (int)ox
                                    : a.y + (size_t)(T.g0 + (int)p) * ohw + (size_t)ys * a.ow + ox;
            for (int oy = ys; oy < ye; ++oy) {
                if (ST == 2) rB = op.row(a, item, L, oy * 2 - a.pt + 1, c);
                rC = op.row(a, item, L, oy * ST - a.pt + 2, c);
                yo[(oy - ys) * a.ow] = op.finish(a, item, rA, rB, rC, oy * ST);
                if (ST == 1) { rA = rB; rB = rC; }
                else         { rA = rC; }
            }
        }
        if (STAGE) {
            __syncthreads();
            cols_store_stage<NT>(a, T, outb, tid);
        }
        cur ^= 1;
    }
}

// MaxPool: a lane keeps the horizontal max of a row's three taps; an output is the max of three of them and of the zero floor.
struct MaxPool3Op {
    static constexpr bool kAnyAlign = false;
    struct Item { float flr_c; };      // 0.0 where the column's windows touch pad cells inside the padded extent, else -inf
    typedef float Row;
    __device__ __forceinline__ Item item(const Pool3Args& a, int, const Cols3& c) const {
        const bool zc = (c.px0 < 0) || (min(c.px0 + a.pl + 2, a.wp - 1) - a.pl >= a.w);
        return Item{zc ? 0.0f : -INFINITY};
    }
    __device__ __forceinline__ Row row(const Pool3Args& a, const Item&, const float* L, int iy, const Cols3& c) const {
        const float* q = L + min(max(iy, 0), a.h - 1) * a.w;
        const float  v0 = q[c.c0], v1 = q[c.c1], v2 = q[c.c2];
        return max3_nan(v0, v1, v2);           // a NaN in the row IS its maximum, as for np.max
    }
    __device__ __forceinline__ float finish(const Pool3Args& a, const Item& item, Row hA, Row hB, Row hC, int py0) const {
        const float m  = max3_nan(hA, hB, hC);
        const bool  zr = (py0 < a.pt) || (min(py0 + 2, a.hp - 1) - a.pt >= a.h);
        const float fl = zr ? 0.0f : item.flr_c;
        return max3_nan(m, fl, fl);
    }
};

template <int ST, bool STAGE, bool NT>
__global__ __launch_bounds__(kBlock) void maxpool3x3_cols_kernel(Pool3Args a, Pool3Divs dv) {
    cols_pipeline<MaxPool3Op, ST, STAGE, NT>(a, dv, MaxPool3Op{});
}


// Tile geometry for maxpool3x3_cols_kernel, or false when the shape is not its (the caller falls back).
// Env overrides for tuning runs: PVHIP_POOL3=0 disables, PVHIP_POOL3_CFG="G,S,band_rows", PVHIP_POOL3_KB (LDS budget
// of one input buffer), PVHIP_POOL3_STAGE=0 (direct stores), PVHIP_POOL3_WG (workgroups per CU of the persistent grid).
struct Pool3Plan {
    Pool3Args a;
    size_t    lds;
    int       grid;
    bool      stage;
};

// any_align: the caller's kernel copies from the 16-byte boundary below a band / group start and reads its LDS image shifted by the
// remainder (dwconv3x3_cols_kernel), so starts need not be 16-byte aligned (odd widths, 150-wide rows)
bool plan_pool3_search(const float* x, float* y, int planes, int h, int w, int oh, int ow, int st, int pt, int pl, int hp, int wp,
                Pool3Plan& out, bool any_align = false, int stage_override = -1) {
    if (pt > 2 || pl > 2 || (oh - 1) * st > pt + h - 1 || (ow - 1) * st > pl + w - 1) return false;   // clamped taps stay in their window
    if (ow > kBlock || hp < pt + h || wp < pl + w) return false;
    const int hw = h * w, ohw = oh * ow;
    const Settings& cfg = settings();                   // PVHIP_POOL3_KB / _STAGE / _CFG / _WG: tuning runs only
    const size_t budget = (size_t)cfg.pool3_kb * 1024;
    const bool stage = stage_override >= 0 ? stage_override != 0 : cfg.pool3_stage != 0;
    int G = cfg.pool3_g, S = cfg.pool3_s, band = cfg.pool3_band;
    const bool forced = G > 0 && S > 0 && band > 0;
    const bool need4 = !any_align && ((hw % 4 != 0) || (ohw % 4 != 0));      // group starts must stay 16-byte aligned
    if (!forced) {
        double best = -1.0;
        const size_t row_b = (size_t)w * 4;
        for (int nb = 1; nb <= oh; ++nb) {                    // number of bands
            const int br = (oh + nb - 1) / nb;
            if ((oh + br - 1) / br != nb) continue;
            const int rows_in = (nb == 1) ? h : min(h, (br - 1) * st + 3);
            if (nb > 1 && (w % 4 != 0) && !any_align) break;  // band starts must be 16-byte aligned
            const size_t plane_b = (size_t)rows_in * row_b;
            if (plane_b > 2 * budget) continue;
            const double halo_eff = (nb == 1) ? 1.0 : (double)(br * st) / (double)((br - 1) * st + 3);
            for (int g = 1; g <= 64 && (size_t)g * plane_b <= budget + budget / 2; ++g) {
                if (g > planes) break;
                if (need4 && nb == 1 && (g % 4 != 0) && g != planes) continue;
                if (need4 && nb > 1) continue;
                // any_align (depthwise): the plan must fit as it is (two input buffers + the output stage in 64 KB: a stride-1 layer's
                // output is as large as its input), and tiles whose outputs start on 16-byte boundaries are preferred
                bool   fits = true;
                double vec_eff = 1.0;
                if (any_align) {
                    const size_t in_f  = (nb == 1) ? (((size_t)g * hw + 3 + 255) & ~(size_t)255) : (size_t)g * (((size_t)rows_in * w + 3 + 255) & ~(size_t)255);
                    const size_t out_f = (nb == 1) ? (size_t)g * ohw : (size_t)g * br * ow;
                    fits = in_f * 8 + (stage ? ((out_f + 3) & ~(size_t)3) * 4 : 0) <= 64 * 1024;
                    const bool vec = (nb == 1) ? ((size_t)g * ohw % 4 == 0 || g == planes) : (ohw % 4 == 0 && (br * ow) % 4 == 0);
                    vec_eff = vec ? 1.0 : 0.8;
                    if (nb > 1 && (w & 1)) vec_eff *= 0.6;       // bands of odd-width planes start on no boundary at all (measured: slow)
                }
                if (!fits) break;
                for (int s = 1; s <= 8 && s <= br; ++s) {
                    const int items = g * s * ow;
                    const int sr = (br + s - 1) / s;
                    const double util = (double)items / (double)(((items + kBlock - 1) / kBlock) * kBlock);
                    const double seg_eff = (double)br / (double)(s * sr) * ((double)(sr * st) / (double)(sr * st + 3 - st));
                    const double size_eff = (double)((size_t)g * plane_b) / (double)((size_t)g * plane_b + 2048);   // per-tile overhead
                    const double sc = util * seg_eff * halo_eff * size_eff * vec_eff;
                    if (sc > best) { best = sc; G = g; S = s; band = br; }
                }
            }
            if (nb == 1 && best > 0.0 && (size_t)h * row_b <= budget) break;   // whole planes fit: no bands
        }
        if (best < 0.0) return false;
    }
    Pool3Args a{};
    a.x = x; a.y = y; a.n_planes = planes; a.h = h; a.w = w; a.oh = oh; a.ow = ow; a.pt = pt; a.pl = pl; a.hp = hp; a.wp = wp;
    a.x_bytes = (unsigned long long)planes * hw * 4ull;
    if (G > planes) G = planes;
    a.G = G; a.S = S; a.band_rows = band; a.n_bands = (oh + band - 1) / band;
    a.dense = (a.n_bands == 1);
    if (!a.dense && !any_align && (w % 4 != 0 || need4)) return false;
    if (a.dense && need4 && (G % 4 != 0) && G != planes) return false;
    const int rows_in = a.dense ? h : min(h, (band - 1) * st + 3);
    const int slack = any_align ? 3 : 0;               // the copy starts up to three floats below the first one
    a.plane_l     = a.dense ? hw : ((rows_in * w + slack + 255) & ~255);
    a.in_floats   = a.dense ? ((G * hw + slack + 255) & ~255) : G * a.plane_l;
    a.out_plane_l = a.dense ? ohw : band * ow;
    a.n_tiles     = ((planes + G - 1) / G) * a.n_bands;
    a.vec_out     = a.dense ? (((size_t)G * ohw % 4 == 0 || G == planes) ? 1 : 0) : ((ohw % 4 == 0) && ((band * ow) % 4 == 0));
    const size_t out_b = stage ? (size_t)((G * a.out_plane_l + 3) & ~3) * 4 : 0;
    out.lds = (size_t)a.in_floats * 8 + out_b;
    if (out.lds > 64 * 1024 || G * S * ow <= 0) return false;
    int per_cu = (int)((size_t)(160 * 1024) / out.lds);
    if (per_cu > 8) per_cu = 8;
    if (per_cu < 1) per_cu = 1;
    if (cfg.pool3_wg > 0) per_cu = cfg.pool3_wg;
    out.grid  = min(a.n_tiles, per_cu * kNumCU);
    out.a     = a;
    out.stage = stage;
    return true;
}

// The search above costs tens of microseconds; a forward pass asks for the same few shapes over and over.
bool plan_pool3(const float* x, float* y, int planes, int h, int w, int oh, int ow, int st, int pt, int pl, int hp, int wp,
                Pool3Plan& out, bool any_align = false, int stage_override = -1) {
    if (!settings().pool3) return false;
    struct Entry { int key[12]; bool ok; Pool3Plan plan; };
    static std::vector<Entry> cache;
    const int key[12] = {planes, h, w, oh, ow, st, pt, pl, hp, wp, settings().generation, (any_align ? 1 : 0) + 2 * (stage_override + 1)};
    for (const Entry& e : cache)
        if (memcmp(e.key, key, sizeof key) == 0) {
            if (!e.ok) return false;
            out = e.plan; out.a.x = x; out.a.y = y;
            return true;
        }
    Entry e{};              // (a plan that is refused prints as zeros)
    memcpy(e.key, key, sizeof key);
    e.ok = plan_pool3_search(x, y, planes, h, w, oh, ow, st, pt, pl, hp, wp, e.plan, any_align, stage_override);
    if (settings().pool3_verbose)
        fprintf(stderr, "pool3 planes=%d %dx%d->%dx%d s%d: %s G=%d S=%d band=%d bands=%d tiles=%d lds=%zu grid=%d\n", planes, h, w, oh, ow, st,
                e.ok ? "ok" : "fallback", e.plan.a.G, e.plan.a.S, e.plan.a.band_rows, e.plan.a.n_bands, e.plan.a.n_tiles, e.plan.lds, e.plan.grid);
    if (cache.size() >= 256) cache.clear();
    cache.push_back(e);
    if (!e.ok) return false;
    out = e.plan;
    return true;
}


// AvgPool with the reference's window rule (AvgPool.py:56): rows [oy*sh, min(h-1, oy*sh+kh)),
// cols [ox*sw, min(w-1, ox*sw+kw)), no padding; mean = sum / count in fp32; empty window -> NaN.
__global__ __launch_bounds__(kBlock) void avgpool2d_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            PoolArgs a, unsigned total) {
    const unsigned stride = gridDim.x * blockDim.x;
    const unsigned ohw    = (unsigned)(a.oh * a.ow);
    for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const unsigned plane = e / ohw;
        const unsigned rem   = e - plane * ohw;
        const int      oy    = (int)(rem / (unsigned)a.ow);
        const int      ox    = (int)(rem - (unsigned)oy * (unsigned)a.ow);
        const float* __restrict__ xp = x + (size_t)plane * (size_t)(a.h * a.w);
        const int y0 = oy * a.sh, x0 = ox * a.sw;
        int       y1 = y0 + a.kh, x1 = x0 + a.kw;
        if (y1 > a.h - 1) y1 = a.h - 1;
        if (x1 > a.w - 1) x1 = a.w - 1;
        float sum = 0.0f;
        int   cnt = 0;
        for (int iy = y0; iy < y1; ++iy)
            for (int ix = x0; ix < x1; ++ix) {
                sum += xp[iy * a.w + ix];
                ++cnt;
            }
        y[e] = (cnt > 0) ? sum / (float)cnt : NAN;
    }
}

// LDS-staged AvgPool for small planes (the 7x7 global pool of the classifiers): a workgroup streams G whole
// planes (one dense run) into LDS with 16-byte loads, then one lane per output averages its window from LDS.
// Same window rule as avgpool2d_kernel (AvgPool.py:56), same sequential fp32 sum.
__global__ __launch_bounds__(kBlock) void avgpool2d_lds_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                PoolArgs a, int G, PoolDivs dv) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int hw = a.h * a.w, ohw = a.oh * a.ow;
    const BandGeom b = band_geom(a, G, a.oh, a.kh, 0, true);     // whole planes, no padding
    stage_dense_run(tile, x + b.in_off, b.n_in, b.aligned);
    __syncthreads();
    for (int o = threadIdx.x; o < b.n_out; o += kBlock) {
        const unsigned g   = fdiv((unsigned)o, dv.ohw);
        const unsigned rem = (unsigned)o - g * (unsigned)ohw;
        const unsigned oy  = fdiv(rem, dv.ow);
        const unsigned ox  = rem - oy * (unsigned)a.ow;
        const float* __restrict__ tp = tile + g * hw;
        const int y0 = (int)oy * a.sh, x0 = (int)ox * a.sw;
        int       y1 = y0 + a.kh, x1 = x0 + a.kw;
        if (y1 > a.h - 1) y1 = a.h - 1;
        if (x1 > a.w - 1) x1 = a.w - 1;
        float sum = 0.0f;
        int   cnt = 0;
        for (int iy = y0; iy < y1; ++iy)
            for (int ix = x0; ix < x1; ++ix) {
                sum += tp[iy * a.w + ix];
                ++cnt;
            }
        y[b.out_off + o] = (cnt > 0) ? sum / (float)cnt : NAN;
    }
}

// Depthwise convolution (GroupConvolution.py:53-79, one input and one output channel per group), LDS-staged
// like MaxPool: a workgroup owns G consecutive (n, channel) planes (or a band of output rows of one plane), the
// zero-PADDED image in LDS makes every tap an unconditional LDS read, the kh*kw weights of the group's planes sit
// in LDS too.  Optional fused epilogue: + bias[channel], then ReLU or clamp (the Add / Clamp nodes that follow
// every depthwise layer of the MobileNet backbone).
struct DwEpilogue {
    const float* bias;   // [channels] or nullptr
    int          act;    // 0 none, 1 ReLU, 2 clamp
    float        lo, hi;
};
// the bias of channel ch; -0.0 for none (x + -0.0 is x, bit for bit, for every x)
__device__ __forceinline__ float dw_bias(const DwEpilogue& ep, int ch) { return ep.bias != nullptr ? ep.bias[ch] : -0.0f; }
__device__ __forceinline__ float dw_epilogue(float sum, float bv, const DwEpilogue& ep) {
    sum = sum + bv;
    if (ep.act == 1) sum = (sum < 0.0f) ? 0.0f : sum;
    else if (ep.act == 2) { sum = (sum < ep.lo) ? ep.lo : sum; sum = (sum > ep.hi) ? ep.hi : sum; }
    return sum;
}

template <int KH, int KW>   // 0 = run-time extent
__global__ __launch_bounds__(kBlock) void dwconv2d_lds_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                               float* __restrict__ y, PoolArgs a, int channels, int G,
                                                               int band_rows, PoolDivs dv, DwEpilogue ep) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int kh = KH ? KH : a.kh, kw = KW ? KW : a.kw;
    const BandGeom b = band_geom(a, G, band_rows, kh, blockIdx.y, gridDim.y == 1);
    const int wl = a.wp;
    float* __restrict__ yout = y + b.out_off;
    float* wts = tile + ((b.gn * b.plane_l + 3) & ~3);       // [gn][kh*kw] after the images
    {   // the weights of this group's planes
        const int kk = kh * kw;
        for (int i = threadIdx.x; i < b.gn * kk; i += kBlock) {
            const int g = i / kk, t = i - g * kk;
            wts[i] = w[(size_t)((b.g0 + g) % channels) * kk + t];
        }
    }
    stage_padded_images(tile, x + b.in_off, a, b, dv);
    __syncthreads();

    for (int o = threadIdx.x; o < b.n_out; o += kBlock) {
        const unsigned g   = b.whole ? fdiv((unsigned)o, dv.ohw) : 0u;
        const unsigned rem = (unsigned)o - g * (unsigned)b.obw;
        const unsigned oyl = fdiv(rem, dv.ow);
        const unsigned ox  = rem - oyl * (unsigned)a.ow;
        const int py0 = (int)(b.oy0 + oyl) * a.sh, px0 = (int)ox * a.sw;
        const float* __restrict__ tp = tile + g * b.plane_l + (py0 - b.py_lo) * wl + px0;
        const float* __restrict__ wg = wts + g * (kh * kw);
        float sum = 0.0f;
        if (KH != 0) {
#pragma unroll
            for (int ky = 0; ky < (KH ? KH : 1); ++ky)
#pragma unroll
                for (int kx = 0; kx < (KW ? KW : 1); ++kx) sum += tp[ky * wl + kx] * wg[ky * (KW ? KW : 1) + kx];
        } else {
            for (int ky = 0; ky < kh; ++ky)
                for (int kx = 0; kx < kw; ++kx) sum += tp[ky * wl + kx] * wg[ky * kw + kx];
        }
        yout[o] = dw_epilogue(sum, dw_bias(ep, (b.g0 + (int)g) % channels), ep);
    }
}

// Depthwise 3x3 (stride 1 or 2) on the column pipeline of maxpool3x3_cols_kernel (same planner, same tiles): persistent grid, the dense
// input of tile t + 1 arrives by LDS-DMA (nontemporal, 16 bytes per lane) while tile t is computed; a lane owns one output COLUMN of a row
// segment and slides down it with the last rows' three taps in registers (stride 1: three LDS reads per output instead of nine, and
// no LDS reads for the weights: the nine weights of the lane's plane sit in registers; a tap in the padding reads as 0.0);
// outputs meet in LDS and leave as dense 16-byte nontemporal runs.  The one-shot kernel above zeroes a padded LDS image, fills it
// through registers with three divisions per 16 bytes, reads 18 LDS words per output and stores 4 bytes per lane: 2.3-3.5 TB/s on the
// MobileNet layers.  Same products in the same order (ky, then kx; a padded tap is 0 * w): the same bits.
// STAGE = false (stride-1 layers whose planes fill LDS twice over as it is: MobileNet's 75x75): a lane stores its outputs itself
struct DwConv3Op {
    static constexpr bool kAnyAlign = true;
    const float* wts;
    int          channels;
    DwEpilogue   ep;
    // the plane's nine weights in registers; a tap in the padding reads as 0.0 (the VALUE is masked, as in the reference's padded
    // image: 0 * w -- masking the weight instead would turn an infinite neighbour into NaN)
    struct Item { bool m0, m1, m2; float wk[9], bv; };
    struct Row { float v0, v1, v2; };      // the three taps of an input row (zeros for a row in the padding)
    __device__ __forceinline__ Item item(const Pool3Args& a, int plane, const Cols3& c) const {
        const int ch = plane % channels;
        Item it;
        it.m0 = (unsigned)c.px0 < (unsigned)a.w; it.m1 = (unsigned)(c.px0 + 1) < (unsigned)a.w; it.m2 = (unsigned)(c.px0 + 2) < (unsigned)a.w;
#pragma unroll
        for (int k = 0; k < 9; ++k) it.wk[k] = wts[ch * 9 + k];
        it.bv = dw_bias(ep, ch);
        return it;
    }
    __device__ __forceinline__ Row row(const Pool3Args& a, const Item& it, const float* L, int iy, const Cols3& c) const {
        const bool   ok = (unsigned)iy < (unsigned)a.h;
        const float* q  = L + min(max(iy, 0), a.h - 1) * a.w;
        return Row{(ok && it.m0) ? q[c.c0] : 0.0f, (ok && it.m1) ? q[c.c1] : 0.0f, (ok && it.m2) ? q[c.c2] : 0.0f};
    }
    __device__ __forceinline__ float finish(const Pool3Args&, const Item& it, const Row& ra, const Row& rb, const Row& rc, int) const {
        float sum = 0.0f;
        sum += ra.v0 * it.wk[0]; sum += ra.v1 * it.wk[1]; sum += ra.v2 * it.wk[2];
        sum += rb.v0 * it.wk[3]; sum += rb.v1 * it.wk[4]; sum += rb.v2 * it.wk[5];
        sum += rc.v0 * it.wk[6]; sum += rc.v1 * it.wk[7]; sum += rc.v2 * it.wk[8];
        return dw_epilogue(sum, it.bv, ep);
    }
};

template <int ST, bool NT, bool STAGE = true>
__global__ __launch_bounds__(kBlock) void dwconv3x3_cols_kernel(Pool3Args a, Pool3Divs dv, const float* __restrict__ wts, int channels,
                                                                 DwEpilogue ep) {
    cols_pipeline<DwConv3Op, ST, STAGE, NT>(a, dv, DwConv3Op{wts, channels, ep});
}

// Direct fallback (planes whose bands do not fit LDS): one lane per output.
struct DwArgs {
    int G, H, W, OH, OW, kh, kw, sh, sw, pt, pl;
};
__global__ __launch_bounds__(kBlock) void dwconv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         float* __restrict__ y, DwArgs a, unsigned total, DwEpilogue ep) {
    const unsigned stride = gridDim.x * blockDim.x;
    const unsigned ohw    = (unsigned)(a.OH * a.OW);
    for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const unsigned plane = e / ohw;  // n*G + g
        const unsigned rem   = e - plane * ohw;
        const int      oy    = (int)(rem / (unsigned)a.OW);
        const int      ox    = (int)(rem - (unsigned)oy * (unsigned)a.OW);
        const int      g     = (int)(plane % (unsigned)a.G);
        const float* __restrict__ xp = x + (size_t)plane * (size_t)(a.H * a.W);
        const float* __restrict__ wg = w + (size_t)g * (a.kh * a.kw);
        const int iy0 = oy * a.sh - a.pt, ix0 = ox * a.sw - a.pl;
        float     sum = 0.0f;
        for (int r = 0; r < a.kh; ++r) {
            const int iy = iy0 + r;
            if ((unsigned)iy >= (unsigned)a.H) continue;
            for (int s = 0; s < a.kw; ++s) {
                const int ix = ix0 + s;
                if ((unsigned)ix >= (unsigned)a.W) continue;
                sum += xp[iy * a.W + ix] * wg[r * a.kw + s];
            }
        }
        y[e] = dw_epilogue(sum, dw_bias(ep, g), ep);
    }
}

int check_pool_dims(const char* who, int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh, int sw) {
    if (n < 0 || c < 0 || h <= 0 || w <= 0 || oh < 0 || ow < 0 || kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0)
        return fail(PVHIP_EINVAL, "%s: bad dims n=%d c=%d h=%d w=%d oh=%d ow=%d k=%dx%d s=%dx%d", who, n, c, h, w, oh, ow,
                    kh, kw, sh, sw);
    const unsigned long long in_e  = (unsigned long long)n * c * h * w;
    const unsigned long long out_e = (unsigned long long)n * c * oh * ow;
    if (in_e >= (1ull << 31) || out_e >= (1ull << 31))
        return fail(PVHIP_EUNSUPPORTED, "%s: tensor exceeds 2^31 elements", who);
    return PVHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Launch plans.  Which kernel form a pooling / depthwise launch takes is decided HERE and nowhere else: the compute entries
// switch on the plan, the pvhip_*_form queries (no device needed) report it.  No pointer is read; x / y only travel into the
// argument block of the column kernels.

// nontemporal accesses from the size on where the tensors cannot stay in L2 for the consumer anyway (PVHIP_STREAM_NT)
bool stream_nt(int planes, int h, int w, int oh, int ow) {
    const int ntm = settings().stream_nt;
    return ntm == 2 || (ntm == 1 && (size_t)planes * ((size_t)h * w + (size_t)oh * ow) * 4 >= ((size_t)64 << 20));
}

// Groups of whole planes, or bands of one plane, for a one-shot LDS kernel: several whole (padded) planes per workgroup when planes
// are small, bands of output rows of one plane when a plane is larger than `budget` bytes of LDS.  rows_l: padded rows per image.
struct GroupBand {
    int G, band_rows, n_bands, rows_l;
};
GroupBand choose_group_band(size_t plane_bytes, size_t row_bytes, int kh, int sh, int oh, size_t budget, int hw, int planes) {
    GroupBand gb{1, oh, 1, 0};
    const int hp = (int)(plane_bytes / row_bytes);
    if (plane_bytes <= budget) {
        int G = (int)(budget / plane_bytes);
        while (G > 4 && (planes + G - 1) / G < 8 * kNumCU) G >>= 1;
        if (hw % 4 != 0 && G >= 4) G &= ~3;          // every group starts 16-byte aligned in HBM
        if (G > planes) G = planes;
        gb.G = G;
    } else {
        const size_t min_band = (size_t)(kh + sh) * row_bytes;       // at least two output rows per band
        const size_t fit      = budget > min_band ? budget : min_band;
        const int    rows_in  = (int)(fit / row_bytes);              // padded input rows per band: >= kh + sh, so band_rows >= 2
        int band_rows = (rows_in - kh) / sh + 1;
        if (band_rows > oh) band_rows = oh;
        int n_bands = (oh + band_rows - 1) / band_rows;
        band_rows = (oh + n_bands - 1) / n_bands;                    // even out the bands
        gb.band_rows = band_rows;
        gb.n_bands   = (oh + band_rows - 1) / band_rows;
    }
    gb.rows_l = (gb.n_bands == 1) ? hp : ((gb.band_rows - 1) * sh + kh < hp ? (gb.band_rows - 1) * sh + kh : hp);
    return gb;
}

struct MaxPoolPlan {
    int       kind = PVHIP_MAXPOOL_GLOBAL;
    int       G = 1, band_rows = 0, n_bands = 1;
    bool      clip = false, nt = false;
    size_t    lds = 0;
    Pool3Plan p3{};            // PVHIP_MAXPOOL_COLS_*
};

MaxPoolPlan plan_maxpool(const float* x, float* y, const PoolArgs& a) {
    MaxPoolPlan p;
    const int planes = a.n_planes, h = a.h, w = a.w, oh = a.oh, ow = a.ow, kh = a.kh, kw = a.kw, sh = a.sh, sw = a.sw;
    p.band_rows = oh;
    if (kh == 3 && kw == 3 && sh == sw && (sh == 1 || sh == 2) &&
        plan_pool3(x, y, planes, h, w, oh, ow, sh, a.pt, a.pl, a.hp, a.wp, p.p3)) {
        p.kind = sh == 1 ? PVHIP_MAXPOOL_COLS_S1 : PVHIP_MAXPOOL_COLS_S2;
        p.G = p.p3.a.G; p.band_rows = p.p3.a.band_rows; p.n_bands = p.p3.a.n_bands;
        p.lds = p.p3.lds;
        p.nt  = stream_nt(planes, h, w, oh, ow);
        return p;
    }
    // LDS-staged path.  ~16 KB of LDS per workgroup (8-10 workgroups per CU overlap each other's load and
    // compute phases; measured best on the GoogLeNet shapes).
    const size_t group_bytes = (size_t)settings().pool_lds_kb * 1024;       // PVHIP_POOL_LDS_KB: tuning runs only
    const size_t row_bytes   = (size_t)a.wp * sizeof(float);
    if ((size_t)(kh + sh) * row_bytes > 60 * 1024) return p;        // not even two output rows fit: one lane per output
    const GroupBand gb = choose_group_band((size_t)a.hp * row_bytes, row_bytes, kh, sh, oh, group_bytes, h * w, planes);
    p.lds = (((size_t)gb.G * gb.rows_l * row_bytes) + 15) & ~(size_t)15;
    // lds > 64 KB needs PVHIP_POOL_LDS_KB above 64: whole planes take G * plane_bytes <= group_bytes, and a band holds
    // rows_l <= (band_rows - 1) * sh + kh <= rows_in rows (evening the bands out only shrinks band_rows), i.e. at most
    // max(group_bytes, (kh + sh) * row_bytes) <= 60 KB at the default of 16.  More than 65535 bands: a plane of 131070 rows
    // and more whose rows are wider than 16 KB / (kh + sh).
    if (p.lds > 64 * 1024 || gb.n_bands > 65535) return p;
    p.kind = (kh == 3 && kw == 3) ? PVHIP_MAXPOOL_LDS_3X3 : (kh == 2 && kw == 2) ? PVHIP_MAXPOOL_LDS_2X2 : PVHIP_MAXPOOL_LDS;
    p.G = gb.G; p.band_rows = gb.band_rows; p.n_bands = gb.n_bands;
    p.clip = ((oh - 1) * sh + kh > a.hp) || ((ow - 1) * sw + kw > a.wp);
    return p;
}

struct AvgPoolPlan {
    int    kind = PVHIP_AVGPOOL_GLOBAL;
    int    G = 1;
    size_t lds = 0;
};

AvgPoolPlan plan_avgpool(const PoolArgs& a) {
    AvgPoolPlan p;
    const size_t plane_bytes = (size_t)a.h * a.w * sizeof(float);
    if (plane_bytes > 16 * 1024) return p;               // whole planes only
    p.kind = PVHIP_AVGPOOL_LDS;
    p.G    = choose_group_band(plane_bytes, (size_t)a.w * sizeof(float), a.kh, a.sh, a.oh, 16 * 1024, a.h * a.w, a.n_planes).G;
    p.lds  = (((size_t)p.G * plane_bytes) + 15) & ~(size_t)15;
    return p;
}

struct DwPlan {
    int       kind = PVHIP_DWCONV_GLOBAL;
    int       G = 1, band_rows = 0, n_bands = 1;
    bool      nt = false;
    size_t    lds = 0;
    Pool3Plan p3{};            // PVHIP_DWCONV_COLS_*
};

// a.hp / a.wp: everything the windows touch (cells past the tensor are zeros by definition)
DwPlan plan_dwconv(const float* x, float* y, const PoolArgs& a) {
    DwPlan p;
    const int planes = a.n_planes, h = a.h, wdt = a.w, oh = a.oh, ow = a.ow, kh = a.kh, kw = a.kw, sh = a.sh, sw = a.sw;
    p.band_rows = oh;
    // 3x3, stride 1 or 2: the pipelined kernel on the MaxPool kernel's tiles (PVHIP_DWCONV_COLS=0: the one-shot LDS kernel)
    if (kh == 3 && kw == 3 && sh == sw && (sh == 1 || sh == 2) && settings().dwconv_cols) {
        // The lanes store their outputs themselves (PVHIP_DWCONV_COLS=2: through the MaxPool kernel's output stage in LDS, measured
        // slower on every MobileNet layer: 1.32 against 1.16 ms over the 13 -- the stage costs LDS, i.e. halo rows and resident tiles).
        // (bands of odd-width planes start on no boundary at all and ran 20 % slower than the one-shot kernel; MobileNet's 75x75
        // planes fit whole)
        const bool ok = plan_pool3(x, y, planes, h, wdt, oh, ow, sh, a.pt, a.pl, a.hp, a.wp, p.p3, true, settings().dwconv_cols == 2 ? 1 : 0) &&
                        !(p.p3.a.n_bands > 1 && (wdt & 1));
        if (ok) {
            p.kind = sh == 1 ? PVHIP_DWCONV_COLS_S1 : PVHIP_DWCONV_COLS_S2;
            p.G = p.p3.a.G; p.band_rows = p.p3.a.band_rows; p.n_bands = p.p3.a.n_bands;
            p.lds = p.p3.lds;
            p.nt  = stream_nt(planes, h, wdt, oh, ow);
            return p;
        }
    }
    const size_t row_bytes = (size_t)a.wp * sizeof(float);
    if ((size_t)(kh + sh) * row_bytes > 48 * 1024) return p;         // not even two output rows fit: one lane per output
    const GroupBand gb = choose_group_band((size_t)a.hp * row_bytes, row_bytes, kh, sh, oh, 16 * 1024, h * wdt, planes);
    p.lds = ((((size_t)gb.G * gb.rows_l * a.wp + 3) & ~(size_t)3) + (size_t)gb.G * kh * kw) * sizeof(float);
    // lds > 64 KB is REACHABLE here, unlike in plan_maxpool: the image of a band is at most max(16 KB, (kh + sh) * row_bytes) <= 48 KB,
    // but the kh * kw weights sit behind it, and a window of 100 x 100 taps on rows of 100 floats is 40 KB of band plus 40 KB of
    // weights.  More than 65535 bands: as in plan_maxpool.
    if (p.lds > 64 * 1024 || gb.n_bands > 65535) return p;
    p.kind = (kh == 3 && kw == 3) ? PVHIP_DWCONV_LDS_3X3 : PVHIP_DWCONV_LDS;
    p.G = gb.G; p.band_rows = gb.band_rows; p.n_bands = gb.n_bands;
    return p;
}

// Whether EVERY workgroup of an LDS-staged launch starts on a 16-byte boundary of the input (the kernels ask start_aligned for their
// own start: 16-byte loads where it is aligned, the scalar loop where it is not).  For the form queries only.  Group starts: the rule
// the chooser rounds G by.  It says no for groups of 2 or 3 planes of 4k + 2 floats, which do all start aligned; kept, because the
// answers of the form queries are compared with earlier builds bit for bit.  Band starts (bands only with G == 1): the predicate.
int all_starts_aligned(int h, int w, int G, int planes, int n_bands, int band_rows, int sh, int pt) {
    if (!(((size_t)h * w) % 4 == 0 || G % 4 == 0 || G >= planes)) return 0;
    for (int b = 0; b < n_bands; ++b)
        if (!start_aligned(h, w, pt, sh, 0, b * band_rows)) return 0;
    return 1;
}

// One request per entry pair: the arguments checked and the launch planned in ONE place, for pvhip_X_f32 (launch: pointers are
// checked and travel into the plan) and pvhip_X_form alike.  total == 0: nothing is launched.  `who`: the entry, for the messages.
#define POOL_CHECK_ARG(who, cond)                                                                       \
    do {                                                                                                \
        if (!(cond)) return fail(PVHIP_EINVAL, "%s: argument check failed: %s", who, #cond);            \
    } while (0)

struct PoolShape {
    int n, c, h, w, oh, ow, kh, kw, sh, sw;
};
template <class Plan>
struct PoolRequest {
    unsigned total = 0;
    PoolArgs a{};
    Plan     p;
};
typedef PoolRequest<MaxPoolPlan> MaxPoolRequest;
typedef PoolRequest<AvgPoolPlan> AvgPoolRequest;
typedef PoolRequest<DwPlan>      DwRequest;
int maxpool_request(const char* who, bool launch, const float* x, float* y, const PoolShape& s, int pad_top, int pad_left,
                    int pad_bottom, int pad_right, MaxPoolRequest& r) {
    int rc = check_pool_dims(who, s.n, s.c, s.h, s.w, s.oh, s.ow, s.kh, s.kw, s.sh, s.sw);
    if (rc) return rc;
    POOL_CHECK_ARG(who, pad_top >= 0 && pad_left >= 0 && pad_bottom >= 0 && pad_right >= 0);
    const unsigned total = (unsigned)s.n * s.c * s.oh * s.ow;
    if (total == 0) return PVHIP_OK;
    if (launch) POOL_CHECK_ARG(who, x != nullptr && y != nullptr);
    r.a = PoolArgs{s.n * s.c, s.h, s.w, s.oh, s.ow, s.kh, s.kw, s.sh, s.sw, pad_top, pad_left, s.h + pad_top + pad_bottom, s.w + pad_left + pad_right};
    // every window must start inside the padded extent (numpy would raise on an empty np.max)
    if ((s.oh - 1) * s.sh >= r.a.hp || (s.ow - 1) * s.sw >= r.a.wp)
        return fail(PVHIP_EINVAL, "%s: window starts outside the padded input", who);
    r.p = plan_maxpool(x, y, r.a);
    r.total = total;
    return PVHIP_OK;
}

int avgpool_request(const char* who, bool launch, const float* x, float* y, const PoolShape& s, AvgPoolRequest& r) {
    int rc = check_pool_dims(who, s.n, s.c, s.h, s.w, s.oh, s.ow, s.kh, s.kw, s.sh, s.sw);
    if (rc) return rc;
    const unsigned total = (unsigned)s.n * s.c * s.oh * s.ow;
    if (total == 0) return PVHIP_OK;
    if (launch) POOL_CHECK_ARG(who, x != nullptr && y != nullptr);
    r.a = PoolArgs{s.n * s.c, s.h, s.w, s.oh, s.ow, s.kh, s.kw, s.sh, s.sw, 0, 0, s.h, s.w};
    r.p = plan_avgpool(r.a);
    r.total = total;
    return PVHIP_OK;
}

// s.c: groups = channels
int dwconv_request(const char* who, bool launch, const float* x, const float* w, float* y, const PoolShape& s, int pad_top, int pad_left,
                   int act, DwRequest& r) {
    int rc = check_pool_dims(who, s.n, s.c, s.h, s.w, s.oh, s.ow, s.kh, s.kw, s.sh, s.sw);
    if (rc) return rc;
    if (launch) POOL_CHECK_ARG(who, pad_top >= 0 && pad_left >= 0 && act >= 0 && act <= 2);
    else        POOL_CHECK_ARG(who, pad_top >= 0 && pad_left >= 0);
    const unsigned total = (unsigned)s.n * s.c * s.oh * s.ow;
    if (total == 0) return PVHIP_OK;
    if (launch) POOL_CHECK_ARG(who, x != nullptr && w != nullptr && y != nullptr);
    int hp = (s.oh - 1) * s.sh + s.kh, wp = (s.ow - 1) * s.sw + s.kw;
    if (hp < s.h + pad_top) hp = s.h + pad_top;
    if (wp < s.w + pad_left) wp = s.w + pad_left;
    r.a = PoolArgs{s.n * s.c, s.h, s.w, s.oh, s.ow, s.kh, s.kw, s.sh, s.sw, pad_top, pad_left, hp, wp};
    r.p = plan_dwconv(x, y, r.a);
    r.total = total;
    return PVHIP_OK;
}
#undef POOL_CHECK_ARG

PoolDivs pool_divs(const PoolArgs& a) {
    return PoolDivs{make_fastdiv((unsigned)(a.h * a.w)), make_fastdiv((unsigned)a.w), make_fastdiv((unsigned)(a.oh * a.ow)), make_fastdiv((unsigned)a.ow)};
}
Pool3Divs pool3_divs(const Pool3Args& a) {
    return Pool3Divs{make_fastdiv((unsigned)a.n_bands), make_fastdiv((unsigned)(a.S * a.ow)), make_fastdiv((unsigned)a.ow)};
}

// run-time bools -> template arguments: f(std::bool_constant..., one per bool)
template <class F>
void with_bools(F&& f) { f(); }
template <class F, class... Bs>
void with_bools(F&& f, bool b, Bs... rest) {
    if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else   with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

void clear_form(int* form) {
    for (int i = 0; i < PVHIP_FORM_INTS; ++i) form[i] = 0;
    form[PVHIP_FORM_KIND] = PVHIP_FORM_NONE;
}

}  // namespace

extern "C" {

int pvhip_maxpool2d_f32(const float* x, float* y, int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh,
                        int sw, int pad_top, int pad_left, int pad_bottom, int pad_right) {
    PVHIP_REQUIRE_INIT();
    MaxPoolRequest r;
    int rc = maxpool_request("pvhip_maxpool2d_f32", true, x, y, PoolShape{n, c, h, w, oh, ow, kh, kw, sh, sw}, pad_top, pad_left, pad_bottom, pad_right, r);
    if (rc || r.total == 0) return rc;
    const PoolArgs&    a = r.a;
    const MaxPoolPlan& p = r.p;
    switch (p.kind) {
        case PVHIP_MAXPOOL_COLS_S1:
        case PVHIP_MAXPOOL_COLS_S2: {
            const Pool3Plan& pl3 = p.p3;
            const Pool3Divs  dv3 = pool3_divs(pl3.a);
            with_bools([&](auto S2, auto STAGE, auto NT) {
                hipLaunchKernelGGL((maxpool3x3_cols_kernel<decltype(S2)::value ? 2 : 1, decltype(STAGE)::value, decltype(NT)::value>), dim3(pl3.grid),
                                   dim3(kBlock), pl3.lds, state().stream, pl3.a, dv3);
            }, p.kind == PVHIP_MAXPOOL_COLS_S2, pl3.stage, p.nt);
            break;
        }
        case PVHIP_MAXPOOL_LDS:
        case PVHIP_MAXPOOL_LDS_2X2:
        case PVHIP_MAXPOOL_LDS_3X3: {
            const dim3     grid((a.n_planes + p.G - 1) / p.G, p.n_bands);
            const PoolDivs dv = pool_divs(a);
            with_bools([&](auto K3, auto K2, auto CLIP) {
                constexpr int K = decltype(K3)::value ? 3 : decltype(K2)::value ? 2 : 0;
                hipLaunchKernelGGL((maxpool2d_lds_kernel<K, K, decltype(CLIP)::value>), grid, dim3(kBlock), p.lds, state().stream, x, y, a, p.G, p.band_rows, dv);
            }, p.kind == PVHIP_MAXPOOL_LDS_3X3, p.kind == PVHIP_MAXPOOL_LDS_2X2, p.clip);
            break;
        }
        default:
            hipLaunchKernelGGL(maxpool2d_kernel, dim3(grid_for(r.total)), dim3(kBlock), 0, state().stream, x, y, a, r.total);
    }
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

int pvhip_maxpool2d_form(int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh, int sw, int pad_top, int pad_left,
                         int pad_bottom, int pad_right, int* form) {
    PVHIP_CHECK_ARG(form != nullptr);
    clear_form(form);
    MaxPoolRequest r;
    int rc = maxpool_request("pvhip_maxpool2d_form", false, nullptr, nullptr, PoolShape{n, c, h, w, oh, ow, kh, kw, sh, sw}, pad_top, pad_left, pad_bottom, pad_right, r);
    if (rc || r.total == 0) return rc;
    const MaxPoolPlan& p = r.p;
    const bool cols = p.kind == PVHIP_MAXPOOL_COLS_S1 || p.kind == PVHIP_MAXPOOL_COLS_S2;
    form[PVHIP_FORM_KIND] = p.kind;
    if (p.kind == PVHIP_MAXPOOL_GLOBAL) return PVHIP_OK;
    form[PVHIP_FORM_G] = p.G; form[PVHIP_FORM_BANDS] = p.n_bands; form[PVHIP_FORM_BAND_ROWS] = p.band_rows;
    form[PVHIP_FORM_CLIP] = p.clip ? 1 : 0;
    form[PVHIP_FORM_STAGE] = (cols && p.p3.stage) ? 1 : 0;
    form[PVHIP_FORM_NT] = p.nt ? 1 : 0;
    form[PVHIP_FORM_S] = cols ? p.p3.a.S : 0;
    return PVHIP_OK;
}

int pvhip_avgpool2d_f32(const float* x, float* y, int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh,
                        int sw) {
    PVHIP_REQUIRE_INIT();
    AvgPoolRequest r;
    int rc = avgpool_request("pvhip_avgpool2d_f32", true, x, y, PoolShape{n, c, h, w, oh, ow, kh, kw, sh, sw}, r);
    if (rc || r.total == 0) return rc;
    if (r.p.kind == PVHIP_AVGPOOL_LDS)
        hipLaunchKernelGGL(avgpool2d_lds_kernel, dim3((r.a.n_planes + r.p.G - 1) / r.p.G), dim3(kBlock), r.p.lds, state().stream, x, y, r.a, r.p.G,
                           pool_divs(r.a));
    else
        hipLaunchKernelGGL(avgpool2d_kernel, dim3(grid_for(r.total)), dim3(kBlock), 0, state().stream, x, y, r.a, r.total);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

int pvhip_avgpool2d_form(int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh, int sw, int* form) {
    PVHIP_CHECK_ARG(form != nullptr);
    clear_form(form);
    AvgPoolRequest r;
    int rc = avgpool_request("pvhip_avgpool2d_form", false, nullptr, nullptr, PoolShape{n, c, h, w, oh, ow, kh, kw, sh, sw}, r);
    if (rc || r.total == 0) return rc;
    form[PVHIP_FORM_KIND] = r.p.kind;
    if (r.p.kind == PVHIP_AVGPOOL_GLOBAL) return PVHIP_OK;
    form[PVHIP_FORM_G] = r.p.G; form[PVHIP_FORM_BANDS] = 1; form[PVHIP_FORM_BAND_ROWS] = oh;
    form[PVHIP_FORM_VEC] = all_starts_aligned(h, w, r.p.G, r.a.n_planes, 1, oh, sh, 0);
    return PVHIP_OK;
}

int pvhip_dwconv2d_f32(const float* x, const float* w, float* y, int n, int g, int h, int wdt, int kh, int kw, int oh,
                       int ow, int sh, int sw, int pad_top, int pad_left, const float* bias, int act, float act_lo,
                       float act_hi) {
    PVHIP_REQUIRE_INIT();
    DwRequest r;
    int rc = dwconv_request("pvhip_dwconv2d_f32", true, x, w, y, PoolShape{n, g, h, wdt, oh, ow, kh, kw, sh, sw}, pad_top, pad_left, act, r);
    if (rc || r.total == 0) return rc;
    const PoolArgs& a = r.a;
    const DwPlan&   p = r.p;
    const DwEpilogue ep{bias, act, act_lo, act_hi};
    switch (p.kind) {
        case PVHIP_DWCONV_COLS_S1:
        case PVHIP_DWCONV_COLS_S2: {
            const Pool3Plan& plan = p.p3;
            const Pool3Divs  dv3  = pool3_divs(plan.a);
            with_bools([&](auto S2, auto NT, auto STAGE) {
                hipLaunchKernelGGL((dwconv3x3_cols_kernel<decltype(S2)::value ? 2 : 1, decltype(NT)::value, decltype(STAGE)::value>), dim3(plan.grid),
                                   dim3(kBlock), plan.lds, state().stream, plan.a, dv3, w, g, ep);
            }, p.kind == PVHIP_DWCONV_COLS_S2, p.nt, plan.stage);
            break;
        }
        case PVHIP_DWCONV_LDS:
        case PVHIP_DWCONV_LDS_3X3: {
            const dim3     grid((a.n_planes + p.G - 1) / p.G, p.n_bands);
            const PoolDivs dv = pool_divs(a);
            with_bools([&](auto K3) {
                constexpr int K = decltype(K3)::value ? 3 : 0;
                hipLaunchKernelGGL((dwconv2d_lds_kernel<K, K>), grid, dim3(kBlock), p.lds, state().stream, x, w, y, a, g, p.G, p.band_rows, dv, ep);
            }, p.kind == PVHIP_DWCONV_LDS_3X3);
            break;
        }
        default: {
            DwArgs d{g, h, wdt, oh, ow, kh, kw, sh, sw, pad_top, pad_left};
            hipLaunchKernelGGL(dwconv_kernel, dim3(grid_for((size_t)r.total)), dim3(kBlock), 0, state().stream, x, w, y, d, r.total, ep);
        }
    }
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

int pvhip_dwconv2d_form(int n, int g, int h, int wdt, int kh, int kw, int oh, int ow, int sh, int sw, int pad_top, int pad_left,
                        int* form) {
    PVHIP_CHECK_ARG(form != nullptr);
    clear_form(form);
    DwRequest r;
    int rc = dwconv_request("pvhip_dwconv2d_form", false, nullptr, nullptr, nullptr, PoolShape{n, g, h, wdt, oh, ow, kh, kw, sh, sw}, pad_top, pad_left, 0, r);
    if (rc || r.total == 0) return rc;
    const DwPlan& p = r.p;
    const bool cols = p.kind == PVHIP_DWCONV_COLS_S1 || p.kind == PVHIP_DWCONV_COLS_S2;
    form[PVHIP_FORM_KIND] = p.kind;
    if (p.kind == PVHIP_DWCONV_GLOBAL) return PVHIP_OK;
    form[PVHIP_FORM_G] = p.G; form[PVHIP_FORM_BANDS] = p.n_bands; form[PVHIP_FORM_BAND_ROWS] = p.band_rows;
    // (the column kernel copies from the 16-byte boundary below any start: it has one staging form)
    form[PVHIP_FORM_VEC] = cols ? 1 : all_starts_aligned(h, wdt, p.G, n * g, p.n_bands, p.band_rows, sh, pad_top);
    form[PVHIP_FORM_STAGE] = (cols && p.p3.stage) ? 1 : 0;
    form[PVHIP_FORM_NT] = p.nt ? 1 : 0;
    form[PVHIP_FORM_S] = cols ? p.p3.a.S : 0;
    return PVHIP_OK;
}

}  // extern "C"
