// The class map of a segmentation network's Result (n, C, H, W) in frame pixels: the planes sampled bilinearly at the centres of the
// frame's pixels, straight through the letterbox geometry, and the best class taken after the sampling -- what users of DeepLab-style
// heads make on the host with F.interpolate(logits, size, mode='bilinear', align_corners=False).argmax(1) after reading the whole
// tensor back.  include/pvhip.h states the rule (pvhip_segment_frame_labels_f32); pyopenvino_amd/segments.py (frame_labels) and
// tests/segments_frame_ref.py are the same in numpy and in plain loops.
//
// One call, two launches: the initialisation of areas and extents, and the sampling.
//   tiles      a workgroup owns a tile of one batch row: a band of `per` <= kBandRows frame rows times a chunk of kColChunk frame
//              columns.  A bounded grid of persistent workgroups walks the tiles, which stand batch row by batch row, with a static stride.
//   positions  separable: the 64-bit divisions of the rule (pvhip_frame_taps.h) run once per tile for its rows and once for its columns
//              and leave (first tap relative to the window, second tap the same or the next, Q16 fraction) in one LDS word each.
//   quads      the labels (n, Fh, Fw) are one flat run of bytes, cut at its own 4-byte boundaries into quads.  Within a tile's row a
//              lane owns one quad, a wave one row at a time and kBandRows / 4 rows in all: kColChunk = 4 * 64 - 4 columns are at most 64
//              quads at any phase.  A whole quad is one aligned 32-bit store, the ragged ends of a chunk's row are stored by the byte;
//              Fw % 4 != 0 puts every row at another phase.  Every byte is written exactly once.
//   staged     (PVHIP_SEGMENT_FRAME_FORM_STAGED) the tile's window of map pixels, its clamped tap rows times its clamped tap columns, is
//              staged into LDS for `cc` classes at a time -- consecutive lanes on consecutive floats of a plane's row --, and a lane takes
//              its pixels through all chunks with their running best in registers: the 32-bit order word of pvhip_segments.hip and the
//              class.  Classes ascend through the chunks and only a strictly larger word replaces, so a tie or a NaN across the seam of
//              two chunks still resolves to the lower class.  Per class and pixel: four LDS taps, three lerps (no contraction: the pragma
//              below and -ffp-contract=off), one comparison; a pixel whose column word equals its left neighbour's -- most, when
//              upsampling -- takes that pixel's taps and reads nothing.
//   direct     (PVHIP_SEGMENT_FRAME_FORM_DIRECT) steep downsampling: the window would hold map pixels no tap reads, so the taps come
//              straight from global memory.  Tables, order, stores and sums are the same code.
//   sums       as pvhip_segment_labels_f32: per (wave, class) -- the wave takes the class of its first lane that still has a pixel, the
//              lanes add theirs up, five wave reductions --, one lane adds them by integer LDS atomics to the workgroup's table of one
//              batch row, and the table leaves by vector atomics when the workgroup's batch row changes or its walk ends.  Integers: the
//              same bits every call.
// The matrix cores are deliberately not used: bilinear resampling as two small matrix products would change the order and the number of
// roundings, and the rule's value is its bits.
#include "pvhip_common.h"
#include "pvhip_frame_taps.h"
#include "pvhip_topk_keys.h"

#pragma clang fp contract(off)

using namespace pvhip;

namespace {

constexpr int kLdsFloats   = PVHIP_SEGMENT_FRAME_LDS_FLOATS;
constexpr int kBandRows    = PVHIP_SEGMENT_FRAME_BAND_ROWS;
constexpr int kColChunk    = PVHIP_SEGMENT_FRAME_COL_CHUNK;
constexpr int kClassChunk  = PVHIP_SEGMENT_FRAME_CLASS_CHUNK;
constexpr int kGridPerCU   = PVHIP_SEGMENT_FRAME_GRID_PER_CU;
constexpr int kMinTiles    = PVHIP_SEGMENT_FRAME_MIN_TILES;
constexpr int kDirectStep  = PVHIP_SEGMENT_FRAME_DIRECT_STEP;
constexpr int kWaves       = kBlock / kWave;
constexpr int kRowsPerWave = kBandRows / kWaves;
constexpr int kQuad        = 4;
constexpr int kMaxPlane    = 4096;
constexpr int kMaxExtent   = 16384;
constexpr unsigned kNaNOrder = 0xFFFFFFFFu;
constexpr int kVoid        = PVHIP_SEGMENT_VOID;
static_assert(kBandRows % kWaves == 0 && kColChunk % kQuad == 0 && kColChunk + kQuad <= kQuad * kWave, "a row of a chunk is at most one quad a lane");
static_assert((kDirectStep * (kColChunk - 1) + 2) * 2 <= kLdsFloats, "one frame row of a staged chunk always fits the window");

struct FrameArgs {
    const float*   x;
    unsigned char* labels;
    int*           areas;
    int*           extents;
    long long      tiles;           // n * bands * chunks
    int n, c, h, w, hn, wn, fh, fw, dx, dy, iw, ih;
    int has_min;
    unsigned min_order;             // order_of(min_score)
    int per, bands, chunks, cc;     // rows a band, bands and column chunks a frame, classes a staged chunk
    int phase;                      // labels & 3
};

struct Plan {
    int form, per, bands, chunks, cc;
};

inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// What a launch over these extents does, PVHIP_SEGMENT_FRAME_FORM_NONE for what the entry refuses.  k frame positions further on the
// first tap is at most ceil(k * step / den) map positions further on (pvhip_frame_masks.hip, band_rows): a chunk's window is at most
// `cw` columns, and `per` is the most rows whose window of one class fits kLdsFloats beside them.
Plan plan_of(int c, int h, int w, int hn, int wn, int fh, int fw, int dx, int dy, int iw, int ih) {
    Plan p{PVHIP_SEGMENT_FRAME_FORM_NONE, 0, 0, 0, 0};
    if (c < 1 || c > PVHIP_SEGMENT_MAX_CLASSES || h < 1 || h > kMaxPlane || w < 1 || w > kMaxPlane || (long long)h * w < 2) return p;
    if (hn < 1 || hn > kMaxExtent || wn < 1 || wn > kMaxExtent || fh < 1 || fh > kMaxExtent || fw < 1 || fw > kMaxExtent) return p;
    if (dx < 0 || dx > kMaxExtent || dy < 0 || dy > kMaxExtent || iw < 1 || iw > kMaxExtent || ih < 1 || ih > kMaxExtent) return p;
    const Axis ax = axis_of(dx, iw, fw, w, wn), ay = axis_of(dy, ih, fh, h, hn);
    const bool direct = ax.step > kDirectStep * ax.den || ay.step > kDirectStep * ay.den;
    p.form   = direct ? PVHIP_SEGMENT_FRAME_FORM_DIRECT : PVHIP_SEGMENT_FRAME_FORM_STAGED;
    p.chunks = (int)ceil_div(fw, kColChunk);
    p.per    = fh < kBandRows ? fh : kBandRows;
    p.cc     = c;
    if (!direct) {
        const long long cn = fw < kColChunk ? fw : kColChunk;
        long long cw = ceil_div((cn - 1) * ax.step, ax.den) + 2;
        if (cw > w) cw = w;
        const long long room = kLdsFloats / cw - 2;                  // >= 0: the static_assert above
        const long long rows = 1 + room * (ay.den / 2) / (ay.step / 2);
        if (rows < p.per) p.per = (int)rows;
        long long wr = ceil_div((p.per - 1) * ay.step, ay.den) + 2;
        if (wr > h) wr = h;
        const long long fit = kLdsFloats / (wr * cw);                // >= 1
        p.cc = (int)(fit < kClassChunk ? fit : kClassChunk);
        if (p.cc > c) p.cc = c;
    }
    p.bands = (int)ceil_div(fh, p.per);
    return p;
}

__device__ __forceinline__ unsigned order_of(float v) { return (unsigned)(topk_key(__float_as_uint(v), 0u) >> 32); }

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, kWave));
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, kWave));
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

__global__ __launch_bounds__(kBlock) void segment_frame_init_kernel(int* __restrict__ areas, int* __restrict__ extents, long long cells, int fh, int fw) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < cells; i += (long long)gridDim.x * kBlock) {
        areas[i] = 0;
        extents[4 * i + 0] = fw;
        extents[4 * i + 1] = fh;
        extents[4 * i + 2] = 0;
        extents[4 * i + 3] = 0;
    }
}

template <bool kStaged>
__global__ __launch_bounds__(kBlock) void segment_frame_kernel(FrameArgs k) {
    __shared__ float    win[kStaged ? kLdsFloats : 1];
    __shared__ unsigned colpos[kColChunk];
    __shared__ unsigned rowpos[kBandRows];
    __shared__ int      sums[PVHIP_SEGMENT_MAX_CLASSES * 5];            // per class: area, x0, y0, x1, y1 of row `held`

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Axis ax = axis_of(k.dx, k.iw, k.fw, k.w, k.wn), ay = axis_of(k.dy, k.ih, k.fh, k.h, k.hn);
    const size_t plane = (size_t)k.h * k.w;
    // (every thread of the workgroup: `r` is the same in all of them)  The sums of row r leave for the global block; the table is empty again.
    auto flush = [&](int r) {
        __syncthreads();
        for (int c = tid; c < k.c; c += kBlock) {
            int* cell = sums + 5 * c;
            if (r >= 0 && cell[0] > 0) {
                const size_t to = (size_t)r * k.c + c;
                atomicAdd(k.areas + to, cell[0]);
                atomicMin(k.extents + 4 * to + 0, cell[1]);
                atomicMin(k.extents + 4 * to + 1, cell[2]);
                atomicMax(k.extents + 4 * to + 2, cell[3]);
                atomicMax(k.extents + 4 * to + 3, cell[4]);
            }
            cell[0] = 0; cell[1] = k.fw; cell[2] = k.fh; cell[3] = 0; cell[4] = 0;
        }
        __syncthreads();
    };
    int held = -1;
    const int per_row = k.bands * k.chunks;
    for (long long t = blockIdx.x; t < k.tiles; t += gridDim.x) {          // (the same trips in every lane of the workgroup)
        const int r   = (int)(t / per_row), rem = (int)(t - (long long)r * per_row);
        const int b   = rem / k.chunks, ch = rem - b * k.chunks;
        const int y0  = b * k.per, rows = min(k.per, k.fh - y0);
        const int c0  = ch * kColChunk, cn = min(kColChunk, k.fw - c0);
        if (r != held) {                        // (either way a barrier: the tile before is done with)
            flush(held);
            held = r;
        } else {
            __syncthreads();
        }
        // ---- the window and the positions
        int wr0 = 0, wc0 = 0, rs = k.w, wsize = 0;
        if (kStaged) {
            const Tap rf = tap_of(ay, y0), rl = tap_of(ay, y0 + rows - 1), cf = tap_of(ax, c0), cl = tap_of(ax, c0 + cn - 1);
            wr0 = rf.a;
            wc0 = cf.a;
            rs  = cl.b - cf.a + 1;
            wsize = (rl.b - rf.a + 1) * rs;
            if ((long long)wsize * k.cc > kLdsFloats) continue;         // (never: plan_of's bound)
        }
        for (int i = tid; i < rows; i += kBlock) rowpos[i] = packed(tap_of(ay, y0 + i), wr0);
        for (int i = tid; i < cn; i += kBlock) colpos[i] = packed(tap_of(ax, c0 + i), wc0);

        const float* img = k.x + (size_t)r * k.c * plane;
        unsigned ord[kRowsPerWave][kQuad];
        int      cls[kRowsPerWave][kQuad];
#pragma unroll
        for (int i = 0; i < kRowsPerWave; ++i)
#pragma unroll
            for (int p = 0; p < kQuad; ++p) { ord[i][p] = 0u; cls[i][p] = 0; }        // (no order word is 0: class 0 is taken first)

        const int step = kStaged ? k.cc : k.c;
        for (int cbase = 0; cbase < k.c; cbase += step) {                // (direct: one trip)
            const int cnt = min(step, k.c - cbase);
            if (kStaged) {
                __syncthreads();                // the chunk before is done with
                const int count = cnt * wsize;
                for (int idx = tid; idx < count; idx += kBlock) {
                    const int cl = idx / wsize, at = idx - cl * wsize, wy = at / rs, wx = at - wy * rs;
                    win[idx] = img[((size_t)(cbase + cl) * k.h + wr0 + wy) * (size_t)k.w + wc0 + wx];
                }
            }
            __syncthreads();                    // the window and the tables are whole
            const float* src = kStaged ? win : img + (size_t)cbase * plane;
            const size_t cs  = kStaged ? (size_t)wsize : plane;
#pragma unroll
            for (int i = 0; i < kRowsPerWave; ++i) {
                const int j = wave + kWaves * i;
                if (j < rows) {                 // (wave-uniform)
                    const long long flat = ((long long)r * k.fh + y0 + j) * k.fw;
                    const int xs = c0 - (int)((k.phase + flat + c0) & 3) + kQuad * lane - c0;      // the quad's first column in the chunk
                    unsigned cp[kQuad];
                    float    fx[kQuad];
#pragma unroll
                    for (int p = 0; p < kQuad; ++p) {                   // (a pixel outside the chunk samples an edge column and is dropped)
                        cp[p] = colpos[min(max(xs + p, 0), cn - 1)];
                        fx[p] = (float)(cp[p] >> 16) * (1.0f / 65536.0f);
                    }
                    const unsigned rp = rowpos[j];
                    const float fy = (float)(rp >> 16) * (1.0f / 65536.0f);
                    const float* top = src + (size_t)(rp & 0x7FFF) * rs;
                    const float* bot = top + (size_t)((rp >> 15) & 1) * rs;
                    for (int cl = 0; cl < cnt; ++cl) {
                        float a0 = 0.0f, a1 = 0.0f, b0 = 0.0f, b1 = 0.0f;
#pragma unroll
                        for (int p = 0; p < kQuad; ++p) {
                            if (p == 0 || (cp[p] & 0xFFFFu) != (cp[p - 1] & 0xFFFFu)) {      // other taps than the pixel to the left
                                const int xa = cp[p] & 0x7FFF, xb = xa + ((cp[p] >> 15) & 1);
                                a0 = top[xa]; a1 = top[xb]; b0 = bot[xa]; b1 = bot[xb];
                            }
                            const float t0 = a0 + fx[p] * (a1 - a0);
                            const float t1 = b0 + fx[p] * (b1 - b0);
                            const unsigned o = order_of(t0 + fy * (t1 - t0));
                            if (o > ord[i][p]) { ord[i][p] = o; cls[i][p] = cbase + cl; }
                        }
                        top += cs;
                        bot += cs;
                    }
                }
            }
        }

        // ---- labels
        unsigned lab[kRowsPerWave], pend = 0u;  // a row's four labels as stored; bit 4 i + p: pixel p of row i awaits its sums
        int      px0[kRowsPerWave];
#pragma unroll
        for (int i = 0; i < kRowsPerWave; ++i) {
            const int j = wave + kWaves * i;
            lab[i] = 0u;
            px0[i] = 0;
            if (j < rows) {
                const long long flat = ((long long)r * k.fh + y0 + j) * k.fw;
                const int xs = c0 - (int)((k.phase + flat + c0) & 3) + kQuad * lane;
                px0[i] = xs;
                unsigned live = 0u;
#pragma unroll
                for (int p = 0; p < kQuad; ++p) {
                    const int label = (ord[i][p] == kNaNOrder || (k.has_min && ord[i][p] < k.min_order)) ? kVoid : cls[i][p];
                    lab[i] |= (unsigned)label << (8 * p);
                    if (xs + p >= c0 && xs + p < c0 + cn) {
                        live |= 1u << p;
                        if (label != kVoid) pend |= 1u << (kQuad * i + p);
                    }
                }
                unsigned char* at = k.labels + flat + xs;
                if (live == 0xFu) {
                    *reinterpret_cast<unsigned*>(at) = lab[i];
                } else {
#pragma unroll
                    for (int p = 0; p < kQuad; ++p)
                        if (live & (1u << p)) at[p] = (unsigned char)(lab[i] >> (8 * p));
                }
            }
        }

        // ---- areas and extents: per (wave, class); every pixel of the tile is of row `held`
        for (;;) {                              // (the whole wave: every condition below is wave-uniform)
            const unsigned long long pending = __ballot(pend != 0u);
            if (pending == 0ull) break;
            const int first = __ffsll((long long)pending) - 1;
            int mine = 0;
            {
                const int q = pend ? __ffs((int)pend) - 1 : 0;
                unsigned word = lab[0];
#pragma unroll
                for (int i = 1; i < kRowsPerWave; ++i)
                    if ((q >> 2) == i) word = lab[i];
                mine = (int)((word >> (8 * (q & 3))) & 0xFFu);
            }
            const int c = __shfl(mine, first, kWave);
            int count = 0, x0 = k.fw, x1 = 0, ya = k.fh, yb = 0;
#pragma unroll
            for (int i = 0; i < kRowsPerWave; ++i)
#pragma unroll
                for (int p = 0; p < kQuad; ++p) {
                    const unsigned bit = 1u << (kQuad * i + p);
                    if ((pend & bit) && (int)((lab[i] >> (8 * p)) & 0xFFu) == c) {
                        const int y = y0 + wave + kWaves * i;
                        ++count;
                        x0 = min(x0, px0[i] + p);
                        x1 = max(x1, px0[i] + p + 1);
                        ya = min(ya, y);
                        yb = max(yb, y + 1);
                        pend &= ~bit;
                    }
                }
            const int sum = wave_sum_i32(count);
            const int wx0 = wave_min_i32(x0), wx1 = wave_max_i32(x1), wy0 = wave_min_i32(ya), wy1 = wave_max_i32(yb);
            if (lane == first) {                // (LDS atomics: the four waves of the workgroup share the table)
                int* cell = sums + 5 * c;
                atomicAdd(cell + 0, sum);
                atomicMin(cell + 1, wx0);
                atomicMin(cell + 2, wy0);
                atomicMax(cell + 3, wx1);
                atomicMax(cell + 4, wy1);
            }
        }
    }
    flush(held);
}

}  // namespace

extern "C" {

int pvhip_segment_frame_labels_form(int c, int h, int w, int hn, int wn, int fh, int fw, int dx, int dy, int iw, int ih) {
    return plan_of(c, h, w, hn, wn, fh, fw, dx, dy, iw, ih).form;
}

int pvhip_segment_frame_labels_f32(const float* x, int n, int c, int h, int w, int hn, int wn, int fh, int fw, int dx, int dy, int iw, int ih,
                                   int has_min, float min_score, unsigned char* labels, int* areas, int* extents) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(x != nullptr && labels != nullptr && areas != nullptr && extents != nullptr);
    PVHIP_CHECK_ARG(((uintptr_t)x & 3u) == 0 && ((uintptr_t)areas & 3u) == 0 && ((uintptr_t)extents & 3u) == 0);
    PVHIP_CHECK_ARG(n >= 1);
    const Plan plan = plan_of(c, h, w, hn, wn, fh, fw, dx, dy, iw, ih);
    PVHIP_CHECK_ARG(plan.form != PVHIP_SEGMENT_FRAME_FORM_NONE);               // the ranges of c, h, w and of the geometry
    PVHIP_CHECK_ARG((long long)n * fh * fw < (1LL << 31));
    PVHIP_CHECK_ARG(has_min == 0 || has_min == 1);
    PVHIP_CHECK_ARG(min_score - min_score == 0.0f);                              // finite
    unsigned min_bits;
    __builtin_memcpy(&min_bits, &min_score, sizeof min_bits);
    const unsigned mag = min_bits & 0x7FFFFFFFu;                                 // the order word of pvhip_topk_keys.h, of a finite value
    const unsigned min_order = mag == 0u ? 0x80000000u : ((min_bits & 0x80000000u) ? ~min_bits : (min_bits | 0x80000000u));
    const long long tiles = (long long)n * plan.bands * plan.chunks;
    const FrameArgs k{x, labels, areas, extents, tiles, n, c, h, w, hn, wn, fh, fw, dx, dy, iw, ih, has_min, min_order,
                      plan.per, plan.bands, plan.chunks, plan.cc, (int)((uintptr_t)labels & 3u)};
    const long long cells = (long long)n * c;
    hipLaunchKernelGGL(segment_frame_init_kernel, dim3((unsigned)grid_for((size_t)cells)), dim3(kBlock), 0, state().stream, areas, extents, cells, fh, fw);
    PVHIP_LAUNCH_CHECK();
    long long grid = tiles <= kMinTiles ? 1 : tiles;                             // (a launch that small is latency either way)
    if (grid > (long long)kNumCU * kGridPerCU) grid = (long long)kNumCU * kGridPerCU;
    if (plan.form == PVHIP_SEGMENT_FRAME_FORM_STAGED)
        hipLaunchKernelGGL(segment_frame_kernel<true>, dim3((unsigned)grid), dim3(kBlock), 0, state().stream, k);
    else
        hipLaunchKernelGGL(segment_frame_kernel<false>, dim3((unsigned)grid), dim3(kBlock), 0, state().stream, k);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
