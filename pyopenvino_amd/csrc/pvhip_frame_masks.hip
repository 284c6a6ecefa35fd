// Instance masks in frame pixels: for every box a pvhip_dense_boxes_tail_f32 call has just kept, the logits coefficients @ prototypes
// sampled bilinearly at the centres of the box's frame pixels, straight through the letterbox geometry, thresholded after the
// sampling and packed one bit a pixel -- what Ultralytics' process_mask with upsampling (retina_masks) makes on the host.
// include/pvhip.h states the rule (pvhip_frame_masks_f32); pyopenvino_amd/masks.py (make_frame) and tests/frame_masks_ref.py are the
// same in numpy and in plain loops.
//
// One call, two launches behind pvhip_dense_boxes_tail_f32 on the same stream; both read that call's header and rows on the device.
//   plan      one workgroup of 1024 lanes scans the rows 1024 at a time: a row's word count h * ceil(w / 32) (0 for a rectangle that is
//             not inside the frame) and its count of bands, two block-wide prefix sums with a carry.  It writes the exclusive int64
//             offsets and the band prefix to `scratch`, and (made, used) -- the rows whose words fit max_words, and their words -- to
//             the 8-byte header the host reads.  Rows from `made` on get no bands: nothing is written for them.
//   band      a run of rectangle rows of one detection, the unit of work of the second launch: band_rows() gives its height, the most
//             rows whose window of prototype pixels -- the clamped tap rows times the clamped tap columns of the rectangle -- fits
//             PVHIP_FRAME_MASKS_LDS_FLOATS floats, at most PVHIP_FRAME_MASKS_BAND_ROWS (the row table's room).  Both launches call it.
//   masks     a fixed grid of persistent workgroups walks the bands with a static stride and finds a band's row by binary search in
//             the prefix: the host never knows total, so the grid cannot be sized by it.  Per band:
//     stage      the T coefficients of the anchor; then one lane per window pixel runs the rule's fmaf chain, t ascending from +0,
//                over the T planes -- consecutive lanes read consecutive floats of a plane's row -- and puts the logit into LDS, NaN
//                where one of the pixel's T values is not finite.  This is a matrix-vector product per detection (M = 1): the
//                32 x 32 x 2 matrix instruction would spend 31 of its 32 rows on zeros, and fmaf in t order is the rule's bits
//                already.  The matrix cores are deliberately not used in this file.
//     positions  separable: the 64-bit divisions of the rule run once per band for its rows and, 4096 at a time, its columns, and
//                leave (first tap relative to the window, second tap the same or the next, Q16 fraction) in one LDS word each.
//     sample     PVHIP_FRAME_MASKS_FORM_ROW (w > 32): a wave takes 64 consecutive pixels of one rectangle row; a lane reads four
//                LDS taps, does three lerps (no contraction: -ffp-contract=off and the pragma below) and compares; one wave-wide
//                ballot is two finished words, stored as 8 bytes where both exist.  PVHIP_FRAME_MASKS_FORM_PAIR (w <= 32): a wave
//                takes two rectangle rows, a half each; its ballot is the two rows' words, which stand side by side.
//             Every word of every row below `made` is written exactly once, padding bits 0; nothing else is written.  A detection
//             with a coefficient that is not finite skips the stage and writes zeros.
// No global-memory atomics, no workgroup waits for another, the same words every call.
#include "pvhip_common.h"
#include "pvhip_frame_taps.h"

#pragma clang fp contract(off)

using namespace pvhip;

namespace {

constexpr int kLdsFloats   = PVHIP_FRAME_MASKS_LDS_FLOATS;      // the window of logits
constexpr int kBandRows    = PVHIP_FRAME_MASKS_BAND_ROWS;       // the row table
constexpr int kColChunk    = 4096;                              // the column table: a multiple of 64
constexpr int kGridPerCU   = PVHIP_FRAME_MASKS_GRID_PER_CU;
constexpr int kWaves       = kBlock / kWave;
constexpr int kPlanBlock   = 1024;
constexpr int kMaxTail     = 64;
constexpr int kMaxPlane    = 4096;
constexpr int kMaxExtent   = 16384;
constexpr int kMaxPerImage = 4096;                              // PVHIP_BOXES_MAX_CANDIDATES
constexpr long long kMaxRows  = 1LL << 24;                      // n * max_per_image
constexpr long long kMaxWords = 1LL << 28;

struct FrameArgs {
    const float* head;      // (n, e, a) or (n, a, e)
    const float* protos;    // (n, tail, hp, wp)
    const int*   header;    // counts[n], selected[n], total
    const int*   rows;      // [total][8]: r, x, y, w, h, label, score bits, r * a + anchor
    int*         info;      // scratch: total, bands, 0, 0; then the offsets and the band prefix
    int*         made;      // made, used
    unsigned*    words;
    long long    max_words;
    int n, a, e, planes, tail_at, tail, hp, wp, hn, wn, fh, fw, dx, dy, iw, ih, per_image;
};

__device__ __forceinline__ long long* offsets_of(int* info) { return reinterpret_cast<long long*>(info + 4); }
__device__ __forceinline__ int* prefix_of(int* info, long long room) { return reinterpret_cast<int*>(offsets_of(info) + room + 1); }

__device__ __forceinline__ bool not_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u; }

// (Axis, Tap, tap_of and packed -- rule 2 -- are pvhip_frame_taps.h's, shared with pvhip_segments_frame.hip.)

// The height of a detection's bands: the most frame rows whose tap rows times `cw` tap columns fit the LDS window.  k frame rows
// further on the first tap is at most ceil(k * ih * hp / (fh * hn)) rows further on, and a band's taps are the first row's first
// and the last row's second: at most ceil((rows - 1) * num / den) + 2 prototype rows.  One frame row always fits: 2 cw <= the room.
__device__ __forceinline__ int band_rows(int h, int cw, const Axis& ay) {
    const long long room = kLdsFloats / cw - 2;
    const long long rows = 1 + room * (ay.den / 2) / (ay.step / 2);
    return (int)min(rows, (long long)min(h, kBandRows));
}

struct Rect {
    int r, x, y, w, h, wr;                      // wr: words per rectangle row, 0 for a rectangle that owns none
};
__device__ __forceinline__ Rect rect_of(const FrameArgs& k, long long j) {
    const int4 v = *reinterpret_cast<const int4*>(k.rows + 8 * j);
    const int h = k.rows[8 * j + 4];
    const bool inside = v.y >= 0 && v.w >= 1 && (long long)v.y + v.w <= k.fw && v.z >= 0 && h >= 1 && (long long)v.z + h <= k.fh;
    return Rect{min(max(v.x, 0), k.n - 1), v.y, v.z, v.w, h, inside ? (v.w + 31) >> 5 : 0};
}
// The rectangle's clamped tap columns [first, first + cw) and the height of its bands.
__device__ __forceinline__ int bands_of(const FrameArgs& k, const Rect& c, const Axis& ax, const Axis& ay, int* first, int* cw) {
    const Tap lo = tap_of(ax, c.x), hi = tap_of(ax, c.x + c.w - 1);
    *first = lo.a;
    *cw = hi.b - lo.a + 1;
    return band_rows(c.h, *cw, ay);
}

// Inclusive prefix sum over the workgroup's 1024 lanes; `part` holds a value per wave.  Two barriers.
__device__ __forceinline__ long long block_scan(long long v, long long* part, long long* sum) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const long long o = __shfl_up(v, d, kWave);
        if (lane >= d) v += o;
    }
    __syncthreads();                            // the scan before is read
    if (lane == kWave - 1) part[wave] = v;
    __syncthreads();
    long long before = 0, all = 0;
    for (int i = 0; i < kPlanBlock / kWave; ++i) {
        const long long p = part[i];
        before += i < wave ? p : 0;
        all += p;
    }
    *sum = all;
    return v + before;
}

__global__ __launch_bounds__(kPlanBlock) void frame_plan_kernel(FrameArgs k) {
    __shared__ long long part[kPlanBlock / kWave];
    const int tid = threadIdx.x;
    const long long room = (long long)k.n * k.per_image;
    long long*  offsets = offsets_of(k.info);
    int*        prefix  = prefix_of(k.info, room);
    const Axis ax = axis_of(k.dx, k.iw, k.fw, k.wp, k.wn), ay = axis_of(k.dy, k.ih, k.fh, k.hp, k.hn);

    long long mine = 0, total = 0;              // the rows: the counts clamped to what the rows hold
    for (int i = tid; i < k.n; i += kPlanBlock) mine += min(max(k.header[i], 0), k.per_image);
    block_scan(mine, part, &total);

    long long carry_w = 0, carry_b = 0, made = 0, used = 0;
    for (long long base = 0; base < total; base += kPlanBlock) {           // (the same trips in every lane)
        const long long j = base + tid;
        long long w = 0, b = 0, sum_w, sum_b;
        if (j < total) {
            const Rect c = rect_of(k, j);
            if (c.wr) {
                int first, cw;
                const int rows = bands_of(k, c, ax, ay, &first, &cw);
                w = (long long)c.h * c.wr;
                b = (c.h + rows - 1) / rows;
            }
        }
        const long long end = carry_w + block_scan(w, part, &sum_w);       // offsets[j + 1]
        const bool has = j < total && end <= k.max_words;
        if (!has) b = 0;
        const long long bend = carry_b + block_scan(b, part, &sum_b);
        if (j < total) {
            offsets[j] = end - w;
            prefix[j]  = (int)(bend - b);
        }
        made += has ? 1 : 0;
        used = has ? end : used;                // (a lane's rows ascend, and so do the offsets)
        carry_w += sum_w;
        carry_b += sum_b;
    }
    long long all_made, all_used;
    block_scan(made, part, &all_made);
    // the largest `used` of any lane: the offsets ascend, so it is offsets[made]
    long long m = used;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, __shfl_xor(m, d, kWave));
    __syncthreads();
    if ((tid & (kWave - 1)) == 0) part[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        all_used = 0;
        for (int i = 0; i < kPlanBlock / kWave; ++i) all_used = max(all_used, part[i]);
        offsets[total] = carry_w;
        prefix[total]  = (int)carry_b;
        k.info[0] = (int)total;
        k.info[1] = (int)carry_b;
        k.info[2] = 0;
        k.info[3] = 0;
        k.made[0] = (int)all_made;
        k.made[1] = (int)all_used;
    }
}

struct __attribute__((packed, aligned(4))) WordPair {
    unsigned lo, hi;
};

__global__ __launch_bounds__(kBlock) void frame_masks_kernel(FrameArgs k) {
    __shared__ float    win[kLdsFloats];
    __shared__ unsigned colpos[kColChunk];
    __shared__ unsigned rowpos[kBandRows];
    __shared__ float    coef[kMaxTail];
    __shared__ int      bad;

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long room = (long long)k.n * k.per_image;
    const long long* offsets = offsets_of(k.info);
    const int*       prefix  = prefix_of(k.info, room);
    const int total = k.info[0], bands = k.info[1];
    const Axis ax = axis_of(k.dx, k.iw, k.fw, k.wp, k.wn), ay = axis_of(k.dy, k.ih, k.fh, k.hp, k.hn);
    const int T = k.tail, hw = k.hp * k.wp;

    for (int b = blockIdx.x; b < bands; b += gridDim.x) {                  // (the same trips in every lane of the workgroup)
        int lo = 0, hi = total;                 // the last row whose prefix is at most b: prefix[total] = bands > b
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (prefix[mid] <= b) lo = mid; else hi = mid;
        }
        const Rect c = rect_of(k, lo);
        if (!c.wr) continue;                    // (never: such a row has no band)
        int wc0, cw;
        const int per  = bands_of(k, c, ax, ay, &wc0, &cw);
        const int y0   = (b - prefix[lo]) * per;
        const int rows = min(per, c.h - y0);
        if (rows < 1) continue;                 // (never)
        const Tap rf = tap_of(ay, c.y + y0), rl = tap_of(ay, c.y + y0 + rows - 1);
        const int wr0 = rf.a, count = min((rl.b - wr0 + 1) * cw, kLdsFloats);

        __syncthreads();                        // the band before is done with
        if (tid < kWave) {
            float v = 0.0f;
            if (tid < T) {
                const int anchor = min(max(k.rows[8 * (size_t)lo + 7] - c.r * k.a, 0), k.a - 1), ch = k.tail_at + tid;
                v = k.planes ? k.head[((size_t)c.r * k.e + ch) * (size_t)k.a + anchor] : k.head[((size_t)c.r * k.a + anchor) * (size_t)k.e + ch];
            }
            coef[tid] = v;
            const unsigned long long nf = __ballot(not_finite(v));
            if (tid == 0) bad = nf != 0ull;
        }
        for (int i = tid; i < rows; i += kBlock) rowpos[i] = packed(tap_of(ay, c.y + y0 + i), wr0);
        __syncthreads();
        const bool empty = bad != 0;

        // ---- the window's logits
        if (!empty) {
            const float* planes = k.protos + (size_t)c.r * T * (size_t)hw;
            for (int idx = tid; idx < count; idx += kBlock) {
                const int wy = idx / cw, wx = idx - wy * cw;
                const float* p = planes + (size_t)(wr0 + wy) * k.wp + wc0 + wx;
                float acc = 0.0f;
                bool  nf  = false;
#pragma unroll 8
                for (int t = 0; t < T; ++t) {
                    const float v = p[(size_t)t * hw];
                    nf |= not_finite(v);
                    acc = __builtin_fmaf(coef[t], v, acc);
                }
                win[idx] = nf ? __builtin_nanf("") : acc;
            }
        }

        unsigned* out = k.words + offsets[lo] + (long long)y0 * c.wr;
        for (int c0 = 0; c0 < c.w; c0 += kColChunk) {
            const int cn = min(kColChunk, c.w - c0);
            __syncthreads();                    // the window is whole; the chunk before is done with
            for (int i = tid; i < cn; i += kBlock) colpos[i] = packed(tap_of(ax, c.x + c0 + i), wc0);
            __syncthreads();
            const bool pair  = c.w <= 32;       // PVHIP_FRAME_MASKS_FORM_PAIR
            const int  segs  = (cn + kWave - 1) / kWave;
            const int  units = pair ? (rows + 1) >> 1 : rows * segs;
            for (int u = wave; u < units; u += kWaves) {
                const int ry  = pair ? 2 * u + (lane >> 5) : u / segs;
                const int sg  = pair ? 0 : u - ry * segs;
                const int col = pair ? (lane & 31) : sg * kWave + lane;
                bool on = false;
                if (!empty && col < cn && ry < rows) {
                    const unsigned cp = colpos[col], rp = rowpos[ry];
                    const int   xa = cp & 0x7FFF, xs = (cp >> 15) & 1, ya = rp & 0x7FFF, ys = (rp >> 15) & 1;
                    const float fx = (float)(cp >> 16) * (1.0f / 65536.0f), fy = (float)(rp >> 16) * (1.0f / 65536.0f);
                    const float* top = win + ya * cw + xa;
                    const float* bot = top + ys * cw;
                    const float t0 = top[0] + fx * (top[xs] - top[0]);
                    const float t1 = bot[0] + fx * (bot[xs] - bot[0]);
                    on = t0 + fy * (t1 - t0) > 0.0f;
                }
                const unsigned long long m = __ballot(on);
                if (lane == 0) {
                    unsigned* at = pair ? out + 2 * u : out + (size_t)ry * c.wr + (c0 >> 5) + 2 * sg;
                    const bool both = pair ? 2 * u + 1 < rows : (c0 >> 5) + 2 * sg + 1 < c.wr;
                    if (both) *reinterpret_cast<WordPair*>(at) = WordPair{(unsigned)m, (unsigned)(m >> 32)};
                    else *at = (unsigned)m;
                }
            }
        }
    }
}

}  // namespace

extern "C" {

int pvhip_frame_masks_form(int w) {
    if (w < 1 || w > kMaxExtent) return PVHIP_FRAME_MASKS_FORM_NONE;
    return w <= 32 ? PVHIP_FRAME_MASKS_FORM_PAIR : PVHIP_FRAME_MASKS_FORM_ROW;
}

int pvhip_frame_masks_f32(const float* head, int n, int a, int e, int layout, int tail_at, int tail,
                          const float* protos, int hp, int wp, int hn, int wn,
                          int frame_h, int frame_w, int dx, int dy, int iw, int ih,
                          int max_per_image, long long max_words, int workgroups,
                          const int* header, const int* rows, void* scratch, int* made, unsigned* words) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(head != nullptr && protos != nullptr && header != nullptr && rows != nullptr && scratch != nullptr && made != nullptr && words != nullptr);
    PVHIP_CHECK_ARG(((uintptr_t)head & 3u) == 0 && ((uintptr_t)protos & 3u) == 0 && ((uintptr_t)header & 3u) == 0 && ((uintptr_t)words & 3u) == 0);
    PVHIP_CHECK_ARG(((uintptr_t)rows & 15u) == 0 && ((uintptr_t)scratch & 15u) == 0 && ((uintptr_t)made & 7u) == 0);
    PVHIP_CHECK_ARG(n >= 1 && n <= 65535 && a >= 1 && e >= 1 && (long long)n * a * e < (1LL << 31));
    PVHIP_CHECK_ARG(layout == PVHIP_BOXES_LAYOUT_NCA || layout == PVHIP_BOXES_LAYOUT_NAC);
    PVHIP_CHECK_ARG(tail >= 1 && tail <= kMaxTail && tail_at >= 4 && (long long)tail_at + tail <= e);
    PVHIP_CHECK_ARG(hp >= 1 && hp <= kMaxPlane && wp >= 1 && wp <= kMaxPlane && (long long)hp * wp >= 2 && 2 * wp <= kLdsFloats);
    PVHIP_CHECK_ARG(hn >= 1 && hn <= kMaxExtent && wn >= 1 && wn <= kMaxExtent);
    PVHIP_CHECK_ARG(frame_h >= 1 && frame_h <= kMaxExtent && frame_w >= 1 && frame_w <= kMaxExtent);
    PVHIP_CHECK_ARG(dx >= 0 && dx <= kMaxExtent && dy >= 0 && dy <= kMaxExtent && iw >= 1 && iw <= kMaxExtent && ih >= 1 && ih <= kMaxExtent);
    PVHIP_CHECK_ARG(max_per_image >= 1 && max_per_image <= kMaxPerImage && (long long)n * max_per_image <= kMaxRows);
    PVHIP_CHECK_ARG(max_words >= 1 && max_words <= kMaxWords);
    PVHIP_CHECK_ARG(workgroups >= 0 && workgroups <= 65535);            // (the last refusal: nothing is done before it)

    const FrameArgs k{head, protos, header, rows, static_cast<int*>(scratch), made, words, max_words, n, a, e,
                      layout == PVHIP_BOXES_LAYOUT_NCA ? 1 : 0, tail_at, tail, hp, wp, hn, wn, frame_h, frame_w, dx, dy, iw, ih, max_per_image};
    hipLaunchKernelGGL(frame_plan_kernel, dim3(1), dim3(kPlanBlock), 0, state().stream, k);
    PVHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(frame_masks_kernel, dim3((unsigned)(workgroups ? workgroups : kNumCU * kGridPerCU)), dim3(kBlock), 0, state().stream, k);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
