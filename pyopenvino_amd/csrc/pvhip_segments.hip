// The class map of a segmentation network's Result (n, C, H, W), on the device: what users of DeepLab-style and road-segmentation heads do
// on the host with np.argmax(axis=1) after reading the whole tensor back, and the pixel count and bounding rectangle of every class with
// it.  include/pvhip.h states the rule (pvhip_segment_labels_f32), pyopenvino_amd/segments.py and tests/segments_ref.py are the same in
// numpy and in plain loops.
//
// A streaming reduction across planes: every score is read once, one byte per pixel is written.
//   quads   the labels (n, H, W) are one flat run of n * H * W bytes.  It is cut at the 4-byte boundaries of its own addresses into
//           quads: a lane owns one quad, four consecutive pixels, and a workgroup kTripPixels = 1024 of them per trip.  A whole quad is
//           one aligned 32-bit store; the quads at the two ends of the run may be partial and are stored by the byte.
//   loads   a quad whose four pixels lie in one batch row reads 16 bytes per class, at whatever 4-byte phase x, the class and the row put
//           it: global loads of 16 bytes need 4-byte alignment only, so one form serves every phase (the type F4 says so to the compiler).
//           A quad across the seam of two rows, or a partial one, reads its pixels one by one: one lane in H * W / 4 where H * W % 4 != 0.
//           Classes are walked four at a time, the four loads issued before the first comparison.
//   order   one 32-bit word per pixel, the high word of pvhip_topk_keys.h's key: walking the classes upward and taking a strictly larger
//           word gives the first NaN, +0.0 == -0.0 and the lower class of a tie.  min_score is compared as such a word.
//   sums    areas and extents are accumulated per (wave, batch row, class): the wave takes the (row, class) of its first lane that still
//           has a pixel, the lanes holding pixels of it add them up -- counts by ballots, x by two wave reductions, y from the first and
//           the last of those lanes, for the flat order is the order of y --, and one lane adds them by five integer LDS atomics to the
//           workgroup's table of one batch row (255 classes x 5 words).  A wave of a real class map holds one to three classes.  A
//           workgroup takes consecutive trips, so the row it holds changes seldom; when it does, and at the end, the table leaves by
//           vector atomics for the block the entry has initialised in a launch of its own.  The pixels of a trip behind a seam of two
//           rows (planes smaller than a trip: every trip has some) go there directly.
// The grid is bounded: kMaxBlocks workgroups at most, each with ceil(trips / kMaxBlocks) trips.
#include "pvhip_common.h"
#include "pvhip_topk_keys.h"

using namespace pvhip;

namespace {

constexpr int      kQuad       = 4;                    // pixels per lane and trip
constexpr int      kTripPixels = kBlock * kQuad;       // pixels a workgroup takes per trip
static_assert(kTripPixels == 1024, "tests/test_segments.py states the same figure (TRIP_PIXELS) and stands at its seam");
constexpr unsigned kNaNOrder   = 0xFFFFFFFFu;
constexpr int      kVoid       = PVHIP_SEGMENT_VOID;

struct __attribute__((aligned(4))) F4 { unsigned x, y, z, w; };     // 16 bytes at any 4-byte phase

__device__ __forceinline__ unsigned order_of(unsigned bits) { return (unsigned)(topk_key(bits, 0u) >> 32); }

struct Best {
    unsigned ord[kQuad];
    int      cls[kQuad];
    __device__ __forceinline__ void take(int i, unsigned bits, int c) {
        const unsigned o = order_of(bits);
        if (o > ord[i]) { ord[i] = o; cls[i] = c; }
    }
    __device__ __forceinline__ void take(const F4& q, int c) {
        take(0, q.x, c); take(1, q.y, c); take(2, q.z, c); take(3, q.w, c);
    }
};

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

struct SegmentRule {
    int      c, h, w, size;             // size = h * w
    long long total;                    // n * h * w
    int      has_min;
    unsigned min_order;                 // order_of(min_score)
};

__global__ __launch_bounds__(kBlock) void segment_init_kernel(int* __restrict__ areas, int* __restrict__ extents, long long cells, int h, int w) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < cells; i += (long long)gridDim.x * kBlock) {
        areas[i] = 0;
        extents[4 * i + 0] = w;
        extents[4 * i + 1] = h;
        extents[4 * i + 2] = 0;
        extents[4 * i + 3] = 0;
    }
}

// `phase` = labels & 3: quad j holds the pixels 4 j - phase .. 4 j - phase + 3 of the flat run, those within [0, total).
// Workgroup b takes the trips [b * per_block, (b + 1) * per_block) below `trips`, consecutive pixels, and keeps the sums of one batch
// row, `held`, in LDS between them.
__global__ __launch_bounds__(kBlock) void segment_labels_kernel(const unsigned* __restrict__ x, SegmentRule rule, int phase, long long quads,
                                                                long long trips, int per_block, unsigned char* __restrict__ labels,
                                                                int* __restrict__ areas, int* __restrict__ extents) {
    __shared__ int sums[PVHIP_SEGMENT_MAX_CLASSES * 5];                 // per class: area, x0, y0, x1, y1 of row `held`
    const int lane = threadIdx.x & (kWave - 1);
    // (every thread of the workgroup: `r` is the same in all of them)  The sums of row r leave for the global block; the table is empty again.
    auto flush = [&](int r) {
        __syncthreads();
        for (int k = threadIdx.x; k < rule.c; k += kBlock) {
            int* cell = sums + 5 * k;
            if (r >= 0 && cell[0] > 0) {
                const size_t to = (size_t)r * rule.c + k;
                atomicAdd(areas + to, cell[0]);
                atomicMin(extents + 4 * to + 0, cell[1]);
                atomicMin(extents + 4 * to + 1, cell[2]);
                atomicMax(extents + 4 * to + 2, cell[3]);
                atomicMax(extents + 4 * to + 3, cell[4]);
            }
            cell[0] = 0; cell[1] = rule.w; cell[2] = rule.h; cell[3] = 0; cell[4] = 0;
        }
        __syncthreads();
    };
    int held = -1;
    const long long first_trip = (long long)blockIdx.x * per_block;
    const long long last_trip  = first_trip + per_block < trips ? first_trip + per_block : trips;
    for (long long trip = first_trip; trip < last_trip; ++trip) {      // (the same trips in every thread of the workgroup)
        {   // the batch row of the trip's first pixel
            const long long g = 4 * trip * kBlock - phase;
            const int r = (int)((unsigned)(g < 0 ? 0 : g) / (unsigned)rule.size);
            if (r != held) {
                flush(held);
                held = r;
            }
        }
        const long long j  = trip * kBlock + threadIdx.x;
        const long long g0 = 4 * j - phase;                            // the flat index of the quad's first pixel; < 0 for the first of a run off phase
        int  row[kQuad], pos[kQuad], px[kQuad], py[kQuad];
        bool live[kQuad];
        {   // one division by H * W and one by W per lane; the pixels behind the first step on from it (total < 2^31)
            const unsigned start = g0 < 0 ? 0u : (g0 < rule.total ? (unsigned)g0 : (unsigned)(rule.total - 1));
            int r = (int)(start / (unsigned)rule.size);
            int p = (int)(start - (unsigned)r * (unsigned)rule.size);
            int y = (int)((unsigned)p / (unsigned)rule.w);
            int xx = p - y * rule.w;
#pragma unroll
            for (int i = 0; i < kQuad; ++i) {
                const long long g = g0 + i;
                live[i] = j < quads && g >= 0 && g < rule.total;
                if (live[i] && g > (long long)start) {                  // (one step: g - 1 was `start` or the pixel before this one)
                    ++p; ++xx;
                    if (xx == rule.w) { xx = 0; ++y; }
                    if (p == rule.size) { p = 0; y = 0; ++r; }
                }
                row[i] = r; pos[i] = p; px[i] = xx; py[i] = y;
            }
        }
        const bool whole = live[0] && live[3];
        const bool wide  = whole && row[0] == row[3];
        Best best;
#pragma unroll
        for (int i = 0; i < kQuad; ++i) { best.ord[i] = 0u; best.cls[i] = 0; }          // (no order word is 0: class 0 is taken first)
        if (wide) {
            const unsigned* at = x + ((size_t)row[0] * rule.c) * (size_t)rule.size + pos[0];
            int c = 0;
            for (; c + 4 <= rule.c; c += 4) {
                const F4 q0 = *reinterpret_cast<const F4*>(at);
                const F4 q1 = *reinterpret_cast<const F4*>(at + (size_t)rule.size);
                const F4 q2 = *reinterpret_cast<const F4*>(at + 2 * (size_t)rule.size);
                const F4 q3 = *reinterpret_cast<const F4*>(at + 3 * (size_t)rule.size);
                best.take(q0, c); best.take(q1, c + 1); best.take(q2, c + 2); best.take(q3, c + 3);
                at += 4 * (size_t)rule.size;
            }
            for (; c < rule.c; ++c) {
                best.take(*reinterpret_cast<const F4*>(at), c);
                at += rule.size;
            }
        } else {
#pragma unroll
            for (int i = 0; i < kQuad; ++i) {
                if (!live[i]) continue;
                const unsigned* at = x + ((size_t)row[i] * rule.c) * (size_t)rule.size + pos[i];
                for (int c = 0; c < rule.c; ++c) {
                    best.take(i, *at, c);
                    at += rule.size;
                }
            }
        }
        int label[kQuad];
#pragma unroll
        for (int i = 0; i < kQuad; ++i)
            label[i] = (best.ord[i] == kNaNOrder || (rule.has_min && best.ord[i] < rule.min_order)) ? kVoid : best.cls[i];
        if (whole) {
            *reinterpret_cast<unsigned*>(labels + g0) = (unsigned)label[0] | ((unsigned)label[1] << 8) | ((unsigned)label[2] << 16) | ((unsigned)label[3] << 24);
        } else {
#pragma unroll
            for (int i = 0; i < kQuad; ++i)
                if (live[i]) labels[g0 + i] = (unsigned char)label[i];
        }
        // areas and extents: per (wave, row, class)
        bool has[kQuad];
#pragma unroll
        for (int i = 0; i < kQuad; ++i) has[i] = live[i] && label[i] != kVoid;
        for (;;) {                                                      // (the whole wave: every condition below is wave-uniform)
            const bool any = has[0] || has[1] || has[2] || has[3];
            const unsigned long long pending = __ballot(any);
            if (pending == 0ull) break;
            const int first = __ffsll((long long)pending) - 1;
            const int mine  = has[0] ? 0 : has[1] ? 1 : has[2] ? 2 : 3;
            int my_row = row[0], my_cls = label[0];
#pragma unroll
            for (int i = 1; i < kQuad; ++i)
                if (mine == i) { my_row = row[i]; my_cls = label[i]; }
            const int r = __shfl(my_row, first, kWave), k = __shfl(my_cls, first, kWave);
            int count = 0, x0 = rule.w, x1 = 0, y0 = 0, y1 = 0;
#pragma unroll
            for (int i = 0; i < kQuad; ++i) {
                if (has[i] && row[i] == r && label[i] == k) {
                    if (count == 0) y0 = py[i];                         // the lane's pixels stand in flat order: the first has its least y
                    y1 = py[i] + 1;
                    x0 = min(x0, px[i]);
                    x1 = max(x1, px[i] + 1);
                    ++count;
                    has[i] = false;
                }
            }
            const unsigned long long in = __ballot(count > 0);         // (never empty: lane `first` is in it)
            const int sum = __popcll(in) + __popcll(__ballot(count > 1)) + __popcll(__ballot(count > 2)) + __popcll(__ballot(count > 3));
            const int wx0 = wave_min_i32(x0), wx1 = wave_max_i32(x1);
            const int wy0 = __shfl(y0, __ffsll((long long)in) - 1, kWave);           // lanes, too, stand in flat order
            const int wy1 = __shfl(y1, 63 - __clzll((long long)in), kWave);
            if (lane == first) {
                if (r == held) {                                        // (LDS atomics: the four waves of the workgroup share the table)
                    int* cell = sums + 5 * k;
                    atomicAdd(cell + 0, sum);
                    atomicMin(cell + 1, wx0);
                    atomicMin(cell + 2, wy0);
                    atomicMax(cell + 3, wx1);
                    atomicMax(cell + 4, wy1);
                } else {                                                // the pixels of a trip behind the seam of two rows
                    const size_t cell = (size_t)r * rule.c + k;
                    atomicAdd(areas + cell, sum);
                    atomicMin(extents + 4 * cell + 0, wx0);
                    atomicMin(extents + 4 * cell + 1, wy0);
                    atomicMax(extents + 4 * cell + 2, wx1);
                    atomicMax(extents + 4 * cell + 3, wy1);
                }
            }
        }
    }
    flush(held);
}

int segment_form(int c, int h, int w) {
    if (c < 1 || c > PVHIP_SEGMENT_MAX_CLASSES || h < 1 || w < 1) return PVHIP_SEGMENT_FORM_NONE;
    const long long size = (long long)h * w;
    if (size < 2 || size > PVHIP_SEGMENT_MAX_PLANE) return PVHIP_SEGMENT_FORM_NONE;
    return PVHIP_SEGMENT_FORM_QUADS;
}

}  // namespace

extern "C" {

int pvhip_segment_labels_form(int c, int h, int w) { return segment_form(c, h, w); }

int pvhip_segment_labels_f32(const float* x, int n, int c, int h, int w, int has_min, float min_score,
                             unsigned char* labels, int* areas, int* extents) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(x != nullptr && labels != nullptr && areas != nullptr && extents != nullptr);
    PVHIP_CHECK_ARG(((uintptr_t)x & 3u) == 0 && ((uintptr_t)areas & 3u) == 0 && ((uintptr_t)extents & 3u) == 0);
    PVHIP_CHECK_ARG(n >= 1 && c >= 1 && h >= 1 && w >= 1);
    PVHIP_CHECK_ARG(c <= PVHIP_SEGMENT_MAX_CLASSES);
    PVHIP_CHECK_ARG(segment_form(c, h, w) != PVHIP_SEGMENT_FORM_NONE);          // 2 <= h * w <= 2^24
    PVHIP_CHECK_ARG((long long)n * h * w < (1LL << 31));
    PVHIP_CHECK_ARG(has_min == 0 || has_min == 1);
    PVHIP_CHECK_ARG(min_score - min_score == 0.0f);                              // finite
    unsigned min_bits;
    __builtin_memcpy(&min_bits, &min_score, sizeof min_bits);
    const unsigned mag = min_bits & 0x7FFFFFFFu;                                 // the order word of pvhip_topk_keys.h, of a finite value
    const unsigned min_order = mag == 0u ? 0x80000000u : ((min_bits & 0x80000000u) ? ~min_bits : (min_bits | 0x80000000u));
    const SegmentRule rule{c, h, w, h * w, (long long)n * h * w, has_min, min_order};
    const long long cells = (long long)n * c;
    hipLaunchKernelGGL(segment_init_kernel, dim3((unsigned)grid_for((size_t)cells)), dim3(kBlock), 0, state().stream, areas, extents, cells, h, w);
    PVHIP_LAUNCH_CHECK();
    const int       phase = (int)((uintptr_t)labels & 3u);
    const long long quads = (rule.total + phase + kQuad - 1) / kQuad;
    const long long trips = (quads + kBlock - 1) / kBlock;
    const int       per_block = (int)((trips + kMaxBlocks - 1) / kMaxBlocks);      // a bounded grid: kMaxBlocks workgroups at most (trips < 2^21)
    const dim3 grid((unsigned)((trips + per_block - 1) / per_block));
    hipLaunchKernelGGL(segment_labels_kernel, grid, dim3(kBlock), 0, state().stream, reinterpret_cast<const unsigned*>(x), rule, phase, quads,
                       trips, per_block, labels, areas, extents);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
