// The greedy CTC decoding of a text recogniser's Result, on the device: what users of CRNN-style heads do on the host with
// x.argmax(-1) and a collapse after reading the whole tensor back.  include/pvhip.h states the rule (pvhip_ctc_greedy_f32),
// pyopenvino_amd/text.py and tests/text_ref.py are the same in numpy and in plain loops.
//
// Two launches with the (n, T) 8-byte keys of pvhip_topk_keys.h between them; no global-memory atomics, so the bits repeat.
//   winners  rows    (TNC, NTC: the classes of a timestep are contiguous)  pvhip_topk.hip's row walk with one round: one wave per
//                    (r, t) row, the row split at its 16-byte boundaries into head, body of 16-byte pieces and tail, one pass, one
//                    wave_max_u64, no LDS.  The grid is bounded by PVHIP_TEXT_MAX_BLOCKS workgroups of four waves; they stride.
//            planes  (NCT: the timesteps of a class are contiguous)  pvhip_segments.hip's walk across planes: a lane owns four
//                    consecutive timesteps of one batch row and reads 16 bytes per class at whatever 4-byte phase the plane stands
//                    (the last quad of a row with T % 4 != 0 reads its timesteps one by one), four classes' loads ahead of the first
//                    comparison; a strictly larger order word replaces, so ties stay with the lower class.  One workgroup per 1024
//                    timesteps: n * T < 2^30, so the grid needs no cap.
//   collapse one workgroup per batch row.  The row's keys (32 KB at most) are read in chunks of 256, once for void, which is one
//            __syncthreads_or, and once more, from the cache, for the slots: chunk by chunk, the slot of an emitting timestep is the chunks before it (a running
//            base, the same in every thread), the waves before it (four counts in LDS, two sets so that one barrier per chunk is
//            enough) and the lanes before it (a ballot and a popcount).  w(t - 1) is the neighbouring lane's key; lane 0 reads it.
//            The slots behind the string are filled by the same workgroup: every word of the row is written exactly once.
#include "pvhip_common.h"
#include "pvhip_topk_keys.h"

using namespace pvhip;

namespace {

constexpr int      kQuad       = 4;                                  // timesteps per lane of the planes form
constexpr int      kWaves      = kBlock / kWave;
constexpr unsigned kNaNOrder   = 0xFFFFFFFFu;
constexpr unsigned kQuietNaN   = 0x7FC00000u;
static_assert(PVHIP_TEXT_MAX_BLOCKS == kMaxBlocks, "the bounded grid of the library");

struct __attribute__((aligned(4))) F4 { unsigned x, y, z, w; };     // 16 bytes at any 4-byte phase

__device__ __forceinline__ unsigned order_of(unsigned bits) { return (unsigned)(topk_key(bits, 0u) >> 32); }

__device__ __forceinline__ void take_max(unsigned long long& best, unsigned long long key) { best = key > best ? key : best; }

// Memory row m of `rows` = n * t rows of c classes: timestep m / n of batch row m % n (TNC) or timestep m % t of batch row m / t (NTC).
__global__ __launch_bounds__(kBlock) void text_rows_kernel(const unsigned* __restrict__ x, int rows, int n, int t, int c, int layout,
                                                           unsigned long long* __restrict__ scratch) {
    const int lane = threadIdx.x & (kWave - 1);
    for (int m = blockIdx.x * kWaves + (threadIdx.x >> 6); m < rows; m += gridDim.x * kWaves) {      // (the whole wave: no barrier below)
        const unsigned* row = x + (size_t)m * c;
        // head | body of 16-byte pieces | tail
        const int head = min(c, (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2));
        const int npiece = (c - head) >> 2, tail = (c - head) & 3;
        const uint4* body = reinterpret_cast<const uint4*>(row + head);
        const bool has_edge = lane < head + tail;                               // lanes 0-5: one element of the head or the tail
        const int  edge     = lane < head ? lane : head + 4 * npiece + (lane - head);
        unsigned long long best = has_edge ? topk_key(row[edge], (unsigned)edge) : 0ull;
#pragma unroll 4
        for (int p = lane; p < npiece; p += kWave) {
            const uint4    q  = body[p];
            const unsigned at = (unsigned)(head + 4 * p);
            take_max(best, topk_key(q.x, at + 0u));
            take_max(best, topk_key(q.y, at + 1u));
            take_max(best, topk_key(q.z, at + 2u));
            take_max(best, topk_key(q.w, at + 3u));
        }
        best = wave_max_u64(best);                                              // (c >= 2: never 0)
        if (lane == 0) {
            const int r = layout == PVHIP_TEXT_LAYOUT_TNC ? m % n : m / t;
            const int i = layout == PVHIP_TEXT_LAYOUT_TNC ? m / n : m % t;
            scratch[(size_t)r * t + i] = best;
        }
    }
}

struct Best {
    unsigned ord[kQuad];
    int      cls[kQuad];
    __device__ __forceinline__ void take(int i, unsigned bits, int k) {
        const unsigned o = order_of(bits);
        if (o > ord[i]) { ord[i] = o; cls[i] = k; }
    }
    __device__ __forceinline__ void take(const F4& q, int k) {
        take(0, q.x, k); take(1, q.y, k); take(2, q.z, k); take(3, q.w, k);
    }
};

// Item j of n * quads items: quad j % quads of batch row j / quads, the timesteps 4 q .. 4 q + 3 below t.
__global__ __launch_bounds__(kBlock) void text_planes_kernel(const unsigned* __restrict__ x, long long items, int quads, int t, int c,
                                                             unsigned long long* __restrict__ scratch) {
    const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (j >= items) return;
    const int r  = (int)(j / quads);
    const int t0 = kQuad * (int)(j - (long long)r * quads);
    const unsigned* at = x + (size_t)r * c * (size_t)t + t0;
    Best best;
#pragma unroll
    for (int i = 0; i < kQuad; ++i) { best.ord[i] = 0u; best.cls[i] = 0; }      // (no order word is 0: class 0 is taken first)
    const int live = min(kQuad, t - t0);
    if (live == kQuad) {
        int k = 0;
        for (; k + 4 <= c; k += 4) {
            const F4 q0 = *reinterpret_cast<const F4*>(at);
            const F4 q1 = *reinterpret_cast<const F4*>(at + (size_t)t);
            const F4 q2 = *reinterpret_cast<const F4*>(at + 2 * (size_t)t);
            const F4 q3 = *reinterpret_cast<const F4*>(at + 3 * (size_t)t);
            best.take(q0, k); best.take(q1, k + 1); best.take(q2, k + 2); best.take(q3, k + 3);
            at += 4 * (size_t)t;
        }
        for (; k < c; ++k) {
            best.take(*reinterpret_cast<const F4*>(at), k);
            at += t;
        }
    } else {
        for (int k = 0; k < c; ++k) {
#pragma unroll
            for (int i = 0; i < kQuad - 1; ++i)
                if (i < live) best.take(i, at[i], k);
            at += t;
        }
    }
    unsigned long long* to = scratch + (size_t)r * t + t0;
#pragma unroll
    for (int i = 0; i < kQuad; ++i)
        if (i < live) to[i] = ((unsigned long long)best.ord[i] << 32) | (unsigned long long)(kIndexTop - (unsigned)best.cls[i]);
}

__global__ __launch_bounds__(kBlock) void text_collapse_kernel(const unsigned* __restrict__ x, int n, int t, int c, int layout, int blank,
                                                               int merge, const unsigned long long* __restrict__ scratch,
                                                               int* __restrict__ lengths, int* __restrict__ symbols,
                                                               unsigned* __restrict__ scores, int* __restrict__ steps) {
    __shared__ int counts[2][kWaves];
    const int r = blockIdx.x, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const unsigned long long* keys = scratch + (size_t)r * t;
    const int chunks = (t + kBlock - 1) / kBlock;
    int any_nan = 0;
    for (int s = (int)threadIdx.x; s < t; s += kBlock) any_nan |= (unsigned)(keys[s] >> 32) == kNaNOrder;
    const bool is_void = __syncthreads_or(any_nan) != 0;
    const size_t out = (size_t)r * t;
    int base = 0;                                                               // slots filled by the chunks before: the same in every thread
    if (!is_void) {
        for (int i = 0; i < chunks; ++i) {                                      // (the same trips in every thread: all meet the barrier)
            const int  s = i * kBlock + (int)threadIdx.x;
            const bool in = s < t;
            const int  w = in ? (int)(kIndexTop - (unsigned)keys[s]) : 0;       // (again: the row's keys are 32 KB at most and stand in the cache)
            // w(s - 1): the key of the lane before; lane 0 of a wave reads its neighbour's from memory
            int before = __shfl_up(w, 1, kWave);
            if (lane == 0 && in && s > 0) before = (int)(kIndexTop - (unsigned)keys[s - 1]);
            const bool emit = in && w != blank && (merge == 0 || s == 0 || w != before);
            const unsigned long long votes = __ballot(emit);
            if (lane == 0) counts[i & 1][wave] = __popcll(votes);
            __syncthreads();
            int slot = base + __popcll(votes & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
            for (int v = 0; v < kWaves; ++v) {
                const int count = counts[i & 1][v];
                slot  += v < wave ? count : 0;
                total += count;
            }
            if (emit) {
                const size_t from = layout == PVHIP_TEXT_LAYOUT_TNC ? ((size_t)s * n + r) * c + w
                                  : layout == PVHIP_TEXT_LAYOUT_NTC ? ((size_t)r * t + s) * c + w
                                                                    : ((size_t)r * c + w) * t + s;
                symbols[out + slot] = w;
                scores[out + slot]  = x[from];                                  // the score's own bits
                steps[out + slot]   = s;
            }
            base += total;
        }
    }
    for (int slot = base + (int)threadIdx.x; slot < t; slot += kBlock) {       // the filler behind the string: all of a void row
        symbols[out + slot] = -1;
        scores[out + slot]  = kQuietNaN;
        steps[out + slot]   = -1;
    }
    if (threadIdx.x == 0) lengths[r] = is_void ? -1 : base;
}

int text_form(int layout, int t, int c) {
    if (t < 1 || t > PVHIP_TEXT_MAX_STEPS || c < 2) return PVHIP_TEXT_FORM_NONE;
    if (layout == PVHIP_TEXT_LAYOUT_TNC || layout == PVHIP_TEXT_LAYOUT_NTC) return PVHIP_TEXT_FORM_ROWS;
    return layout == PVHIP_TEXT_LAYOUT_NCT ? PVHIP_TEXT_FORM_PLANES : PVHIP_TEXT_FORM_NONE;
}

}  // namespace

extern "C" {

int pvhip_ctc_greedy_form(int layout, int t, int c) { return text_form(layout, t, c); }

int pvhip_ctc_greedy_f32(const float* x, int n, int t, int c, int layout, int blank, int merge, unsigned long long* scratch,
                         int* lengths, int* symbols, float* scores, int* steps) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(x != nullptr && scratch != nullptr && lengths != nullptr && symbols != nullptr && scores != nullptr && steps != nullptr);
    PVHIP_CHECK_ARG(((uintptr_t)x & 3u) == 0 && ((uintptr_t)lengths & 3u) == 0 && ((uintptr_t)symbols & 3u) == 0
                    && ((uintptr_t)scores & 3u) == 0 && ((uintptr_t)steps & 3u) == 0);
    PVHIP_CHECK_ARG(((uintptr_t)scratch & 7u) == 0);
    PVHIP_CHECK_ARG(n >= 1 && t >= 1 && c >= 2);
    PVHIP_CHECK_ARG(t <= PVHIP_TEXT_MAX_STEPS);
    PVHIP_CHECK_ARG(layout == PVHIP_TEXT_LAYOUT_TNC || layout == PVHIP_TEXT_LAYOUT_NTC || layout == PVHIP_TEXT_LAYOUT_NCT);
    PVHIP_CHECK_ARG(blank >= 0 && blank < c);
    PVHIP_CHECK_ARG(merge == 0 || merge == 1);
    PVHIP_CHECK_ARG((long long)n * t * c < (1LL << 31));
    const unsigned* bits = reinterpret_cast<const unsigned*>(x);
    if (text_form(layout, t, c) == PVHIP_TEXT_FORM_ROWS) {
        const int rows = n * t;
        const dim3 grid((unsigned)grid_for((size_t)rows, kWaves));
        hipLaunchKernelGGL(text_rows_kernel, grid, dim3(kBlock), 0, state().stream, bits, rows, n, t, c, layout, scratch);
    } else {
        const int       quads = (t + kQuad - 1) / kQuad;
        const long long items = (long long)n * quads;
        const dim3 grid((unsigned)((items + kBlock - 1) / kBlock));             // n * t < 2^30: below 2^20 workgroups
        hipLaunchKernelGGL(text_planes_kernel, grid, dim3(kBlock), 0, state().stream, bits, items, quads, t, c, scratch);
    }
    PVHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(text_collapse_kernel, dim3((unsigned)n), dim3(kBlock), 0, state().stream, bits, n, t, c, layout, blank, merge,
                       scratch, lengths, symbols, reinterpret_cast<unsigned*>(scores), steps);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
