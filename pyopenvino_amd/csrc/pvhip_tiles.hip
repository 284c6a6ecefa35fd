// A tiled detector's answer on the device: the batch rows of one pass are tiles of m frames (a RoiInput's table); their DetectionOutput
// records become one table of frame detections -- shifted into frame pixels, ordered by score and greedily suppressed across the tiles
// of a frame -- what a caller did on the host after reading every record back.  include/pvhip.h states the rule
// (pvhip_detections_merge_tiles), tests/tiles_ref.py is the same in numpy; the screen and the rectangle are pvhip_detect_rule.h's, the
// walk over a tile's records is pvhip_detections_compact's.
//
// pvhip_detections_merge_regions is the same answer for batch rows that are REGIONS of any aspect -- a RoiInput's table or the table
// pvhip_detections_to_rois left on the device -- placed in the detector's input by an aspect-preserving fit: the candidates kernel is a
// template on FIT, each wave computes its region's fitted rectangle once (fit_rect, pvhip_fit_rect.h: the function the preprocessing launch
// placed the pixels with) and walks its records with it (walk_image<true>: every corner mapped back before the rectangle rule).  The
// frames and write kernels do not know the difference.
//
// Three launches on one stream, at most kMaxCandidates = 4096 candidates in all:
//   tiles   one wave per tile (walk_image): candidate `rank` < max_per_tile of tile b becomes row b max_per_tile + rank of the scratch,
//           already in its final form (f, x + x0, y + y0, w, h, label, score bits, record); taken[b] counts them.  A tile whose frame is
//           outside [0, m) or whose extent is not in [1, 2^24] takes nothing.
//   frames  one workgroup of 1024 lanes per frame, no other workgroup's words read or written.
//           keys    scratch row s of a tile of this frame becomes the 64-bit key (ordered score, ~s); every other slot is 0.  Rows of one
//                   frame stand in (tile, position) = record order, so "the lower record" is the lower s, and the rule's order is the
//                   descending order of the keys: a bitonic sort in LDS over the next power of two of n max_per_tile.
//           greedy  lane t keeps the candidates at sorted places t, t + 1024, ... in registers.  The places are taken in chunks of 64 --
//                   chunk c belongs to wave c % 16 --: the owning wave settles its chunk alone (a loop over the lanes still alive, the
//                   winner's rectangle broadcast by shuffles), publishes the chunk's kept mask and rectangles in LDS (two buffers, so one
//                   barrier per chunk), and every lane tests its later candidates against the kept ones.  It stops at the frame's last
//                   candidate or when max_per_frame are kept.
//           places  a kept candidate's place in its frame is the number of kept ones before it (the chunk masks, a wave scan); place[s]
//                   = that, or -1 for a suppressed or capped one; counts[f], selected[f].
//   write   one wave per tile again, behind the frames launch so every count is there: base = counts[0] + .. + counts[f - 1]
//           (lane-strided loads, a wave reduction); row s with place[s] >= 0 is copied to row base + place[s] in two 16-byte stores.
//           The last tile's wave writes total.
// No workgroup waits for another one and nothing is added atomically: every output word has one writer and its value depends on the
// records and the table alone.
#include "pvhip_common.h"
#include "pvhip_detect_rule.h"
#include "pvhip_fit_rect.h"
#include "pvhip_suppress.h"

using namespace pvhip;

namespace {

constexpr int kMaxCandidates = 4096;
constexpr int kFrameBlock    = 1024;                          // lanes of a frame's workgroup
constexpr int kFrameWaves    = kFrameBlock / kWave;           // 16
constexpr int kPerLane       = kMaxCandidates / kFrameBlock;  // sorted places a lane keeps
constexpr int kChunks        = kMaxCandidates / kWave;        // 64: one bit of a wave-wide scan each
constexpr int kTilesPerBlock = kBlock / kWave;
constexpr int kMaxExtent     = 1 << 24;                       // exact as fp32

struct MergeArgs {
    ScreenWalk  walk;      // the records [n * P][7] and the screen
    const int*  tiles;     // [n][5]: (f, x, y, w, h)
    int4*       cand;      // [n * per_tile][2]: candidate rows
    int*        place;     // [n * per_tile]: the place of a candidate in its frame's answer, or -1
    int*        taken;     // [n]: candidates of a tile
    int*        header;    // counts[m], selected[m], total
    int4*       rows;      // [min(n * per_tile, m * per_frame)][2]
    int   n, m, per_tile, per_frame, slots, sort_n, kind, per_label;
    float threshold;
};

// The detector's input extent and how a region was placed in it (1 LETTERBOX, 2 TOP_LEFT).
struct FitNet {
    int net_h, net_w, fit;
};

// FIT: launched with one FitNet behind the MergeArgs; without it the kernel's arguments -- and its code -- are what the tiles entry always
// launched.
template <bool FIT, typename... Net>
__global__ __launch_bounds__(kBlock) void tiles_candidates_kernel(MergeArgs a, Net... net) {
    const int b = blockIdx.x * kTilesPerBlock + (threadIdx.x >> 6);
    if (b >= a.n) return;                                                       // (the whole wave: nothing below meets a barrier)
    const int* t = a.tiles + 5 * (size_t)b;
    const int  f = t[0], x = t[1], y = t[2], w = t[3], h = t[4];
    int taken = 0;
    if (f >= 0 && f < a.m && w >= 1 && w <= kMaxExtent && h >= 1 && h <= kMaxExtent) {
        int4* out = a.cand + 2 * (size_t)b * a.per_tile;
        DetectionFit g{};
        if constexpr (FIT) {                                                    // (wave-uniform: once per region)
            const FitNet  q = (net, ...);
            const FitRect p = fit_rect(h, w, q.net_h, q.net_w, q.fit);
            g = DetectionFit{q.net_h, q.net_w, p.dx, p.dy, p.iw, p.ih};
        }
        const int seen = walk_image<FIT>(a.walk, b, h, w, a.per_tile, [&](int rank, int r, const DetectionRect& rect, const float* q) {
            // (a frame rectangle wraps like an int32 sum where the table is no RoiInput's: defined, and the rule's)
            out[2 * rank + 0] = make_int4(f, (int)((unsigned)x + (unsigned)rect.x0), (int)((unsigned)y + (unsigned)rect.y0), rect.w);
            out[2 * rank + 1] = make_int4(rect.h, detection_label(q[1]), (int)__float_as_uint(q[2]), r);
        }, g);
        taken = min(seen, a.per_tile);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) a.taken[b] = taken;
}

__global__ __launch_bounds__(kFrameBlock) void tiles_frames_kernel(MergeArgs a) {
    __shared__ unsigned long long keys[kMaxCandidates];       // 32 KB
    __shared__ unsigned long long kept_mask[kChunks];
    __shared__ int4 chunk_box[2][kWave];
    __shared__ int  chunk_label[2][kWave];
    __shared__ int  before[kChunks + 1];                      // kept candidates in front of a chunk; [kChunks]: all of them
    __shared__ int  wave_sum[kFrameWaves];

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int f = blockIdx.x;
    const unsigned* cand_words = reinterpret_cast<const unsigned*>(a.cand);

    // ---- keys
    int mine = 0;
    for (int s = tid; s < a.sort_n; s += kFrameBlock) {
        unsigned long long key = 0ull;
        if (s < a.slots) {
            const int b = s / a.per_tile, k = s - b * a.per_tile;
            if (a.tiles[5 * (size_t)b] == f && k < a.taken[b]) {                // (taken[b] is 0 for a tile that takes nothing)
                key = ((unsigned long long)ordered_score(cand_words[8 * (size_t)s + 6]) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)s);
                ++mine;
            }
        }
        keys[s] = key;
    }
    if (tid < kChunks) kept_mask[tid] = 0ull;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, kWave);
    if (lane == 0) wave_sum[wave] = mine;
    __syncthreads();
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < kFrameWaves; ++i) cnt += wave_sum[i];

    // ---- sort, descending: the valid keys are distinct, the zeros come last
    for (int k = 2; k <= a.sort_n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (a.sort_n >> 1); i += kFrameBlock) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const unsigned long long u = keys[lo], v = keys[hi];
                if (((lo & k) == 0) ? (u < v) : (u > v)) {
                    keys[lo] = v;
                    keys[hi] = u;
                }
            }
            __syncthreads();
        }
    }

    // ---- this lane's candidates: sorted places q * 1024 + tid
    Box  box[kPerLane];
    int  slot[kPerLane];
    bool alive[kPerLane];
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) {
        const int p = q * kFrameBlock + tid;
        alive[q] = p < cnt;
        slot[q]  = 0;
        box[q]   = Box{0, 0, 0, 0, 0};
        if (alive[q]) {
            slot[q] = (int)(0xFFFFFFFFu - (unsigned)keys[p]);
            const int4 r0 = a.cand[2 * (size_t)slot[q] + 0], r1 = a.cand[2 * (size_t)slot[q] + 1];
            box[q] = Box{r0.y, r0.z, r0.w, r1.x, r1.y};
        }
    }

    // ---- greedy suppression, a chunk of 64 places at a time
    const bool   per_label = a.per_label != 0;
    const double threshold = (double)a.threshold;
    int  kept = 0;
    bool more = true;
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) {
        for (int wv = 0; wv < kFrameWaves && more; ++wv) {
            const int c = q * kFrameWaves + wv, buf = c & 1;
            if (c * kWave >= cnt || kept >= a.per_frame) {                      // (uniform over the workgroup)
                more = false;
                break;
            }
            if (wave == wv) {                                                   // the owning wave settles its chunk alone
                bool live = alive[q];
                unsigned long long settled = 0ull;
                for (;;) {
                    const unsigned long long open = __ballot(live) & ~settled;
                    if (!open) break;
                    const int t = __builtin_ctzll(open);                        // the best one still alive: kept
                    settled |= (2ull << t) - 1ull;
                    const Box j{__shfl(box[q].x0, t, kWave), __shfl(box[q].y0, t, kWave), __shfl(box[q].w, t, kWave),
                                __shfl(box[q].h, t, kWave), __shfl(box[q].label, t, kWave)};
                    if (live && lane > t && suppresses(j, box[q], a.kind, per_label, threshold)) live = false;
                }
                alive[q] = live;
                const unsigned long long mask = __ballot(live);
                if (lane == 0) kept_mask[c] = mask;
                chunk_box[buf][lane]   = make_int4(box[q].x0, box[q].y0, box[q].w, box[q].h);
                chunk_label[buf][lane] = box[q].label;
            }
            __syncthreads();
            unsigned long long mask = kept_mask[c];
            kept += __popcll(mask);
            while (mask) {                                                      // (uniform: every lane walks the same kept ones)
                const int  t = __builtin_ctzll(mask);
                mask &= mask - 1ull;
                const int4 r = chunk_box[buf][t];
                const Box  j{r.x, r.y, r.z, r.w, chunk_label[buf][t]};
#pragma unroll
                for (int q2 = q; q2 < kPerLane; ++q2) {                         // the places behind chunk c
                    if ((q2 > q || wave > wv) && alive[q2] && suppresses(j, box[q2], a.kind, per_label, threshold)) alive[q2] = false;
                }
            }
        }
    }
    __syncthreads();

    // ---- places
    if (wave == 0) {
        const int own = __popcll(kept_mask[lane]);
        int upto = own;                                                         // inclusive scan over the 64 chunks
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int o = __shfl_up(upto, d, kWave);
            if (lane >= d) upto += o;
        }
        before[lane] = upto - own;
        if (lane == kWave - 1) before[kChunks] = upto;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) {
        const int p = q * kFrameBlock + tid;
        if (p < cnt) {
            const int c = q * kFrameWaves + wave;
            const unsigned long long mask = kept_mask[c];
            const int at = before[c] + __popcll(mask & ((1ull << lane) - 1ull));
            a.place[slot[q]] = ((mask >> lane) & 1ull) && at < a.per_frame ? at : -1;
        }
    }
    if (tid == 0) {
        a.header[f]       = min(before[kChunks], a.per_frame);
        a.header[a.m + f] = cnt;
    }
}

__global__ __launch_bounds__(kBlock) void tiles_write_kernel(MergeArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int b    = blockIdx.x * kTilesPerBlock + (threadIdx.x >> 6);
    if (b >= a.n) return;
    const int taken = a.taken[b];
    if (taken > 0) {                                                            // (so the tile's frame is in [0, m))
        const int f = a.tiles[5 * (size_t)b];
        int base = 0;                                                           // rows of the frames before f (<= 4096)
        for (int i = lane; i < f; i += kWave) base += a.header[i];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) base += __shfl_xor(base, d, kWave);
        for (int k = lane; k < taken; k += kWave) {
            const size_t s = (size_t)b * a.per_tile + k;
            const int    at = a.place[s];
            if (at >= 0) {
                a.rows[2 * (size_t)(base + at) + 0] = a.cand[2 * s + 0];
                a.rows[2 * (size_t)(base + at) + 1] = a.cand[2 * s + 1];
            }
        }
    }
    if (b == a.n - 1) {
        int total = 0;
        for (int i = lane; i < a.m; i += kWave) total += a.header[i];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) total += __shfl_xor(total, d, kWave);
        if (lane == 0) a.header[2 * (size_t)a.m] = total;
    }
}

}  // namespace

// The argument checks and the three launches of both entries; fit 0: no mapping at all (net_h, net_w unused).
static int pvhip_detections_merge(const float* records, const int* tiles, int n, int records_per_tile, int frames, float min_confidence, const int* labels,
                                 int num_labels, int min_h, int min_w, int max_per_tile, int overlap, float threshold, int per_label,
                                 int max_per_frame, int net_h, int net_w, int fit, int* scratch, int* header, int* rows) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(records != nullptr && tiles != nullptr && scratch != nullptr && header != nullptr && rows != nullptr);
    PVHIP_CHECK_ARG(((uintptr_t)rows & 15u) == 0 && ((uintptr_t)scratch & 15u) == 0);
    PVHIP_CHECK_ARG(((uintptr_t)header & 3u) == 0 && ((uintptr_t)records & 3u) == 0 && ((uintptr_t)tiles & 3u) == 0);
    PVHIP_CHECK_ARG(n >= 1 && records_per_tile >= 1 && frames >= 1 && frames < (1 << 30));
    PVHIP_CHECK_ARG(min_h >= 1 && min_w >= 1 && max_per_tile >= 1 && max_per_frame >= 1);
    PVHIP_CHECK_ARG((long long)n * records_per_tile < ((1LL << 31) / 7));
    PVHIP_CHECK_ARG((long long)n * max_per_tile <= kMaxCandidates);
    PVHIP_CHECK_ARG(num_labels >= 0 && num_labels <= kScreenLabels && (num_labels == 0 || labels != nullptr));   // (NULL: any label)
    PVHIP_CHECK_ARG(overlap == PVHIP_OVERLAP_IOU || overlap == PVHIP_OVERLAP_IOS);
    PVHIP_CHECK_ARG(threshold >= 0.0f && threshold <= 1.0f);                    // (false for NaN)
    PVHIP_CHECK_ARG(per_label == 0 || per_label == 1);
    PVHIP_CHECK_ARG(fit >= 0 && fit <= 2);
    PVHIP_CHECK_ARG(fit == 0 || (net_h >= 1 && net_h <= kMaxExtent && net_w >= 1 && net_w <= kMaxExtent));
    MergeArgs a;
    a.walk  = ScreenWalk{records, labels, records_per_tile, num_labels, min_h, min_w, min_confidence};
    a.tiles = tiles;
    a.slots = n * max_per_tile;
    a.cand  = reinterpret_cast<int4*>(scratch);
    a.place = scratch + 8 * (size_t)a.slots;
    a.taken = a.place + a.slots;
    a.header = header; a.rows = reinterpret_cast<int4*>(rows);
    a.n = n; a.m = frames; a.per_tile = max_per_tile; a.per_frame = max_per_frame;
    a.kind = overlap; a.per_label = per_label; a.threshold = threshold;
    a.sort_n = 1;
    while (a.sort_n < a.slots) a.sort_n <<= 1;
    const dim3 tile_grid((n + kTilesPerBlock - 1) / kTilesPerBlock);
    if (fit != 0) hipLaunchKernelGGL((tiles_candidates_kernel<true, FitNet>), tile_grid, dim3(kBlock), 0, state().stream, a, FitNet{net_h, net_w, fit});
    else          hipLaunchKernelGGL(tiles_candidates_kernel<false>, tile_grid, dim3(kBlock), 0, state().stream, a);
    hipLaunchKernelGGL(tiles_frames_kernel, dim3(frames), dim3(kFrameBlock), 0, state().stream, a);
    hipLaunchKernelGGL(tiles_write_kernel, tile_grid, dim3(kBlock), 0, state().stream, a);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

extern "C" {

int pvhip_detections_merge_tiles(const float* records, const int* tiles, int n, int records_per_tile, int frames, float min_confidence,
                                 const int* labels, int num_labels, int min_h, int min_w, int max_per_tile, int overlap, float threshold,
                                 int per_label, int max_per_frame, int* scratch, int* header, int* rows) {
    return pvhip_detections_merge(records, tiles, n, records_per_tile, frames, min_confidence, labels, num_labels, min_h, min_w, max_per_tile,
                                  overlap, threshold, per_label, max_per_frame, 0, 0, 0, scratch, header, rows);
}

int pvhip_detections_merge_regions(const float* records, const int* regions, int n, int records_per_region, int frames, float min_confidence,
                                   const int* labels, int num_labels, int min_h, int min_w, int max_per_region, int overlap, float threshold,
                                   int per_label, int max_per_frame, int net_h, int net_w, int fit, int* scratch, int* header, int* rows) {
    return pvhip_detections_merge(records, regions, n, records_per_region, frames, min_confidence, labels, num_labels, min_h, min_w,
                                  max_per_region, overlap, threshold, per_label, max_per_frame, net_h, net_w, fit, scratch, header, rows);
}

}  // extern "C"
