// The local maxima of every plane of a stack of heatmaps (n, K, H, W), on the device: what users of CenterNet-style detectors and of
// multi-person pose heads do on the host with a 3 x 3 maximum filter and a partial sort after reading the whole tensor back.
// include/pvhip.h states the rule (pvhip_heatmap_maxima_f32), pyopenvino_amd/maxima.py and tests/maxima_ref.py are the same in numpy and
// in plain loops.  One entry, two launches, no initialising launch, no global-memory atomics: three passes give the same bits.
//
// Launch 1, candidates (maxima_planes_kernel<TEAM>): planes are walked by a grid-stride loop, a team of TEAM threads per plane -- one
// wave (a workgroup of 64) up to kWavePlane elements, a workgroup of 256 beyond; pvhip_heatmap_maxima_form names which.
//   tiles   a plane goes through LDS in tiles of `rows` whole rows (where W > kChunk, 1022 for a workgroup and 510 for a wave: of column
//           chunks of kChunk), as 32-bit order words (the high word of the key of pvhip_topk_keys.h).  A tile is staged with one row
//           above and one below it (and one column on each side of a chunk): that halo is what is read from HBM twice, 2 / rows of a
//           trip (+ 2 / kChunk for a chunk).  rows is kTileWords / W - 2, at most kTileRows = 24 (or, for planes narrower than 128,
//           the rows that make kTileTarget words) and bounded by the key buffer below: 24 rows of a 128-wide plane (8 %), 10 rows of
//           a 512-wide one (20 %), the whole plane where it fits (26 x 26, 46 x 46, 32 x 57: no halo at all).  The launch asks for
//           the LDS this takes and no more: 13 KB + 8 KB for 128-wide planes, seven workgroups a CU.  Rows that are whole in LDS are
//           one flat run of global memory: 16-byte loads with head and tail peeled, at whatever 4-byte phase the plane stands; the
//           tile's origin in LDS is shifted by that phase, so that a piece is one 16-byte LDS store.
//   test    separable: a lane walks down a column strip with the maximum of three along x of the row above, its own row's three words
//           and the maximum of three of the row below in registers: three LDS reads per element, lanes on consecutive words.  Keys are
//           distinct, so "larger than every neighbour" is: the order word above those of the four neighbours before it in raster order,
//           not below those of the four behind it.  Outside the plane stands 0, below every order word; a NaN's word is all ones, which
//           nothing is above and which is never taken.  The 64-bit key is formed for a maximum only.
//   keep    (keep_add / keep_cut of pvhip_keep.h, used by both launches) keys above the floor are appended to a buffer in LDS through an LDS counter.
//           No two maxima are neighbours, so a tile adds at most ceil(rows / 2) * ceil(cols / 2) keys; when the next tile could
//           overflow the buffer it is sorted descending (the bitonic pattern of tiles_frames_kernel, over the next power of two of its
//           fill) and cut to the M wanted, and the M-th key becomes the floor: later keys that are not above it are skipped.  The keys
//           are distinct and the sort is total, so neither the number of maxima nor the order in which lanes find them shows in the
//           result.  min_score is the first floor (rule 2: the keys that pass are an upper set of the order).
//   out     the plane's at most M keys, descending and padded with zeros (no key is 0), to the scratch (n, K, M).
// Launch 2, rows (maxima_rows_kernel): one workgroup per batch row walks that row's K * M scratch keys kRowTrip at a time, re-keys them
// with the channel (rule 4: index c * H * W + p) and keeps the R largest by the same two functions; then one lane per slot reads the
// plane's own bits and, under PVHIP_PEAKS_QUARTER, the at most four neighbours (L2 hits), applies the point rule (pvhip_point_rule.h)
// and writes the slot; the slots behind the count get the filler, and counts[r] is written too.
#include <cstring>

#include "pvhip_common.h"
#include "pvhip_keep.h"
#include "pvhip_point_rule.h"
#include "pvhip_topk_keys.h"

using namespace pvhip;

namespace {

constexpr int kWavePlane = 1024;               // H * W at most for the wave form
constexpr int kTileRows  = 24;                 // rows of a tile at most, where a plane takes several
constexpr int kTileTarget = 3072;              // or, for planes narrower than 128, the rows that make as many words
constexpr int kRowKeys   = 2048;               // the key buffer of maxima_rows_kernel
constexpr int kRowTrip   = 1024;               // scratch keys it takes per trip: kRowKeys - PVHIP_MAXIMA_MAX_PER_ROW

template <int TEAM> struct Sizes;
// The most LDS a team takes (the launch asks for what the plane shape needs: PlanePlan).  kChunk: columns of a tile at most; a chunk and
// its two halo columns are a row of 512 or 1024 words, and three such rows fit the tile.
template <> struct Sizes<kWave>  { static constexpr int kTileWords = 1536, kKeys = 512, kChunk = 510; };       // 6 KB + 4 KB of LDS per wave
template <> struct Sizes<kBlock> { static constexpr int kTileWords = 6144, kKeys = 2048, kChunk = 1022; };     // 24 KB + 16 KB per workgroup

struct PlanePlan {
    int h, w;
    int cols, rows, pitch, full;       // a tile: `rows` x `cols` elements; LDS row pitch; full: cols == w, rows contiguous in memory
    int ncx, ncy;                      // tiles across and down a plane
    int bound;                         // maxima of one tile at most
    int cap, tile_words;               // LDS of a team: keys (a power of two >= keep + bound), words of a staged tile
    int keep;                          // M
    unsigned long long floor;          // keys not above it fail min_score (0: none given)
};

struct RowPlan {
    int k, h, w, keep, per_row, refine, space;
};

__device__ __forceinline__ unsigned order_word(unsigned bits) { return (unsigned)(topk_key(bits, 0u) >> 32); }

// `count` consecutive words of global memory as order words into LDS: 16-byte loads between the run's own 16-byte boundaries.
template <int TEAM>
__device__ __forceinline__ void stage_run(unsigned* dst, const unsigned* __restrict__ src, int count, int tid) {
    const int head = min(count, (int)(((16u - (unsigned)((uintptr_t)src & 15u)) & 15u) >> 2));
    const int npiece = (count - head) >> 2, tail = (count - head) & 3;
    if (tid < head + tail) {
        const int e = tid < head ? tid : head + 4 * npiece + (tid - head);
        dst[e] = order_word(src[e]);
    }
    const uint4* body = reinterpret_cast<const uint4*>(src + head);
    unsigned* to = dst + head;
    if ((((unsigned)(uintptr_t)to) & 15u) == 0u) {              // (the team as one: the tile's origin was shifted to make it so)
        for (int p = tid; p < npiece; p += TEAM) {
            const uint4 q = body[p];
            reinterpret_cast<uint4*>(to)[p] = make_uint4(order_word(q.x), order_word(q.y), order_word(q.z), order_word(q.w));
        }
    } else {
        for (int p = tid; p < npiece; p += TEAM) {
            const uint4 q = body[p];
            to[4 * p + 0] = order_word(q.x);
            to[4 * p + 1] = order_word(q.y);
            to[4 * p + 2] = order_word(q.z);
            to[4 * p + 3] = order_word(q.w);
        }
    }
}

struct Three {
    unsigned l, c, r;
};
__device__ __forceinline__ unsigned max3(const Three& t) { return max(max(t.l, t.c), t.r); }

template <int TEAM>
__global__ __launch_bounds__(TEAM) void maxima_planes_kernel(const float* __restrict__ x, long long planes, PlanePlan a,
                                                             unsigned long long* __restrict__ scratch) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds[];   // a.cap keys, then the tile's a.tile_words + 4 words: what
    unsigned long long* keys = lds;                                             // this plane shape needs, so that small planes get more teams a CU
    unsigned* tile_words = reinterpret_cast<unsigned*>(lds + a.cap);
    const int kKeys = a.cap;
    __shared__ int count;
    const int tid = threadIdx.x;
    const int size = a.h * a.w;
    for (long long i = blockIdx.x; i < planes; i += gridDim.x) {                // (the same trip count in every thread of the team)
        const unsigned* plane = reinterpret_cast<const unsigned*>(x) + (size_t)i * (size_t)size;
        if (tid == 0) count = 0;
        unsigned long long floor = a.floor;
        for (int t = 0; t < a.ncy * a.ncx; ++t) {
            const int ty = t / a.ncx, tx = t - ty * a.ncx;
            const int y0 = ty * a.rows, x0 = tx * a.cols;
            const int rr = min(a.rows, a.h - y0), cc = min(a.cols, a.w - x0);
            __syncthreads();                                                    // the keys of the tile before; its words have been read
            if (count + a.bound > kKeys) floor = keep_cut<TEAM>(keys, &count, kKeys, a.keep, floor);
            // ---- stage rows ya .. yb - 1, columns xa .. xb - 1; element (y, x) at tile[(y - ybase) * pitch + (x - xbase)]
            const int ybase = y0 - 1, ya = max(0, ybase), yb = min(a.h, y0 + rr + 1);
            const int xbase = a.full ? 0 : x0 - 1, xa = max(0, xbase), xb = a.full ? a.w : min(a.w, x0 + cc + 1);
            unsigned* tile = tile_words;
            if (a.full) {
                const unsigned* src = plane + ya * a.w;
                const int at = (ya - ybase) * a.pitch;
                tile += (int)((((unsigned)((uintptr_t)src >> 2)) - (unsigned)at) & 3u);       // LDS word and global word at one 16-byte phase
                stage_run<TEAM>(tile + at, src, (yb - ya) * a.w, tid);
            } else {
                for (int y = ya; y < yb; ++y)
                    stage_run<TEAM>(tile + (y - ybase) * a.pitch + (xa - xbase), plane + y * a.w + xa, xb - xa, tid);
            }
            __syncthreads();
            // ---- column strips: column x0 + s % cc, rows y0 + g * len .. of group g = s / cc
            const int groups = cc < TEAM ? max(1, min(rr, TEAM / cc)) : 1;
            const int len = (rr + groups - 1) / groups;
            for (int s = tid; s < cc * groups; s += TEAM) {
                const int g = s / cc, xx = x0 + (s - g * cc);
                const int ys = y0 + g * len, ye = min(y0 + rr, ys + len);
                if (ys >= ye) continue;
                const unsigned* col = tile + (xx - xbase);
                const bool left = xx > 0, right = xx < a.w - 1;
                auto three = [&](int y) {
                    Three v{0u, 0u, 0u};
                    if (y >= 0 && y < a.h) {
                        const unsigned* at = col + (y - ybase) * a.pitch;
                        v.c = at[0];
                        if (left) v.l = at[-1];
                        if (right) v.r = at[1];
                    }
                    return v;
                };
                unsigned above = max3(three(ys - 1));
                Three cur = three(ys);
                for (int y = ys; y < ye; ++y) {
                    const Three nxt = three(y + 1);
                    const unsigned below = max3(nxt), c = cur.c;
                    if (c != 0xFFFFFFFFu && c > above && c > cur.l && c >= cur.r && c >= below) {
                        const unsigned long long key = ((unsigned long long)c << 32) | (unsigned long long)(kIndexTop - (unsigned)(y * a.w + xx));
                        if (key > floor) keep_add(keys, &count, kKeys, key);
                    }
                    above = max3(cur);
                    cur = nxt;
                }
            }
        }
        __syncthreads();
        floor = keep_cut<TEAM>(keys, &count, kKeys, a.keep, floor);
        const int kept = min(count, a.keep);
        unsigned long long* out = scratch + (size_t)i * (size_t)a.keep;
        for (int j = tid; j < a.keep; j += TEAM) out[j] = j < kept ? keys[j] : 0ull;
        __syncthreads();                                                        // count and keys[] are written again for the next plane
    }
}

__global__ __launch_bounds__(kBlock) void maxima_rows_kernel(const float* __restrict__ x, const unsigned long long* __restrict__ scratch,
                                                             int n, RowPlan a, int* __restrict__ counts, int* __restrict__ channels,
                                                             int* __restrict__ positions, unsigned* __restrict__ scores,
                                                             unsigned* __restrict__ points) {
    __shared__ unsigned long long keys[kRowKeys];
    __shared__ int count;
    const int tid = threadIdx.x;
    const unsigned size = (unsigned)(a.h * a.w);
    const long long total = (long long)a.k * a.keep;
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        const unsigned long long* src = scratch + (size_t)r * (size_t)total;
        if (tid == 0) count = 0;
        unsigned long long floor = 0ull;
        for (long long base = 0; base < total; base += kRowTrip) {
            __syncthreads();
            if (count + kRowTrip > kRowKeys) floor = keep_cut<kBlock>(keys, &count, kRowKeys, a.per_row, floor);
            const long long end = min(total, base + kRowTrip);
            for (long long j = base + tid; j < end; j += kBlock) {
                const unsigned long long key = src[j];
                if (key == 0ull) continue;                                      // (padding)
                const unsigned c = (unsigned)(j / a.keep), p = kIndexTop - (unsigned)key;
                const unsigned long long rekeyed = (key & 0xFFFFFFFF00000000ull) | (unsigned long long)(kIndexTop - (c * size + p));
                if (rekeyed > floor) keep_add(keys, &count, kRowKeys, rekeyed);
            }
        }
        __syncthreads();
        floor = keep_cut<kBlock>(keys, &count, kRowKeys, a.per_row, floor);
        const int kept = min(count, a.per_row);
        if (tid == 0) counts[r] = kept;
        for (int j = tid; j < a.per_row; j += kBlock) {
            const size_t at = (size_t)r * (size_t)a.per_row + (size_t)j;
            int c = -1, p = -1;
            unsigned bits = kQuietNaN, ux = kQuietNaN, uy = kQuietNaN;
            if (j < kept) {
                const unsigned index = kIndexTop - (unsigned)keys[j];
                c = (int)(index / size);
                p = (int)(index - (unsigned)c * size);
                const float* plane = x + ((size_t)r * (size_t)a.k + (size_t)c) * (size_t)size;
                bits = reinterpret_cast<const unsigned*>(plane)[p];             // the plane's own bits
                point_of(plane, p, a.h, a.w, a.refine, a.space, ux, uy);
            }
            channels[at]       = c;
            positions[at]      = p;
            scores[at]         = bits;
            points[2 * at]     = ux;
            points[2 * at + 1] = uy;
        }
        __syncthreads();                                                        // count and keys[] are written again for the next row
    }
}

int maxima_form(int h, int w) {
    if (h < 1 || w < 1) return PVHIP_MAXIMA_FORM_NONE;
    const long long size = (long long)h * w;
    if (size < 2 || size > PVHIP_MAXIMA_MAX_PLANE) return PVHIP_MAXIMA_FORM_NONE;
    return size <= kWavePlane ? PVHIP_MAXIMA_FORM_WAVE : PVHIP_MAXIMA_FORM_BLOCK;
}

// The tiles of an (h, w) plane for a team with at most `tile_words` words and `cap` keys of LDS.  A tile is at most kTileRows rows: 2 / 24
// of halo is little, and what a smaller tile and key buffer leave of the CU's LDS goes to further teams, whose loads hide this one's barriers.
PlanePlan plane_plan(int h, int w, int tile_words, int cap, int chunk, int keep, unsigned long long floor) {
    PlanePlan a{};
    a.h = h;
    a.w = w;
    a.full  = w <= chunk;
    a.cols  = a.full ? w : chunk;
    a.pitch = a.full ? w : chunk + 2;
    const int across = (a.cols + 1) / 2;                                        // maxima of one row of a tile at most
    int rows = tile_words / a.pitch - 2;                                        // (>= 1: three rows of a chunk and its halo fit the tile)
    const int most = kTileRows > kTileTarget / a.pitch ? kTileRows : kTileTarget / a.pitch;      // (narrow planes: more rows, as many words)
    if (rows < h) rows = rows < most ? rows : most;                             // (a plane that fits whole stays whole)
    rows = rows < 2 * ((cap - PVHIP_MAXIMA_MAX_PER_PLANE) / across) ? rows : 2 * ((cap - PVHIP_MAXIMA_MAX_PER_PLANE) / across);
    a.rows  = rows < h ? rows : h;
    a.ncx   = (w + a.cols - 1) / a.cols;
    a.ncy   = (h + a.rows - 1) / a.rows;
    a.bound = ((a.rows + 1) / 2) * across;                                      // (<= cap - 256: a cut buffer and one tile's keys fit)
    a.keep  = keep;
    a.floor = floor;
    a.cap   = 2;
    while (a.cap < keep + a.bound) a.cap <<= 1;                                 // (<= cap)
    a.tile_words = (a.rows + 2) * a.pitch;
    return a;
}

size_t lds_bytes(const PlanePlan& a) { return 8u * (size_t)a.cap + 4u * (size_t)(a.tile_words + 4); }

}  // namespace

extern "C" {

int pvhip_heatmap_maxima_form(int h, int w) { return maxima_form(h, w); }

int pvhip_heatmap_maxima_f32(const float* x, int n, int k, int h, int w, int max_per_plane, int max_per_row, int refine, int space,
                             int has_min, float min_score, unsigned long long* scratch, int* counts, int* channels, int* positions,
                             float* scores, float* points) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(x != nullptr && scratch != nullptr && counts != nullptr && channels != nullptr && positions != nullptr && scores != nullptr &&
                    points != nullptr);
    PVHIP_CHECK_ARG(((uintptr_t)x & 3u) == 0 && ((uintptr_t)scratch & 7u) == 0 && ((uintptr_t)counts & 3u) == 0 && ((uintptr_t)channels & 3u) == 0 &&
                    ((uintptr_t)positions & 3u) == 0 && ((uintptr_t)scores & 3u) == 0 && ((uintptr_t)points & 3u) == 0);
    PVHIP_CHECK_ARG(n >= 1 && k >= 1 && h >= 1 && w >= 1);
    const int form = maxima_form(h, w);
    PVHIP_CHECK_ARG(form != PVHIP_MAXIMA_FORM_NONE);                             // 2 <= h * w <= 2^24
    PVHIP_CHECK_ARG((long long)k * h * w <= 0x7FFFFFFFLL);                       // rule 4's index c * h * w + p
    PVHIP_CHECK_ARG(max_per_plane >= 1 && max_per_plane <= PVHIP_MAXIMA_MAX_PER_PLANE);
    PVHIP_CHECK_ARG(max_per_row >= 1 && max_per_row <= PVHIP_MAXIMA_MAX_PER_ROW);
    PVHIP_CHECK_ARG((long long)n * k * max_per_plane < (1LL << 31));
    PVHIP_CHECK_ARG(refine == PVHIP_PEAKS_NONE || refine == PVHIP_PEAKS_QUARTER);
    PVHIP_CHECK_ARG(space == PVHIP_PEAKS_HEATMAP || space == PVHIP_PEAKS_NORMALISED);
    PVHIP_CHECK_ARG(has_min == 0 || has_min == 1);
    PVHIP_CHECK_ARG(min_score - min_score == 0.0f);                              // finite
    const long long planes = (long long)n * k;
    unsigned min_bits;
    memcpy(&min_bits, &min_score, sizeof min_bits);
    const unsigned mag = min_bits & 0x7FFFFFFFu;                                 // the order word of pvhip_topk_keys.h of a finite value
    const unsigned min_word = mag == 0u ? 0x80000000u : ((min_bits & 0x80000000u) ? ~min_bits : (min_bits | 0x80000000u));
    const unsigned long long floor = has_min ? (((unsigned long long)min_word << 32) - 1ull) : 0ull;
    if (form == PVHIP_MAXIMA_FORM_WAVE) {
        const PlanePlan a = plane_plan(h, w, Sizes<kWave>::kTileWords, Sizes<kWave>::kKeys, Sizes<kWave>::kChunk, max_per_plane, floor);
        const dim3 grid((unsigned)(planes < kMaxBlocks * 4 ? planes : kMaxBlocks * 4));
        hipLaunchKernelGGL(maxima_planes_kernel<kWave>, grid, dim3(kWave), lds_bytes(a), state().stream, x, planes, a, scratch);
    } else {
        const PlanePlan a = plane_plan(h, w, Sizes<kBlock>::kTileWords, Sizes<kBlock>::kKeys, Sizes<kBlock>::kChunk, max_per_plane, floor);
        const dim3 grid((unsigned)(planes < kMaxBlocks * 4 ? planes : kMaxBlocks * 4));
        hipLaunchKernelGGL(maxima_planes_kernel<kBlock>, grid, dim3(kBlock), lds_bytes(a), state().stream, x, planes, a, scratch);
    }
    PVHIP_LAUNCH_CHECK();
    const RowPlan rows{k, h, w, max_per_plane, max_per_row, refine, space};
    const dim3 grid((unsigned)(n < kMaxBlocks * 4 ? n : kMaxBlocks * 4));
    hipLaunchKernelGGL(maxima_rows_kernel, grid, dim3(kBlock), 0, state().stream, x, scratch, n, rows, counts, channels, positions,
                       reinterpret_cast<unsigned*>(scores), reinterpret_cast<unsigned*>(points));
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
