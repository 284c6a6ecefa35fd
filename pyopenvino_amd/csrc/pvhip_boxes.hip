// A dense detector head's answer on the device: the raw tensor of per-anchor boxes and class scores that a YOLO-style export ends in
// becomes the table of detections its users make on the host -- confidence filter, box decoding, greedy suppression -- after reading the
// whole tensor back.  include/pvhip.h states the rule (pvhip_dense_boxes_f32), pyopenvino_amd/boxes.py and tests/boxes_ref.py are the
// same in numpy and in plain loops.
//
// Three launches with the (n, a) 8-byte keys of pvhip_topk_keys.h, the (n, a) winning classes and the per-image staging rows between
// them; no global-memory atomics, no workgroup waits for another, so the bits repeat.
//   score   the tensor is read once.  anchor_in is the rule's steps 1 and 2 for one anchor; its key is that of (score bits, anchor) when it
//           passes, else 0 (no key of a number is 0).
//           planes  (NCA: the anchors of a channel are contiguous)  pvhip_segments.hip's walk across planes: a lane owns four consecutive
//                   anchors of one image and reads 16 bytes per channel at whatever 4-byte phase the plane stands (the last quad of an
//                   image with a % 4 != 0 reads its anchors one by one), four classes' loads ahead of the first comparison; a strictly
//                   larger order word replaces, so ties stay with the lower class and the first NaN stays.  The score's own bits travel
//                   with the order word.  One workgroup per 1024 anchors: n * a < 2^31 / 5, so the grid needs no cap.
//           rows    (NAC: the channels of an anchor are contiguous)  pvhip_topk.hip's row walk with one round, by a team of TEAM lanes per
//                   anchor: the row split at its 16-byte boundaries into head, body of 16-byte pieces and tail, the channels in front of
//                   the classes skipped, one team-wide maximum of keys.  TEAM = 16 (four anchors a wave) for rows of at most
//                   PVHIP_BOXES_TEAM_ROW numbers, where a wave would leave most of its lanes without a piece; TEAM = 64 above.  The team's
//                   first lane then reads the box, the objectness and the winner once more -- from the lines the team has just loaded --
//                   and decides.  The grid is bounded; the teams stride.
//   images  one workgroup of 1024 lanes per image.  It walks the image's keys a trip at a time and keeps the max_candidates largest by
//           keep_add / keep_cut (pvhip_keep.h) in a buffer of dynamic LDS, a power of two of at least twice max_candidates keys (64 KB at
//           4096): a cut buffer and one trip always fit.  The fill is read between two barriers, so that every lane decides alike whether to
//           cut.  selected is the number of nonzero keys.  Lane t then holds the sorted candidates t, t + 1024, ...: it reads their
//           numbers again, makes the rectangle by anchor_in -- the same function, the same bits -- and the workgroup suppresses greedily in
//           chunks of 64 places exactly as tiles_frames_kernel does (pvhip_tiles.hip describes it; Box and suppresses are shared through
//           pvhip_suppress.h).  A kept candidate's place is the number of kept ones before it; the first max_per_image go to the image's
//           staging rows in their final form, the counts to the header.
//   write   one wave per image, behind the images launch so every count is there: base = counts[0] + .. + counts[r - 1] (lane-strided
//           loads, a wave reduction); the image's rows are copied to rows base .. in 16-byte pieces.  The last image's wave writes total.
#include <cstring>

#include "pvhip_common.h"
#include "pvhip_keep.h"
#include "pvhip_suppress.h"
#include "pvhip_topk_keys.h"

using namespace pvhip;

namespace {

constexpr int kQuad        = 4;                                   // anchors per lane of the planes form
constexpr int kTeam        = 16;                                  // lanes of a team of the short-row form
constexpr int kMaxLabels   = 64;
constexpr int kMaxExtent   = 1 << 24;
constexpr int kMaxCand     = PVHIP_BOXES_MAX_CANDIDATES;
constexpr int kImageBlock  = 1024;                                // lanes of an image's workgroup
constexpr int kImageWaves  = kImageBlock / kWave;                 // 16
constexpr int kPerLane     = kMaxCand / kImageBlock;              // sorted places a lane keeps
constexpr int kChunks      = kMaxCand / kWave;                    // 64: one bit of a wave-wide scan each
constexpr int kMinKeys     = 2048;                                // the key buffer at least: a trip is never shorter than the workgroup
constexpr int kImagesPerBlock = kBlock / kWave;

struct __attribute__((aligned(4))) F4 { unsigned x, y, z, w; };  // 16 bytes at any 4-byte phase

// What the rule takes besides an anchor's own numbers.
struct BoxRule {
    const int* labels;     // [num_labels], or NULL: any class
    int   num_labels, objectness, box;
    float min_score;
    int   frame_h, frame_w, dx, dy, iw, ih, min_h, min_w;
};

struct Head {
    const unsigned* x;
    int n, a, c, e, layout;        // e = 4 + objectness + c
};

struct Rect {
    int x0, y0, w, h;
};

__device__ __forceinline__ unsigned order_of(unsigned bits) { return (unsigned)(topk_key(bits, 0u) >> 32); }

__device__ __forceinline__ void take_max(unsigned long long& best, unsigned long long key) { best = key > best ? key : best; }

// A corner in network pixels as a frame coordinate: three binary64 operations (the library is built without contraction).
__device__ __forceinline__ double to_frame(float p, int d, int extent, int i) { return ((double)p - (double)d) * (double)extent / (double)i; }

// Steps 1 and 2 of the rule for one anchor: its four box numbers, its objectness (unused without), its winning class and that class's
// score.  True when the anchor is in; `score_bits` and the frame rectangle `r` are left either way the rule got that far.
__device__ __forceinline__ bool anchor_in(const BoxRule& g, float b0, float b1, float b2, float b3, float obj, float cls, int k,
                                          unsigned& score_bits, Rect& r) {
    const float score = g.objectness ? obj * cls : cls;
    score_bits = __float_as_uint(score);
    if (!(score >= g.min_score)) return false;                                  // (a NaN too)
    if (!(isfinite(b0) && isfinite(b1) && isfinite(b2) && isfinite(b3))) return false;
    float xa = b0, ya = b1, xb = b2, yb = b3;
    if (g.box == PVHIP_BOXES_CXCYWH) {
        const float hw = b2 * 0.5f, hh = b3 * 0.5f;
        xa = b0 - hw; xb = b0 + hw;
        ya = b1 - hh; yb = b1 + hh;
    }
    const double fw = (double)g.frame_w, fh = (double)g.frame_h;
    r.x0 = (int)floor(fmin(fmax(to_frame(xa, g.dx, g.frame_w, g.iw), 0.0), fw));
    r.y0 = (int)floor(fmin(fmax(to_frame(ya, g.dy, g.frame_h, g.ih), 0.0), fh));
    r.w  = (int)ceil(fmin(fmax(to_frame(xb, g.dx, g.frame_w, g.iw), 0.0), fw)) - r.x0;
    r.h  = (int)ceil(fmin(fmax(to_frame(yb, g.dy, g.frame_h, g.ih), 0.0), fh)) - r.y0;
    if (r.w < g.min_w || r.h < g.min_h) return false;
    if (g.labels != nullptr) {
        bool listed = false;
        for (int j = 0; j < g.num_labels; ++j) listed = listed || k == g.labels[j];
        return listed;
    }
    return true;
}

// The same for anchor i of image r with the winner k, its numbers read from the tensor.
__device__ __forceinline__ bool anchor_at(const Head& t, const BoxRule& g, int r, int i, int k, unsigned& score_bits, Rect& rect) {
    const bool   planes = t.layout == PVHIP_BOXES_LAYOUT_NCA;
    const size_t step   = planes ? (size_t)t.a : (size_t)1;
    const unsigned* at  = t.x + (planes ? (size_t)r * t.e * (size_t)t.a + i : ((size_t)r * t.a + i) * (size_t)t.e);
    const int first = 4 + g.objectness;
    const float obj = g.objectness ? __uint_as_float(at[4 * step]) : 0.0f;
    return anchor_in(g, __uint_as_float(at[0]), __uint_as_float(at[step]), __uint_as_float(at[2 * step]), __uint_as_float(at[3 * step]), obj,
                     __uint_as_float(at[(size_t)(first + k) * step]), k, score_bits, rect);
}

// ---- launch 1, planes
struct Best {
    unsigned ord[kQuad], bits[kQuad];
    int      cls[kQuad];
    __device__ __forceinline__ void take(int i, unsigned b, int k) {
        const unsigned o = order_of(b);
        if (o > ord[i]) { ord[i] = o; bits[i] = b; cls[i] = k; }
    }
    __device__ __forceinline__ void take(const F4& q, int k) {
        take(0, q.x, k); take(1, q.y, k); take(2, q.z, k); take(3, q.w, k);
    }
};

// Four consecutive words, the first `live` of them read (the others are 0).
__device__ __forceinline__ F4 load_quad(const unsigned* p, int live) {
    if (live == kQuad) return *reinterpret_cast<const F4*>(p);
    F4 q{p[0], 0u, 0u, 0u};
    if (live > 1) q.y = p[1];
    if (live > 2) q.z = p[2];
    return q;
}

__device__ __forceinline__ unsigned word(const F4& q, int i) { return i == 0 ? q.x : i == 1 ? q.y : i == 2 ? q.z : q.w; }

// Item j of n * quads items: quad j % quads of image j / quads, the anchors 4 q .. 4 q + 3 below a.
__global__ __launch_bounds__(kBlock) void boxes_planes_kernel(Head t, BoxRule g, long long items, int quads,
                                                              unsigned long long* __restrict__ keys, int* __restrict__ winners) {
    const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (j >= items) return;
    const int    r    = (int)(j / quads);
    const int    i0   = kQuad * (int)(j - (long long)r * quads);
    const size_t a    = (size_t)t.a;
    const unsigned* at = t.x + (size_t)r * t.e * a + i0;
    const int live = min(kQuad, t.a - i0);
    const F4 b0 = load_quad(at, live), b1 = load_quad(at + a, live), b2 = load_quad(at + 2 * a, live), b3 = load_quad(at + 3 * a, live);
    F4 obj{0u, 0u, 0u, 0u};
    if (g.objectness) obj = load_quad(at + 4 * a, live);
    at += (size_t)(4 + g.objectness) * a;
    Best best;
#pragma unroll
    for (int i = 0; i < kQuad; ++i) { best.ord[i] = 0u; best.bits[i] = 0u; best.cls[i] = 0; }    // (no order word is 0: class 0 is taken first)
    if (live == kQuad) {
        int k = 0;
        for (; k + 4 <= t.c; k += 4) {
            const F4 q0 = *reinterpret_cast<const F4*>(at);
            const F4 q1 = *reinterpret_cast<const F4*>(at + a);
            const F4 q2 = *reinterpret_cast<const F4*>(at + 2 * a);
            const F4 q3 = *reinterpret_cast<const F4*>(at + 3 * a);
            best.take(q0, k); best.take(q1, k + 1); best.take(q2, k + 2); best.take(q3, k + 3);
            at += 4 * a;
        }
        for (; k < t.c; ++k) {
            best.take(*reinterpret_cast<const F4*>(at), k);
            at += a;
        }
    } else {
        for (int k = 0; k < t.c; ++k) {
#pragma unroll
            for (int i = 0; i < kQuad - 1; ++i)
                if (i < live) best.take(i, at[i], k);
            at += a;
        }
    }
    const size_t to = (size_t)r * a + i0;
#pragma unroll
    for (int i = 0; i < kQuad; ++i) {
        if (i < live) {
            unsigned score_bits;
            Rect     rect;
            const bool in = anchor_in(g, __uint_as_float(word(b0, i)), __uint_as_float(word(b1, i)), __uint_as_float(word(b2, i)),
                                      __uint_as_float(word(b3, i)), __uint_as_float(word(obj, i)), __uint_as_float(best.bits[i]), best.cls[i],
                                      score_bits, rect);
            keys[to + i]    = in ? topk_key(score_bits, (unsigned)(i0 + i)) : 0ull;
            winners[to + i] = best.cls[i];
        }
    }
}

// ---- launch 1, rows
template <int TEAM>
__device__ __forceinline__ unsigned long long team_max_u64(unsigned long long v) {
#pragma unroll
    for (int m = TEAM / 2; m >= 1; m >>= 1) {                                   // (partners stay inside the team: it is TEAM-aligned in its wave)
        const unsigned long long o = __shfl_xor(v, m, kWave);
        v = o > v ? o : v;
    }
    return v;
}

// Memory row m of n * a rows of e numbers: anchor m % a of image m / a.
template <int TEAM>
__global__ __launch_bounds__(kBlock) void boxes_rows_kernel(Head t, BoxRule g, int rows, unsigned long long* __restrict__ keys,
                                                            int* __restrict__ winners) {
    constexpr int kTeams = kBlock / TEAM;
    const int lane = threadIdx.x & (TEAM - 1);
    const int e = t.e, first = 4 + g.objectness;
    for (int m = blockIdx.x * kTeams + (int)threadIdx.x / TEAM; m < rows; m += gridDim.x * kTeams) {     // (the whole team: no barrier below)
        const unsigned* row = t.x + (size_t)m * e;
        // head | body of 16-byte pieces | tail
        const int head = min(e, (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2));
        const int npiece = (e - head) >> 2, tail = (e - head) & 3;
        const uint4* body = reinterpret_cast<const uint4*>(row + head);
        unsigned long long best = 0ull;
        if (lane < head + tail) {                                               // lanes 0-5: one element of the head or the tail
            const int edge = lane < head ? lane : head + 4 * npiece + (lane - head);
            if (edge >= first) best = topk_key(row[edge], (unsigned)(edge - first));
        }
        for (int p = lane; p < npiece; p += TEAM) {
            const uint4 q  = body[p];
            const int   at = head + 4 * p - first;                              // the class of q.x; the box and the objectness are below 0
            if (at + 0 >= 0) take_max(best, topk_key(q.x, (unsigned)(at + 0)));
            if (at + 1 >= 0) take_max(best, topk_key(q.y, (unsigned)(at + 1)));
            if (at + 2 >= 0) take_max(best, topk_key(q.z, (unsigned)(at + 2)));
            if (at + 3 >= 0) take_max(best, topk_key(q.w, (unsigned)(at + 3)));
        }
        best = team_max_u64<TEAM>(best);                                        // (c >= 1: never 0)
        if (lane == 0) {
            const int k = (int)(kIndexTop - (unsigned)best);
            const int r = m / t.a, i = m - r * t.a;
            unsigned score_bits;
            Rect     rect;
            const bool in = anchor_at(t, g, r, i, k, score_bits, rect);         // (the row's own lines, just loaded)
            keys[m]    = in ? topk_key(score_bits, (unsigned)i) : 0ull;
            winners[m] = k;
        }
    }
}

// ---- launch 2
struct ImageArgs {
    Head     t;
    BoxRule  g;
    const unsigned long long* keys;    // [n][a]
    const int* winners;                // [n][a]
    int4*    staging;                  // [n][per_image][2]
    int*     header;                   // counts[n], selected[n], total
    int      keep, cap, per_image, kind, per_label;      // keep = max_candidates; cap: keys of the buffer
    float    threshold;
};

__global__ __launch_bounds__(kImageBlock) void boxes_images_kernel(ImageArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];   // a.cap keys
    __shared__ unsigned long long kept_mask[kChunks];
    __shared__ int4 chunk_box[2][kWave];
    __shared__ int  chunk_label[2][kWave];
    __shared__ int  before[kChunks + 1];                      // kept candidates in front of a chunk; [kChunks]: all of them
    __shared__ int  wave_sum[kImageWaves];
    __shared__ int  count;

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int r = blockIdx.x, A = a.t.a;
    const unsigned long long* src = a.keys + (size_t)r * A;

    // ---- the a.keep largest keys of the image
    if (tid == 0) count = 0;
    if (tid < kChunks) kept_mask[tid] = 0ull;
    const int trip = a.cap - a.keep;                                            // (>= a.keep, >= kImageBlock)
    unsigned long long floor = 0ull;
    int mine = 0;
    for (int base = 0; base < A; base += trip) {                                // (the same trips in every thread)
        __syncthreads();
        const int fill = count;
        __syncthreads();                                                        // (nobody adds before everybody has read the fill)
        if (fill + trip > a.cap) floor = keep_cut<kImageBlock>(keys, &count, a.cap, a.keep, floor);
        const int end = min(A, base + trip);                                    // (base + trip < 2^31 + 2^13: a < 2^31 / 5)
        for (int j = base + tid; j < end; j += kImageBlock) {
            const unsigned long long key = src[j];
            mine += key != 0ull;
            if (key > floor) keep_add(keys, &count, a.cap, key);
        }
    }
    __syncthreads();
    floor = keep_cut<kImageBlock>(keys, &count, a.cap, a.keep, floor);
    const int cnt = min(count, a.keep);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, kWave);
    if (lane == 0) wave_sum[wave] = mine;
    __syncthreads();
    int selected = 0;
#pragma unroll
    for (int i = 0; i < kImageWaves; ++i) selected += wave_sum[i];

    // ---- this lane's candidates: sorted places q * 1024 + tid
    Box      box[kPerLane];
    int      anchor[kPerLane];
    unsigned score[kPerLane];
    bool     alive[kPerLane];
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) {
        const int p = q * kImageBlock + tid;
        alive[q]  = p < cnt;
        anchor[q] = 0;
        score[q]  = 0u;
        box[q]    = Box{0, 0, 0, 0, 0};
        if (alive[q]) {
            anchor[q] = (int)(kIndexTop - (unsigned)keys[p]);
            const int k = a.winners[(size_t)r * A + anchor[q]];
            Rect rect{0, 0, 0, 0};
            anchor_at(a.t, a.g, r, anchor[q], k, score[q], rect);               // (true: its key was not 0)
            box[q] = Box{rect.x0, rect.y0, rect.w, rect.h, k};
        }
    }

    // ---- greedy suppression, a chunk of 64 places at a time (tiles_frames_kernel's)
    const bool   per_label = a.per_label != 0;
    const double threshold = (double)a.threshold;
    int  kept = 0;
    bool more = true;
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) {
        for (int wv = 0; wv < kImageWaves && more; ++wv) {
            const int c = q * kImageWaves + wv, buf = c & 1;
            if (c * kWave >= cnt || kept >= a.per_image) {                      // (uniform over the workgroup)
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
                const int4 rb = chunk_box[buf][t];
                const Box  j{rb.x, rb.y, rb.z, rb.w, chunk_label[buf][t]};
#pragma unroll
                for (int q2 = q; q2 < kPerLane; ++q2) {                         // the places behind chunk c
                    if ((q2 > q || wave > wv) && alive[q2] && suppresses(j, box[q2], a.kind, per_label, threshold)) alive[q2] = false;
                }
            }
        }
    }
    __syncthreads();

    // ---- places, rows, counts
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
    int4* out = a.staging + 2 * (size_t)r * a.per_image;
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) {
        const int p = q * kImageBlock + tid;
        if (p < cnt) {
            const int c = q * kImageWaves + wave;
            const unsigned long long mask = kept_mask[c];                       // (0 for a chunk the loop never reached)
            const int at = before[c] + __popcll(mask & ((1ull << lane) - 1ull));
            if (((mask >> lane) & 1ull) && at < a.per_image) {
                out[2 * at + 0] = make_int4(r, box[q].x0, box[q].y0, box[q].w);
                out[2 * at + 1] = make_int4(box[q].h, box[q].label, (int)score[q], (int)((unsigned)r * (unsigned)A + (unsigned)anchor[q]));
            }
        }
    }
    if (tid == 0) {
        a.header[r]           = min(before[kChunks], a.per_image);
        a.header[a.t.n + r]   = selected;
    }
}

// ---- launch 3
__global__ __launch_bounds__(kBlock) void boxes_write_kernel(const int4* __restrict__ staging, int n, int per_image, int* __restrict__ header,
                                                             int4* __restrict__ rows) {
    const int lane = threadIdx.x & (kWave - 1);
    const int r    = blockIdx.x * kImagesPerBlock + (threadIdx.x >> 6);
    if (r >= n) return;                                                         // (the whole wave)
    int base = 0;                                                               // rows of the images before r
    for (int i = lane; i < r; i += kWave) base += header[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) base += __shfl_xor(base, d, kWave);
    const int   count = header[r];
    const int4* from  = staging + 2 * (size_t)r * per_image;
    int4*       to    = rows + 2 * (size_t)base;
    for (int p = lane; p < 2 * count; p += kWave) to[p] = from[p];
    if (r == n - 1 && lane == 0) header[2 * (size_t)n] = base + count;
}

int boxes_form(int layout, int a, int e) {
    if (a < 1 || e < 5) return PVHIP_BOXES_FORM_NONE;
    if (layout == PVHIP_BOXES_LAYOUT_NCA) return PVHIP_BOXES_FORM_PLANES;
    if (layout == PVHIP_BOXES_LAYOUT_NAC) return e <= PVHIP_BOXES_TEAM_ROW ? PVHIP_BOXES_FORM_ROWS_TEAM : PVHIP_BOXES_FORM_ROWS_WAVE;
    return PVHIP_BOXES_FORM_NONE;
}

}  // namespace

extern "C" {

int pvhip_dense_boxes_form(int layout, int a, int e) { return boxes_form(layout, a, e); }

int pvhip_dense_boxes_f32(const float* x, int n, int a, int c, int layout, int objectness, int box, float min_score,
                          const int* labels, int num_labels, int frame_h, int frame_w, int dx, int dy, int iw, int ih,
                          int min_h, int min_w, int max_candidates, int overlap, float threshold, int per_label, int max_per_image,
                          void* scratch, int* header, int* rows) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(x != nullptr && scratch != nullptr && header != nullptr && rows != nullptr);
    PVHIP_CHECK_ARG(((uintptr_t)x & 3u) == 0 && ((uintptr_t)header & 3u) == 0 && ((uintptr_t)labels & 3u) == 0);
    PVHIP_CHECK_ARG(((uintptr_t)rows & 15u) == 0 && ((uintptr_t)scratch & 15u) == 0);
    PVHIP_CHECK_ARG(n >= 1 && a >= 1 && c >= 1);
    PVHIP_CHECK_ARG(objectness == 0 || objectness == 1);
    PVHIP_CHECK_ARG((long long)n * a * (4LL + objectness + c) < (1LL << 31));
    const int e = 4 + objectness + c;
    const int form = boxes_form(layout, a, e);
    PVHIP_CHECK_ARG(form != PVHIP_BOXES_FORM_NONE);                              // layout one of the two
    PVHIP_CHECK_ARG(box == PVHIP_BOXES_CXCYWH || box == PVHIP_BOXES_XYXY);
    PVHIP_CHECK_ARG(min_score - min_score == 0.0f);                              // finite
    PVHIP_CHECK_ARG(num_labels >= 0 && num_labels <= kMaxLabels && (num_labels == 0 || labels != nullptr));   // (NULL: any class)
    PVHIP_CHECK_ARG(frame_h >= 1 && frame_h <= kMaxExtent && frame_w >= 1 && frame_w <= kMaxExtent);
    PVHIP_CHECK_ARG(iw >= 1 && iw <= kMaxExtent && ih >= 1 && ih <= kMaxExtent && dx >= 0 && dx <= kMaxExtent && dy >= 0 && dy <= kMaxExtent);
    PVHIP_CHECK_ARG(min_h >= 1 && min_w >= 1);
    PVHIP_CHECK_ARG(max_candidates >= 1 && max_candidates <= kMaxCand);
    PVHIP_CHECK_ARG(max_per_image >= 1 && max_per_image <= max_candidates);
    PVHIP_CHECK_ARG(overlap == PVHIP_OVERLAP_IOU || overlap == PVHIP_OVERLAP_IOS);
    PVHIP_CHECK_ARG(threshold >= 0.0f && threshold <= 1.0f);                    // (false for NaN)
    PVHIP_CHECK_ARG(per_label == 0 || per_label == 1);

    const Head    t{reinterpret_cast<const unsigned*>(x), n, a, c, e, layout};
    const BoxRule g{labels, num_labels, objectness, box, min_score, frame_h, frame_w, dx, dy, iw, ih, min_h, min_w};
    const size_t  anchors = (size_t)n * (size_t)a;
    char* const   base    = static_cast<char*>(scratch);
    unsigned long long* keys    = reinterpret_cast<unsigned long long*>(base);
    int*                winners = reinterpret_cast<int*>(base + 8 * anchors);
    int4*               staging = reinterpret_cast<int4*>(base + ((12 * anchors + 15u) & ~(size_t)15u));

    ImageArgs im{t, g, keys, winners, staging, header, max_candidates, kMinKeys, max_per_image, overlap, per_label, threshold};
    while (im.cap < 2 * max_candidates) im.cap <<= 1;                           // (<= 8192 keys: 64 KB)
    static bool attr_set = false;                                               // once, for the largest buffer: no runtime call per pass
    if (!attr_set) {
        PVHIP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&boxes_images_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)(2 * kMaxCand * sizeof(unsigned long long))));
        attr_set = true;
    }

    if (form == PVHIP_BOXES_FORM_PLANES) {
        const int       quads = (a + kQuad - 1) / kQuad;
        const long long items = (long long)n * quads;
        const dim3 grid((unsigned)((items + kBlock - 1) / kBlock));             // n * a < 2^31 / 5: below 2^21 workgroups
        hipLaunchKernelGGL(boxes_planes_kernel, grid, dim3(kBlock), 0, state().stream, t, g, items, quads, keys, winners);
    } else if (form == PVHIP_BOXES_FORM_ROWS_TEAM) {
        const dim3 grid((unsigned)grid_for(anchors, kBlock / kTeam));
        hipLaunchKernelGGL(boxes_rows_kernel<kTeam>, grid, dim3(kBlock), 0, state().stream, t, g, (int)anchors, keys, winners);
    } else {
        const dim3 grid((unsigned)grid_for(anchors, kBlock / kWave));
        hipLaunchKernelGGL(boxes_rows_kernel<kWave>, grid, dim3(kBlock), 0, state().stream, t, g, (int)anchors, keys, winners);
    }
    PVHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(boxes_images_kernel, dim3((unsigned)n), dim3(kImageBlock), (size_t)im.cap * sizeof(unsigned long long), state().stream, im);
    PVHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(boxes_write_kernel, dim3((unsigned)((n + kImagesPerBlock - 1) / kImagesPerBlock)), dim3(kBlock), 0, state().stream,
                       staging, n, max_per_image, header, reinterpret_cast<int4*>(rows));
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
