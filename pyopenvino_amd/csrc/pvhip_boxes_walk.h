// The walk of a dense detector head, shared by the kinds of answer that screen its anchors: launch 1 (score) of pvhip_boxes.hip and of
// pvhip_oriented.hip, and launch 3 (write) of both.  pvhip_boxes.hip describes the forms -- planes for NCA, teams of 16 or 64 lanes for
// NAC, 16-byte loads at any 4-byte phase --; here they are templates over RULE, the anchor test of a kind:
//   RULE::kAngle                       the anchor carries one further channel behind its classes, which the test reads: the planes lane
//                                      loads its quad of that plane, the team's first lane its one number; false: no such load is made
//   g.objectness                       0 or 1
//   g.passes(b0, b1, b2, b3, obj, cls, k, angle, score_bits)      steps 1 and 2 of the kind's rule for one anchor
// The key of an anchor that passes is that of (score bits, anchor), else 0; the winners are written either way.
#pragma once
#include "pvhip_common.h"
#include "pvhip_topk_keys.h"

namespace pvhip {
namespace dense {

constexpr int kQuad = 4;                                          // anchors per lane of the planes form
constexpr int kTeam = 16;                                         // lanes of a team of the short-row form
constexpr int kImagesPerBlock = kBlock / kWave;

struct __attribute__((aligned(4))) F4 { unsigned x, y, z, w; };  // 16 bytes at any 4-byte phase

struct Head {
    const unsigned* x;
    int n, a, c, e, layout;        // e = 4 + objectness + c, the numbers of an anchor that the class walk reads
    int es;                        // the numbers of an anchor in memory: e and the channels behind the classes
};

// An anchor's numbers as a rule takes them; `angle` is channel e, read only where the rule says so.
struct Anchor {
    float b0, b1, b2, b3, obj, cls, angle;
};

__device__ __forceinline__ unsigned order_of(unsigned bits) { return (unsigned)(topk_key(bits, 0u) >> 32); }

__device__ __forceinline__ void take_max(unsigned long long& best, unsigned long long key) { best = key > best ? key : best; }

// Anchor i of image r with the winner k, its numbers read from the tensor.
template <bool ANGLE>
__device__ __forceinline__ Anchor anchor_numbers(const Head& t, int objectness, int r, int i, int k) {
    const bool   planes = t.layout == PVHIP_BOXES_LAYOUT_NCA;
    const size_t step   = planes ? (size_t)t.a : (size_t)1;
    const unsigned* at  = t.x + (planes ? (size_t)r * t.es * (size_t)t.a + i : ((size_t)r * t.a + i) * (size_t)t.es);
    const int first = 4 + objectness;
    Anchor v;
    v.b0 = __uint_as_float(at[0]);
    v.b1 = __uint_as_float(at[step]);
    v.b2 = __uint_as_float(at[2 * step]);
    v.b3 = __uint_as_float(at[3 * step]);
    v.obj = objectness ? __uint_as_float(at[4 * step]) : 0.0f;
    v.cls = __uint_as_float(at[(size_t)(first + k) * step]);
    v.angle = 0.0f;
    if constexpr (ANGLE) v.angle = __uint_as_float(at[(size_t)t.e * step]);
    return v;
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
template <class RULE>
__global__ __launch_bounds__(kBlock) void boxes_planes_kernel(Head t, RULE g, long long items, int quads,
                                                              unsigned long long* __restrict__ keys, int* __restrict__ winners) {
    const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (j >= items) return;
    const int    r    = (int)(j / quads);
    const int    i0   = kQuad * (int)(j - (long long)r * quads);
    const size_t a    = (size_t)t.a;
    const unsigned* at = t.x + (size_t)r * t.es * a + i0;
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
    F4 angle{0u, 0u, 0u, 0u};
    if constexpr (RULE::kAngle) angle = load_quad(at, live);                    // (the plane behind the classes)
    const size_t to = (size_t)r * a + i0;
#pragma unroll
    for (int i = 0; i < kQuad; ++i) {
        if (i < live) {
            unsigned score_bits;
            const bool in = g.passes(__uint_as_float(word(b0, i)), __uint_as_float(word(b1, i)), __uint_as_float(word(b2, i)),
                                     __uint_as_float(word(b3, i)), __uint_as_float(word(obj, i)), __uint_as_float(best.bits[i]), best.cls[i],
                                     __uint_as_float(word(angle, i)), score_bits);
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

// Memory row m of n * a rows of es numbers, the first e of them read: anchor m % a of image m / a.
template <int TEAM, class RULE>
__global__ __launch_bounds__(kBlock) void boxes_rows_kernel(Head t, RULE g, int rows, unsigned long long* __restrict__ keys,
                                                            int* __restrict__ winners) {
    constexpr int kTeams = kBlock / TEAM;
    const int lane = threadIdx.x & (TEAM - 1);
    const int e = t.e, first = 4 + g.objectness;
    for (int m = blockIdx.x * kTeams + (int)threadIdx.x / TEAM; m < rows; m += gridDim.x * kTeams) {     // (the whole team: no barrier below)
        const unsigned* row = t.x + (size_t)m * t.es;
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
            const Anchor v = anchor_numbers<RULE::kAngle>(t, g.objectness, r, i, k);   // (the row's own lines, just loaded)
            const bool in = g.passes(v.b0, v.b1, v.b2, v.b3, v.obj, v.cls, k, v.angle, score_bits);
            keys[m]    = in ? topk_key(score_bits, (unsigned)i) : 0ull;
            winners[m] = k;
        }
    }
}

// ---- launch 3: rows of PIECES 16-byte pieces
template <int PIECES>
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
    const int4* from  = staging + PIECES * (size_t)r * per_image;
    int4*       to    = rows + PIECES * (size_t)base;
    for (int p = lane; p < PIECES * count; p += kWave) to[p] = from[p];
    if (r == n - 1 && lane == 0) header[2 * (size_t)n] = base + count;
}

inline int boxes_form(int layout, int a, int e) {
    if (a < 1 || e < 5) return PVHIP_BOXES_FORM_NONE;
    if (layout == PVHIP_BOXES_LAYOUT_NCA) return PVHIP_BOXES_FORM_PLANES;
    if (layout == PVHIP_BOXES_LAYOUT_NAC) return e <= PVHIP_BOXES_TEAM_ROW ? PVHIP_BOXES_FORM_ROWS_TEAM : PVHIP_BOXES_FORM_ROWS_WAVE;
    return PVHIP_BOXES_FORM_NONE;
}

// Launch 1 in the form of (t.layout, t.a, t.e), which the caller has found not to be NONE.
template <class RULE>
inline void launch_score(int form, const Head& t, const RULE& g, unsigned long long* keys, int* winners, hipStream_t stream) {
    const size_t anchors = (size_t)t.n * (size_t)t.a;
    if (form == PVHIP_BOXES_FORM_PLANES) {
        const int       quads = (t.a + kQuad - 1) / kQuad;
        const long long items = (long long)t.n * quads;
        const dim3 grid((unsigned)((items + kBlock - 1) / kBlock));             // n * a < 2^31 / 5: below 2^21 workgroups
        hipLaunchKernelGGL(boxes_planes_kernel<RULE>, grid, dim3(kBlock), 0, stream, t, g, items, quads, keys, winners);
    } else if (form == PVHIP_BOXES_FORM_ROWS_TEAM) {
        const dim3 grid((unsigned)grid_for(anchors, kBlock / kTeam));
        hipLaunchKernelGGL((boxes_rows_kernel<kTeam, RULE>), grid, dim3(kBlock), 0, stream, t, g, (int)anchors, keys, winners);
    } else {
        const dim3 grid((unsigned)grid_for(anchors, kBlock / kWave));
        hipLaunchKernelGGL((boxes_rows_kernel<kWave, RULE>), grid, dim3(kBlock), 0, stream, t, g, (int)anchors, keys, winners);
    }
}

}  // namespace dense
}  // namespace pvhip
