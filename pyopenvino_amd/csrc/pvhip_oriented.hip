// An oriented detector head's answer on the device: the raw tensor of per-anchor (cx, cy, w, h, [objectness], class scores, angle) that a
// YOLOv8 / v11-obb style export ends in becomes the table of rotated boxes -- confidence filter, corners, greedy rotated suppression --
// that its users make on the host after reading the whole tensor back.  include/pvhip.h states the rule (pvhip_oriented_boxes_f32),
// pyopenvino_amd/oriented.py and tests/oriented_ref.py are the same in numpy and in plain loops.  Every operation of the geometry is one
// binary64 operation, rounded once; the library is built without contraction.
//
// Three launches with the (n, a) 8-byte keys, the (n, a) winners and the per-image staging rows between them; no global-memory atomics,
// no workgroup waits for another, so the bits repeat.
//   score   pvhip_boxes_walk.h's walk, instantiated over OrientedRule: steps 1 and 2 of the rule.  The angle is channel e = 4 + O + c of an
//           anchor of es = e + 1 numbers; the class walk steps over it, the planes lane or the team's first lane reads it once.
//   images  one workgroup of 1024 lanes per image.
//           keep     the K = max_candidates <= 1024 largest keys by pvhip_keep.h, in a buffer of 2048 keys, as boxes_images_kernel does.
//           stage    lane p owns sorted candidate p: it reads the five numbers again, makes cosine and sine by the rule's own polynomial,
//                    the four corners, the area and w + h, and stages them in LDS as structure-of-arrays doubles.
//           suppress by pull, a chunk of 64 places at a time.  For chunk c all 1024 lanes share the pairs (i in c) x (j kept in an earlier
//                    chunk): stage one is the cheap screen (i not yet dead, the labels, the distance bound); the pairs that pass are
//                    compacted by ballot prefix into a worklist in LDS, screening rounds going on until 1024 pairs wait or none are left;
//                    stage two clips the worklist, one pair per lane, so no lane idles behind another's long clip; a hit sets i's bit of the
//                    chunk's dead mask (an LDS OR: the order of hits does not show).  The 64 x 64 pairs inside the chunk, both still
//                    alive, go through the same two stages into 64 bit rows (row i: the j < i that would suppress i), and the chunk's wave
//                    resolves the greedy order on the rows with bit operations alone.  The kept places are appended, in order, to a list in
//                    LDS, which is what later chunks pull from and what the rows are written from.
//           rows     lane q < min(kept, max_per_image) writes kept place q: anchor from its key, numbers from the tensor, corners from LDS
//                    through to_frame, rounded to fp32.
//   write   pvhip_boxes_walk.h's per-image copy behind the counts, with rows of five 16-byte pieces.
//
// LDS of the images launch, for Kp = K rounded up to 64, all dynamic: 2048 keys (16 KB) | 10 Kp doubles: eight corner coordinates, area,
// w + h (80 KB at K = 1024) | 2 Kp floats: the centres, exact as fp32 (8 KB) | Kp labels (4 KB) | the worklist of 2048 pairs (8 KB) | the kept
// list of Kp places (4 KB): 120 KB at K = 1024 of gfx950's 160 KB, one workgroup a CU; static besides: a few hundred bytes of masks and
// counters.  A clip keeps its two polygons of at most eight vertices in the lane's private memory.
#include <cstring>

#include "pvhip_boxes_walk.h"
#include "pvhip_common.h"
#include "pvhip_keep.h"
#include "pvhip_topk_keys.h"

using namespace pvhip;
using namespace pvhip::dense;

namespace {

constexpr int kMaxLabels  = 64;
constexpr int kMaxExtent  = 1 << 24;
constexpr int kMaxCand    = PVHIP_ORIENTED_MAX_CANDIDATES;        // 1024: a lane per sorted candidate
constexpr int kImageBlock = 1024;
constexpr int kImageWaves = kImageBlock / kWave;
constexpr int kKeys       = 2048;                                 // the key buffer: twice the most candidates, a trip of a workgroup at least
constexpr int kWork       = 2 * kImageBlock;                      // the worklist: what waited and one screening round
constexpr int kVerts      = 8;                                    // a quadrilateral clipped by four half planes
constexpr int kPieces     = PVHIP_ORIENTED_ROW_BYTES / 16;        // 5
constexpr int kGeo        = 10;                                   // doubles per staged candidate

struct OrientedRule {
    const int* labels;     // [num_labels], or NULL: any class
    int   num_labels, objectness;
    float min_score, min_h, min_w;
    static constexpr bool kAngle = true;
    // Steps 1 and 2 of the rule for one anchor.
    __device__ __forceinline__ bool passes(float cx, float cy, float w, float h, float obj, float cls, int k, float angle,
                                           unsigned& score_bits) const {
        const float score = objectness ? obj * cls : cls;
        score_bits = __float_as_uint(score);
        if (!(score >= min_score)) return false;                                // (a NaN too)
        if (!(isfinite(cx) && isfinite(cy) && isfinite(w) && isfinite(h) && fabsf(angle) <= 8.0f)) return false;   // (false for a NaN angle)
        if (!(w >= min_w && h >= min_h)) return false;
        if (labels != nullptr) {
            bool listed = false;
            for (int j = 0; j < num_labels; ++j) listed = listed || k == labels[j];
            return listed;
        }
        return true;
    }
};

// Step 3: cosine and sine of an fp32 angle in [-8, 8], the rule's own: two-part reduction by pi / 2, Taylor polynomials in Horner form.
__device__ __forceinline__ void rule_cos_sin(float angle, double& cosine, double& sine) {
    const double a = (double)angle;
    const double k = rint(a * 0.6366197723675814);
    const double r = (a - k * 1.5707963267948966) - k * 6.123233995736766e-17;
    const double z = r * r;
    double S = 1.0 / 355687428096000.0;                                         // 1 / 17!
    S = -1.0 / 1307674368000.0 + z * S;
    S = 1.0 / 6227020800.0 + z * S;
    S = -1.0 / 39916800.0 + z * S;
    S = 1.0 / 362880.0 + z * S;
    S = -1.0 / 5040.0 + z * S;
    S = 1.0 / 120.0 + z * S;
    S = -1.0 / 6.0 + z * S;
    double C = 1.0 / 20922789888000.0;                                          // 1 / 16!
    C = -1.0 / 87178291200.0 + z * C;
    C = 1.0 / 479001600.0 + z * C;
    C = -1.0 / 3628800.0 + z * C;
    C = 1.0 / 40320.0 + z * C;
    C = -1.0 / 720.0 + z * C;
    C = 1.0 / 24.0 + z * C;
    C = -1.0 / 2.0 + z * C;
    const double s = r + r * (z * S), c = 1.0 + z * C;
    const int q = (int)k & 3;
    cosine = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
    sine   = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
}

// A coordinate in network pixels as a frame coordinate: boxes=' three binary64 operations, on a corner that is a double already.
__device__ __forceinline__ double to_frame(double p, int d, int extent, int i) { return (p - (double)d) * (double)extent / (double)i; }

// The staged candidates: structure-of-arrays over Kp places.
struct Staged {
    double* geo;           // [kGeo][kp]: x0, y0, x1, y1, x2, y2, x3, y3, area, w + h
    float*  centre;        // [2][kp]
    int*    label;         // [kp]
    int     kp;
    __device__ __forceinline__ double g(int f, int p) const { return geo[f * kp + p]; }
};

// Step 5's screen of the later candidate i against the kept candidate j: false where the rule says the overlap is 0 without a clip.
__device__ __forceinline__ bool may_overlap(const Staged& s, int i, int j, bool per_label) {
    if (per_label && s.label[i] != s.label[j]) return false;
    const double dx = (double)s.centre[i] - (double)s.centre[j], dy = (double)s.centre[s.kp + i] - (double)s.centre[s.kp + j];
    const double R = (s.g(9, i) + s.g(9, j)) * 0.5;
    return !(dx * dx + dy * dy > R * R);
}

// Step 5's clip and step 6's comparison: the polygon of i clipped by the four edges of j in order.
__device__ bool overlaps(const Staged& s, int i, int j, int kind, double threshold) {
    double px[kVerts], py[kVerts], ox[kVerts], oy[kVerts], side[kVerts];
    int n = 4;
#pragma unroll
    for (int v = 0; v < 4; ++v) { px[v] = s.g(2 * v, i); py[v] = s.g(2 * v + 1, i); }
    for (int e = 0; e < 4 && n > 0; ++e) {
        const int f = (e + 1) & 3;
        const double ax = s.g(2 * e, j), ay = s.g(2 * e + 1, j), bx = s.g(2 * f, j), by = s.g(2 * f + 1, j);
        for (int v = 0; v < n; ++v) side[v] = (bx - ax) * (py[v] - ay) - (by - ay) * (px[v] - ax);
        int m = 0;
        for (int v = 0; v < n; ++v) {
            const int    w  = v + 1 < n ? v + 1 : 0;
            const double sp = side[v], sq = side[w];
            const bool   in_p = sp >= 0.0, in_q = sq >= 0.0;
            if (in_p && m < kVerts) { ox[m] = px[v]; oy[m] = py[v]; ++m; }
            if (in_p != in_q && m < kVerts) {
                const double t = sp / (sp - sq);
                ox[m] = px[v] + t * (px[w] - px[v]);
                oy[m] = py[v] + t * (py[w] - py[v]);
                ++m;
            }
        }
        n = m;
        for (int v = 0; v < n; ++v) { px[v] = ox[v]; py[v] = oy[v]; }
    }
    double acc = 0.0;
    for (int v = 0; v < n; ++v) {
        const int w = v + 1 < n ? v + 1 : 0;
        acc = acc + (px[v] * py[w] - px[w] * py[v]);
    }
    const double inter = fabs(acc) * 0.5;
    const double ai = s.g(8, i), aj = s.g(8, j);
    const double den = kind == PVHIP_OVERLAP_IOS ? fmin(ai, aj) : (ai + aj) - inter;
    return inter > threshold * den;
}

struct ImageArgs {
    Head         t;
    OrientedRule g;
    const unsigned long long* keys;    // [n][a]
    const int*   winners;              // [n][a]
    int4*        staging;              // [n][per_image][kPieces]
    int*         header;               // counts[n], selected[n], total
    int          keep, kp, per_image, kind, per_label;       // keep = max_candidates, kp = keep rounded up to 64
    int          frame_h, frame_w, dx, dy, iw, ih;
    float        threshold;
};

// The dynamic LDS of the images launch for kp places, in bytes; the kernel carves it in this order.
inline size_t image_lds_bytes(int kp) {
    return (size_t)kKeys * 8 + (size_t)kGeo * kp * 8 + (size_t)2 * kp * 4 + (size_t)kp * 4 + (size_t)kWork * 4 + (size_t)kp * 4;
}

// Two stages over `total` pairs, every lane of the workgroup calling alike: pair(t, i, j) names pair t and says whether it is still of
// interest; those that may_overlap wait in the worklist; overlaps() runs on the worklist a pair per lane, hit(i, j) on each that does.
// *work_n is 0 on entry and on return.
template <class PAIR, class HIT>
__device__ __forceinline__ void run_pairs(int total, unsigned* work, int* work_n, const Staged& s, const ImageArgs& a, PAIR pair, HIT hit) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const bool   per_label = a.per_label != 0;
    const double threshold = (double)a.threshold;
    int pos = 0;
    while (pos < total) {                                                       // (uniform over the workgroup)
        int fill;
        do {
            const int t = pos + tid;
            int i = 0, j = 0;
            const bool pass = t < total && pair(t, i, j) && may_overlap(s, i, j, per_label);
            const unsigned long long b = __ballot(pass);
            int base = 0;
            if (lane == 0 && b) base = atomicAdd(work_n, __popcll(b));          // (LDS; fill <= kImageBlock before the round: never past kWork)
            base = __shfl(base, 0, kWave);
            if (pass) work[base + __popcll(b & ((1ull << lane) - 1ull))] = ((unsigned)i << 16) | (unsigned)j;
            pos += kImageBlock;
            __syncthreads();
            fill = *work_n;
            __syncthreads();                                                    // (nobody adds or resets before everybody has read the fill)
        } while (pos < total && fill < kImageBlock);
        for (int e = tid; e < fill; e += kImageBlock) {
            const int i = (int)(work[e] >> 16), j = (int)(work[e] & 0xFFFFu);
            if (overlaps(s, i, j, a.kind, threshold)) hit(i, j);
        }
        __syncthreads();
        if (tid == 0) *work_n = 0;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kImageBlock) void oriented_images_kernel(ImageArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];   // kKeys keys, then the blocks of image_lds_bytes
    __shared__ unsigned long long row[kWave];                                   // row i of the chunk: the j < i of it that would suppress i
    __shared__ unsigned long long dead;                                         // the chunk's places suppressed from earlier chunks
    __shared__ int wave_sum[kImageWaves];
    __shared__ int count, work_n, kept_n;

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int r = blockIdx.x, A = a.t.a, kp = a.kp;
    Staged s;
    s.geo    = reinterpret_cast<double*>(keys + kKeys);
    s.centre = reinterpret_cast<float*>(s.geo + kGeo * kp);
    s.label  = reinterpret_cast<int*>(s.centre + 2 * kp);
    s.kp     = kp;
    unsigned* work = reinterpret_cast<unsigned*>(s.label + kp);
    int*      kept_list = reinterpret_cast<int*>(work + kWork);
    const unsigned long long* src = a.keys + (size_t)r * A;

    // ---- the a.keep largest keys of the image (boxes_images_kernel's)
    if (tid == 0) { count = 0; work_n = 0; kept_n = 0; }
    const int trip = kKeys - a.keep;                                            // (>= a.keep, >= kImageBlock)
    unsigned long long floor = 0ull;
    int mine = 0;
    for (int base = 0; base < A; base += trip) {                                // (the same trips in every thread)
        __syncthreads();
        const int fill = count;
        __syncthreads();                                                        // (nobody adds before everybody has read the fill)
        if (fill + trip > kKeys) floor = keep_cut<kImageBlock>(keys, &count, kKeys, a.keep, floor);
        const int end = min(A, base + trip);
        for (int j = base + tid; j < end; j += kImageBlock) {
            const unsigned long long key = src[j];
            mine += key != 0ull;
            if (key > floor) keep_add(keys, &count, kKeys, key);
        }
    }
    __syncthreads();
    floor = keep_cut<kImageBlock>(keys, &count, kKeys, a.keep, floor);
    const int cnt = min(count, a.keep);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, kWave);
    if (lane == 0) wave_sum[wave] = mine;

    // ---- lane p stages sorted candidate p
    if (tid < cnt) {
        const int anchor = (int)(kIndexTop - (unsigned)keys[tid]);
        const int k = a.winners[(size_t)r * A + anchor];
        const Anchor v = anchor_numbers<true>(a.t, a.g.objectness, r, anchor, k);
        double c, sn;
        rule_cos_sin(v.angle, c, sn);
        const double cx = (double)v.b0, cy = (double)v.b1, w = (double)v.b2, h = (double)v.b3;
        const double ux = (w * 0.5) * c, uy = (w * 0.5) * sn, vx = -((h * 0.5) * sn), vy = (h * 0.5) * c;
        s.geo[0 * kp + tid] = (cx - ux) - vx;  s.geo[1 * kp + tid] = (cy - uy) - vy;
        s.geo[2 * kp + tid] = (cx + ux) - vx;  s.geo[3 * kp + tid] = (cy + uy) - vy;
        s.geo[4 * kp + tid] = (cx + ux) + vx;  s.geo[5 * kp + tid] = (cy + uy) + vy;
        s.geo[6 * kp + tid] = (cx - ux) + vx;  s.geo[7 * kp + tid] = (cy - uy) + vy;
        s.geo[8 * kp + tid] = w * h;
        s.geo[9 * kp + tid] = w + h;
        s.centre[tid] = v.b0;
        s.centre[kp + tid] = v.b1;
        s.label[tid] = k;
    }
    __syncthreads();
    int selected = 0;
#pragma unroll
    for (int i = 0; i < kImageWaves; ++i) selected += wave_sum[i];

    // ---- greedy suppression by pull, a chunk of 64 places at a time
    for (int c = 0; c * kWave < cnt; ++c) {
        const int nk = kept_n;                                                  // (behind a barrier: uniform)
        if (nk >= a.per_image) break;
        const int first = c * kWave;
        if (tid == 0) dead = 0ull;
        if (tid < kWave) row[tid] = 0ull;
        __syncthreads();
        run_pairs(kWave * nk, work, &work_n, s, a,
                  [&](int t, int& i, int& j) {
                      i = first + (t & (kWave - 1));
                      j = kept_list[t >> 6];
                      return i < cnt && !((dead >> (t & (kWave - 1))) & 1ull);
                  },
                  [&](int i, int) { atomicOr(&dead, 1ull << (i - first)); });
        const unsigned long long gone = dead;                                   // (run_pairs ends with a barrier)
        run_pairs(kWave * kWave, work, &work_n, s, a,
                  [&](int t, int& i, int& j) {
                      const int ii = t & (kWave - 1), jj = t >> 6;
                      i = first + ii;
                      j = first + jj;
                      return jj < ii && i < cnt && !(((gone >> ii) | (gone >> jj)) & 1ull);
                  },
                  [&](int i, int j) { atomicOr(&row[i - first], 1ull << (j - first)); });
        if (wave == (c & (kImageWaves - 1))) {                                  // the chunk's wave: the serial chain, bits only
            const int live = min(kWave, cnt - first);
            const unsigned long long valid = (live == kWave ? ~0ull : (1ull << live) - 1ull) & ~gone;
            unsigned long long kept = 0ull;
            for (int i = 0; i < kWave; ++i)
                if (((valid >> i) & 1ull) && !(row[i] & kept)) kept |= 1ull << i;
            if ((kept >> lane) & 1ull) kept_list[nk + __popcll(kept & ((1ull << lane) - 1ull))] = first + lane;
            if (lane == 0) kept_n = nk + __popcll(kept);
        }
        __syncthreads();
    }
    __syncthreads();

    // ---- rows, counts: lane q writes kept place q
    const int rows = min(kept_n, a.per_image);
    if (tid < rows) {
        const int p = kept_list[tid];
        const int anchor = (int)(kIndexTop - (unsigned)keys[p]);
        const int k = s.label[p];
        const Anchor v = anchor_numbers<true>(a.t, a.g.objectness, r, anchor, k);
        const float score = a.g.objectness ? v.obj * v.cls : v.cls;
        float q[8];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            q[2 * f]     = (float)to_frame(s.g(2 * f, p), a.dx, a.frame_w, a.iw);
            q[2 * f + 1] = (float)to_frame(s.g(2 * f + 1, p), a.dy, a.frame_h, a.ih);
        }
        int4* out = a.staging + kPieces * ((size_t)r * a.per_image + tid);
        out[0] = make_int4(r, k, (int)__float_as_uint(score), (int)((unsigned)r * (unsigned)A + (unsigned)anchor));
        out[1] = make_int4(__float_as_int(v.b0), __float_as_int(v.b1), __float_as_int(v.b2), __float_as_int(v.b3));
        out[2] = make_int4(__float_as_int(v.angle), __float_as_int(q[0]), __float_as_int(q[1]), __float_as_int(q[2]));
        out[3] = make_int4(__float_as_int(q[3]), __float_as_int(q[4]), __float_as_int(q[5]), __float_as_int(q[6]));
        out[4] = make_int4(__float_as_int(q[7]), 0, 0, 0);
    }
    if (tid == 0) {
        a.header[r]         = rows;
        a.header[a.t.n + r] = selected;
    }
}

}  // namespace

extern "C" {

int pvhip_oriented_boxes_f32(const float* x, int n, int a, int c, int layout, int objectness, float min_score, const int* labels,
                             int num_labels, int frame_h, int frame_w, int dx, int dy, int iw, int ih, int min_h, int min_w,
                             int max_candidates, int overlap, float threshold, int per_label, int max_per_image, void* scratch, int* header,
                             int* rows) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(x != nullptr && scratch != nullptr && header != nullptr && rows != nullptr);
    PVHIP_CHECK_ARG(((uintptr_t)x & 3u) == 0 && ((uintptr_t)header & 3u) == 0 && ((uintptr_t)labels & 3u) == 0);
    PVHIP_CHECK_ARG(((uintptr_t)rows & 15u) == 0 && ((uintptr_t)scratch & 15u) == 0);
    PVHIP_CHECK_ARG(n >= 1 && a >= 1 && c >= 1);
    PVHIP_CHECK_ARG(objectness == 0 || objectness == 1);
    PVHIP_CHECK_ARG((long long)n * a * (5LL + objectness + c) < (1LL << 31));
    const int e = 4 + objectness + c;
    const int form = boxes_form(layout, a, e);                                  // (of the length the class walk reads)
    PVHIP_CHECK_ARG(form != PVHIP_BOXES_FORM_NONE);                              // layout one of the two
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

    const Head         t{reinterpret_cast<const unsigned*>(x), n, a, c, e, layout, e + 1};
    const OrientedRule g{labels, num_labels, objectness, min_score, (float)min_h, (float)min_w};
    const size_t anchors = (size_t)n * (size_t)a;
    char* const  base    = static_cast<char*>(scratch);
    unsigned long long* keys    = reinterpret_cast<unsigned long long*>(base);
    int*                winners = reinterpret_cast<int*>(base + 8 * anchors);
    int4*               staging = reinterpret_cast<int4*>(base + ((12 * anchors + 15u) & ~(size_t)15u));

    const int kp = (max_candidates + kWave - 1) / kWave * kWave;
    const ImageArgs im{t, g, keys, winners, staging, header, max_candidates, kp, max_per_image, overlap, per_label,
                       frame_h, frame_w, dx, dy, iw, ih, threshold};
    static bool attr_set = false;                                               // once, for the largest buffer: no runtime call per pass
    if (!attr_set) {
        PVHIP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&oriented_images_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)image_lds_bytes(kMaxCand)));
        attr_set = true;
    }

    launch_score(form, t, g, keys, winners, state().stream);
    PVHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(oriented_images_kernel, dim3((unsigned)n), dim3(kImageBlock), image_lds_bytes(kp), state().stream, im);
    PVHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(boxes_write_kernel<kPieces>, dim3((unsigned)((n + kImagesPerBlock - 1) / kImagesPerBlock)), dim3(kBlock), 0,
                       state().stream, staging, n, max_per_image, header, reinterpret_cast<int4*>(rows));
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
