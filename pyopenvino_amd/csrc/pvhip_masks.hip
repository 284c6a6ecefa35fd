// Instance masks on the device: the T mask coefficients in the tail of a dense head's kept anchors times the T prototype planes of a
// second tensor, thresholded and cropped to the box -- what a user of a YOLOv8-seg / YOLOv5-seg / YOLACT export makes on the host with
// `sigmoid(coefficients @ prototypes) > 0.5` after reading both tensors back.  include/pvhip.h states the rule
// (pvhip_instance_masks_f32), pyopenvino_amd/masks.py and tests/masks_ref.py are the same in numpy and in plain loops.
//
// One launch behind pvhip_dense_boxes_tail_f32 on the same stream; it reads that call's header and rows on the device.
//   split     grid (pixel pieces, images).  A workgroup of four waves owns kGroups * 4 groups of 32 consecutive flat pixels of one image;
//             a wave owns kGroups = 4 of them, which are 128 pixels and four consecutive output words of every detection.
//   operands  the prototypes are the B operand of v_mfma_f32_32x32x2_f32: lane (h << 5) | j holds p[2 s + h][q0 + j] for step s, so a half
//             wave's load is 128 contiguous bytes of a plane at whatever 4-byte phase it stands.  A wave loads its PAIRS x kGroups B
//             registers ONCE and keeps them across all the image's detections: the prototypes are read from HBM once per image.  PAIRS is
//             T / 2 rounded up to 4, 8, 16 or 32 (a template argument, so that the registers are indexed statically); the pairs behind T
//             are zeros on both sides, and fmaf(0, 0, acc) changes at most the sign of a zero, which `acc > 0` does not see.
//             kGroups = 4: at T = 64 the B registers are 32 x 4 = 128, the four accumulator tiles 64, and with the addresses a wave stays
//             under 256 registers, so two waves share a SIMD and one's ballots and stores run under the other's matrix steps.  Eight
//             groups would take the whole file and leave the stores exposed; two would halve the pixels a staged coefficient serves.
//   staging   the workgroup stages the image's detections a chunk of kStage = 128 at a time: their coefficients, gathered by `records`
//             from the head, in A-operand order (lane (h << 5) | i of step s of block b holds m[32 b + i][2 s + h], as the gallery
//             kernel stages its query block), and beside them each detection's integer crop window [cx0, cx1) x [cy0, cy1), made once
//             by the binary64 comparisons of the rule.  A void detection (a coefficient that is not finite) gets zeros and the empty
//             window; without crop the window is the whole plane.  Rows behind the chunk's count are zeros with the empty window.
//   chains    one accumulator tile per (detection block, pixel group): the f32-input MFMA is bit for bit a k-ordered fmaf chain
//             (pvhip_gallery.hip), so the tile is the rule's L.  The four groups' tiles advance side by side on one A register per step.
//   packing   tile register e of lane (h << 5) | j is detection (e & 3) + 8 (e >> 2) + 4 h, pixel j: the predicate `acc > 0`, inside the
//             window, pixel not void, goes through one wave-wide ballot whose low and high words are the finished words of two
//             detections.  Lane j < 4 of each half keeps group j's word and stores it: 16 contiguous bytes per detection and register.
//             Every word of every row below total is written exactly once; rows from total on are not written.  No atomics.
//   void      a pixel with a prototype value that is not finite: the OR over the two lane halves that hold its k values, by a ballot when
//             the registers are loaded.  Its B values become zeros, so nothing rests on what the matrix instruction does with them.
#include "pvhip_common.h"

using namespace pvhip;

namespace {

constexpr int kGroups   = PVHIP_MASKS_GROUPS;   // pixel groups of 32 a wave keeps in registers
constexpr int kWaves    = kBlock / kWave;
constexpr int kStage    = PVHIP_MASKS_STAGE;    // detections staged at a time
constexpr int kMaxTail  = 64;
constexpr int kMaxExtent = 1 << 24;
constexpr int kMaxPerImage = 4096;              // PVHIP_BOXES_MAX_CANDIDATES
constexpr long long kMaxWords = 1LL << 26;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct MaskArgs {
    const float* head;      // (n, e, a) or (n, a, e)
    const float* protos;    // (n, tail, hp, wp)
    const int*   header;    // counts[n], selected[n], total
    const int*   rows;      // [total][8]; word 7: r * a + anchor
    unsigned*    words;     // [total][w32]
    int n, a, e, planes, tail_at, tail, box, hp, wp, hn, wn, crop, per_image, hw, w32;
};

__device__ __forceinline__ bool not_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u; }

// The smallest p in 0 .. limit with (double)p * n >= (double)v * ext, both products exact: the first pixel at or beyond the corner v.
__device__ __forceinline__ int first_at(float v, int ext, int n, int limit) {
    const double d = (double)v * (double)ext, dn = (double)n;
    if (!(d > 0.0)) return 0;
    const double g = d / dn;
    int p = g < (double)limit ? (int)ceil(g) : limit;
    while (p > 0 && (double)(p - 1) * dn >= d) --p;                             // (the quotient is rounded: a step at most)
    while (p < limit && (double)p * dn < d) ++p;
    return p;
}

template <int PAIRS>
__global__ __launch_bounds__(kBlock, 2) void instance_masks_kernel(MaskArgs k) {
    __shared__ __attribute__((aligned(16))) float coef[kStage / 32][PAIRS][kWave];      // A-operand order
    __shared__ int4 window[kStage];                                                     // cx0, cx1, cy0, cy1
    __shared__ int  bad[kStage];

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, j = lane & 31;
    const int r = blockIdx.y;
    const int T = k.tail;

    // rows of the images in front, this image's count (clamped to what the rows hold: the words behind stay in bounds whatever the header says)
    int base = 0;
    for (int i = lane; i < r; i += kWave) base += min(max(k.header[i], 0), k.per_image);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) base += __shfl_xor(base, d, kWave);
    const int count = min(max(k.header[r], 0), k.per_image);
    if (count == 0) return;                                                     // (the whole workgroup, before any barrier)

    // ---- this wave's B registers: kGroups groups of 32 pixels from q0 on
    const int  word0  = (blockIdx.x * kWaves + wave) * kGroups;                 // the first of this wave's kGroups output words
    const bool active = word0 < k.w32;                                          // (wave-uniform)
    float b[kGroups][PAIRS];
    int   px[kGroups], py[kGroups];
    bool  ok[kGroups];
    const float* planes = k.protos + (size_t)r * T * (size_t)k.hw;
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
        const int  q    = (word0 + g) * 32 + j;
        const bool real = active && q < k.hw;
        bool nf = false;
#pragma unroll
        for (int s = 0; s < PAIRS; ++s) {
            const int t = 2 * s + h;
            b[g][s] = (real && t < T) ? planes[(size_t)t * k.hw + q] : 0.0f;
            nf |= not_finite(b[g][s]);
        }
        const unsigned long long m = __ballot(nf);
        const bool void_pixel = (((m | (m >> 32)) >> j) & 1ull) != 0ull;        // either half's k values
        if (void_pixel) {
#pragma unroll
            for (int s = 0; s < PAIRS; ++s) b[g][s] = 0.0f;
        }
        ok[g] = real && !void_pixel;
        py[g] = real ? q / k.wp : 0;
        px[g] = real ? q - py[g] * k.wp : 0;
    }

    for (int c0 = 0; c0 < count; c0 += kStage) {                                // (the same trips in every thread)
        const int cnt = min(kStage, count - c0);
        __syncthreads();                                                        // the chunk before is done with
        if (tid < kStage) bad[tid] = 0;
        __syncthreads();
        // ---- the chunk's coefficients, gathered by record
        for (int idx = tid; idx < kStage * 2 * PAIRS; idx += kBlock) {
            const int d = idx / (2 * PAIRS), t = idx - d * (2 * PAIRS);
            float v = 0.0f;
            if (d < cnt && t < T) {
                const int anchor = min(max(k.rows[8 * (size_t)(base + c0 + d) + 7] - r * k.a, 0), k.a - 1);
                const int ch = k.tail_at + t;
                v = k.planes ? k.head[((size_t)r * k.e + ch) * (size_t)k.a + anchor] : k.head[((size_t)r * k.a + anchor) * (size_t)k.e + ch];
                if (not_finite(v)) bad[d] = 1;                                  // (every writer writes 1)
            }
            coef[d >> 5][t >> 1][((t & 1) << 5) | (d & 31)] = v;
        }
        __syncthreads();
        // ---- a void detection's coefficients become zeros; every detection's window
        for (int idx = tid; idx < kStage * 2 * PAIRS; idx += kBlock) {
            const int d = idx / (2 * PAIRS), t = idx - d * (2 * PAIRS);
            if (bad[d]) coef[d >> 5][t >> 1][((t & 1) << 5) | (d & 31)] = 0.0f;
        }
        if (tid < kStage) {
            int4 w = make_int4(0, 0, 0, 0);
            if (tid < cnt && !bad[tid]) {
                w = make_int4(0, k.wp, 0, k.hp);
                if (k.crop) {
                    const int anchor = min(max(k.rows[8 * (size_t)(base + c0 + tid) + 7] - r * k.a, 0), k.a - 1);
                    const size_t step = k.planes ? (size_t)k.a : (size_t)1;
                    const float* at = k.head + (k.planes ? (size_t)r * k.e * (size_t)k.a + anchor : ((size_t)r * k.a + anchor) * (size_t)k.e);
                    const float b0 = at[0], b1 = at[step], b2 = at[2 * step], b3 = at[3 * step];
                    float xa = b0, ya = b1, xb = b2, yb = b3;
                    if (k.box == PVHIP_BOXES_CXCYWH) {
                        const float hw = b2 * 0.5f, hh = b3 * 0.5f;
                        xa = b0 - hw; xb = b0 + hw;
                        ya = b1 - hh; yb = b1 + hh;
                    }
                    if (xa != xa || xb != xb || ya != ya || yb != yb) w = make_int4(0, 0, 0, 0);     // (no comparison with a NaN holds)
                    else w = make_int4(first_at(xa, k.wp, k.wn, k.wp), first_at(xb, k.wp, k.wn, k.wp),
                                       first_at(ya, k.hp, k.hn, k.hp), first_at(yb, k.hp, k.hn, k.hp));
                }
            }
            window[tid] = w;
        }
        __syncthreads();
        if (!active) continue;                                                  // (the whole wave; it still meets the barriers above)

        for (int blk = 0; blk * 32 < cnt; ++blk) {
            f32x16 acc[kGroups];
#pragma unroll
            for (int g = 0; g < kGroups; ++g)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[g][e] = 0.0f;
#pragma unroll
            for (int s = 0; s < PAIRS; ++s) {
                const float a = coef[blk][s][lane];
#pragma unroll
                for (int g = 0; g < kGroups; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[g][s], acc[g], 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int  d = blk * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;       // this half's detection of register e
                const int4 w = window[d];
                unsigned mine = 0u;
#pragma unroll
                for (int g = 0; g < kGroups; ++g) {
                    const bool on = acc[g][e] > 0.0f && ok[g] && px[g] >= w.x && px[g] < w.y && py[g] >= w.z && py[g] < w.w;
                    const unsigned long long m = __ballot(on);
                    const unsigned v = h ? (unsigned)(m >> 32) : (unsigned)m;
                    if (j == g) mine = v;
                }
                if (j < kGroups && d < cnt && word0 + j < k.w32) k.words[(size_t)(base + c0 + d) * k.w32 + word0 + j] = mine;
            }
        }
    }
}

}  // namespace

extern "C" {

int pvhip_instance_masks_f32(const float* head, int n, int a, int e, int layout, int tail_at, int tail, int box,
                             const float* protos, int hp, int wp, int hn, int wn, int crop, int max_per_image,
                             const int* header, const int* rows, unsigned* words) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(head != nullptr && protos != nullptr && header != nullptr && rows != nullptr && words != nullptr);
    PVHIP_CHECK_ARG(((uintptr_t)head & 3u) == 0 && ((uintptr_t)protos & 3u) == 0 && ((uintptr_t)header & 3u) == 0 && ((uintptr_t)words & 3u) == 0);
    PVHIP_CHECK_ARG(((uintptr_t)rows & 15u) == 0);
    PVHIP_CHECK_ARG(n >= 1 && a >= 1 && e >= 1 && (long long)n * a * e < (1LL << 31));
    PVHIP_CHECK_ARG(layout == PVHIP_BOXES_LAYOUT_NCA || layout == PVHIP_BOXES_LAYOUT_NAC);
    PVHIP_CHECK_ARG(tail >= 1 && tail <= kMaxTail && tail_at >= 4 && (long long)tail_at + tail <= e);
    PVHIP_CHECK_ARG(box == PVHIP_BOXES_CXCYWH || box == PVHIP_BOXES_XYXY);
    PVHIP_CHECK_ARG(hp >= 1 && wp >= 1 && (long long)hp * wp >= 2 && (long long)hp * wp <= kMaxExtent);
    PVHIP_CHECK_ARG(hn >= 1 && hn <= kMaxExtent && wn >= 1 && wn <= kMaxExtent);
    PVHIP_CHECK_ARG(crop == 0 || crop == 1);
    PVHIP_CHECK_ARG(max_per_image >= 1 && max_per_image <= kMaxPerImage && n <= 65535);
    const int hw = hp * wp, w32 = (hw + 31) / 32;
    PVHIP_CHECK_ARG((long long)n * max_per_image * w32 <= kMaxWords);           // (the last refusal: nothing is done before it)

    const MaskArgs k{head, protos, header, rows, words, n, a, e, layout == PVHIP_BOXES_LAYOUT_NCA ? 1 : 0, tail_at, tail, box,
                     hp, wp, hn, wn, crop, max_per_image, hw, w32};
    const dim3 grid((unsigned)((w32 + kWaves * kGroups - 1) / (kWaves * kGroups)), (unsigned)n);
    if (tail <= 8)       hipLaunchKernelGGL(instance_masks_kernel<4>, grid, dim3(kBlock), 0, state().stream, k);
    else if (tail <= 16) hipLaunchKernelGGL(instance_masks_kernel<8>, grid, dim3(kBlock), 0, state().stream, k);
    else if (tail <= 32) hipLaunchKernelGGL(instance_masks_kernel<16>, grid, dim3(kBlock), 0, state().stream, k);
    else                 hipLaunchKernelGGL(instance_masks_kernel<32>, grid, dim3(kBlock), 0, state().stream, k);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
