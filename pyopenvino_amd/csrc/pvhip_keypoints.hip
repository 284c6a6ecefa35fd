// The peak of every plane of a stack of heatmaps (n, K, H, W), on the device: what users of landmark, pose and corner heads do on the host
// with an argmax per plane after reading the whole tensor back.  include/pvhip.h states the rule (pvhip_heatmap_peaks_f32),
// pyopenvino_amd/keypoints.py and tests/keypoints_ref.py are the same in numpy and in plain loops.
//
// A streaming reduction: every plane is read once, 16 bytes per lane and load, and nothing but 16 bytes per plane is written.
//   key     (pvhip_topk_keys.h) every element becomes the 64-bit key of top_k's total order; all keys of a plane are distinct and
//           nonzero and the peak is the plane's largest key.  A key carries its index, so any lane may hold any element.
//   loads   a plane starts wherever n, K and H * W put it: it is split at its 16-byte boundaries into a head of 0-3 elements, a body of
//           16-byte pieces and a tail of 0-3 elements (threads 0-5 of the plane's team load head and tail one element each).
//   forms   planes of up to kWavePlane elements: one wave per plane, four planes per workgroup, no LDS, no barrier (a 26 x 26 plane is
//           169 pieces: three loads per lane).  Larger planes: one workgroup per plane, the four waves' winners combined through LDS.
//           pvhip_heatmap_peaks_form names the choice.
//   finish  one lane per plane reads the peak's own bits and, under PVHIP_PEAKS_QUARTER, its at most four neighbours again (they hit in
//           L2: the plane has just gone through it), applies valid / refine / space and writes the answer.
// Planes are walked by a grid-stride loop, so that n * K up to 2^31 - 1 needs no grid of that size.
#include "pvhip_common.h"
#include "pvhip_point_rule.h"
#include "pvhip_topk_keys.h"

using namespace pvhip;

namespace {

constexpr int      kWavePlane = 1024;          // H * W at most for the wave form: 4 pieces of 16 bytes per lane
constexpr int      kWaves     = kBlock / kWave;

struct PeakRule {
    int   h, w, refine, space, has_min;
    float min_score;
};

__device__ __forceinline__ void take(unsigned long long& best, unsigned long long key) { best = key > best ? key : best; }

// The largest key among elements first, first + team, ... of the plane's pieces and (threads 0-5 of the team) its head and tail.
__device__ __forceinline__ unsigned long long plane_scan(const unsigned* __restrict__ plane, int size, int first, int team) {
    const int head = min(size, (int)(((16u - (unsigned)((uintptr_t)plane & 15u)) & 15u) >> 2));
    const int npiece = (size - head) >> 2, tail = (size - head) & 3;
    const uint4* body = reinterpret_cast<const uint4*>(plane + head);
    unsigned long long best = 0ull;
    if (first < head + tail) {
        const int edge = first < head ? first : head + 4 * npiece + (first - head);
        best = topk_key(plane[edge], (unsigned)edge);
    }
#pragma unroll 4
    for (int p = first; p < npiece; p += team) {
        const uint4    q  = body[p];
        const unsigned at = (unsigned)(head + 4 * p);
        take(best, topk_key(q.x, at + 0u));
        take(best, topk_key(q.y, at + 1u));
        take(best, topk_key(q.z, at + 2u));
        take(best, topk_key(q.w, at + 3u));
    }
    return best;
}

// Rules 2-4 for the plane whose largest key is `key`; one lane.
__device__ __forceinline__ void plane_finish(const float* __restrict__ plane, unsigned long long key, const PeakRule& rule, size_t at,
                                             int* __restrict__ positions, unsigned* __restrict__ scores, unsigned* __restrict__ points) {
    const int      p    = (int)(kIndexTop - (unsigned)key);
    const unsigned bits = reinterpret_cast<const unsigned*>(plane)[p];
    const float    v    = __uint_as_float(bits);
    const bool     nan  = (bits & 0x7FFFFFFFu) > 0x7F800000u;
    const bool     valid = !nan && (!rule.has_min || v >= rule.min_score);
    unsigned ux = kQuietNaN, uy = kQuietNaN;
    if (valid) point_of(plane, p, rule.h, rule.w, rule.refine, rule.space, ux, uy);       // rules 3 and 4: pvhip_point_rule.h
    positions[at]      = p;
    scores[at]         = bits;                                                  // the plane's own bits
    points[2 * at]     = ux;
    points[2 * at + 1] = uy;
}

// One wave per plane.
__global__ __launch_bounds__(kBlock) void peaks_wave_kernel(const float* __restrict__ x, long long planes, PeakRule rule,
                                                            int* __restrict__ positions, unsigned* __restrict__ scores,
                                                            unsigned* __restrict__ points) {
    const int lane = threadIdx.x & (kWave - 1);
    const int size = rule.h * rule.w;
    const long long stride = (long long)gridDim.x * kWaves;
    for (long long i = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); i < planes; i += stride) {      // (the whole wave: no barrier)
        const float* plane = x + (size_t)i * (size_t)size;
        const unsigned long long best = wave_max_u64(plane_scan(reinterpret_cast<const unsigned*>(plane), size, lane, kWave));
        if (lane == 0) plane_finish(plane, best, rule, (size_t)i, positions, scores, points);
    }
}

// One workgroup per plane.
__global__ __launch_bounds__(kBlock) void peaks_block_kernel(const float* __restrict__ x, long long planes, PeakRule rule,
                                                             int* __restrict__ positions, unsigned* __restrict__ scores,
                                                             unsigned* __restrict__ points) {
    __shared__ unsigned long long winners[kWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int size = rule.h * rule.w;
    for (long long i = blockIdx.x; i < planes; i += gridDim.x) {                // (the same trip count in every thread of the workgroup)
        const float* plane = x + (size_t)i * (size_t)size;
        const unsigned long long best = wave_max_u64(plane_scan(reinterpret_cast<const unsigned*>(plane), size, (int)threadIdx.x, kBlock));
        if (lane == 0) winners[wave] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long all = winners[0];
#pragma unroll
            for (int j = 1; j < kWaves; ++j) take(all, winners[j]);
            plane_finish(plane, all, rule, (size_t)i, positions, scores, points);
        }
        __syncthreads();                                                        // winners[] is written again in the next trip
    }
}

int peaks_form(int h, int w) {
    if (h < 1 || w < 1) return PVHIP_PEAKS_FORM_NONE;
    const long long size = (long long)h * w;
    if (size < 2 || size > PVHIP_PEAKS_MAX_PLANE) return PVHIP_PEAKS_FORM_NONE;
    return size <= kWavePlane ? PVHIP_PEAKS_FORM_WAVE : PVHIP_PEAKS_FORM_BLOCK;
}

}  // namespace

extern "C" {

int pvhip_heatmap_peaks_form(int h, int w) { return peaks_form(h, w); }

int pvhip_heatmap_peaks_f32(const float* x, int n, int k, int h, int w, int refine, int space, int has_min, float min_score,
                            int* positions, float* scores, float* points) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(x != nullptr && positions != nullptr && scores != nullptr && points != nullptr);
    PVHIP_CHECK_ARG(((uintptr_t)x & 3u) == 0 && ((uintptr_t)positions & 3u) == 0 && ((uintptr_t)scores & 3u) == 0 && ((uintptr_t)points & 3u) == 0);
    PVHIP_CHECK_ARG(n >= 1 && k >= 1 && h >= 1 && w >= 1);
    const int form = peaks_form(h, w);
    PVHIP_CHECK_ARG(form != PVHIP_PEAKS_FORM_NONE);                              // 2 <= h * w <= 2^24
    PVHIP_CHECK_ARG((long long)n * k < (1LL << 31));
    PVHIP_CHECK_ARG(refine == PVHIP_PEAKS_NONE || refine == PVHIP_PEAKS_QUARTER);
    PVHIP_CHECK_ARG(space == PVHIP_PEAKS_HEATMAP || space == PVHIP_PEAKS_NORMALISED);
    PVHIP_CHECK_ARG(has_min == 0 || has_min == 1);
    PVHIP_CHECK_ARG(min_score - min_score == 0.0f);                              // finite
    const long long planes = (long long)n * k;
    const PeakRule  rule{h, w, refine, space, has_min, min_score};
    unsigned* score_bits = reinterpret_cast<unsigned*>(scores);
    unsigned* point_bits = reinterpret_cast<unsigned*>(points);
    if (form == PVHIP_PEAKS_FORM_WAVE) {
        const long long want = (planes + kWaves - 1) / kWaves;
        const dim3 grid((unsigned)(want < kMaxBlocks * 4 ? want : kMaxBlocks * 4));
        hipLaunchKernelGGL(peaks_wave_kernel, grid, dim3(kBlock), 0, state().stream, x, planes, rule, positions, score_bits, point_bits);
    } else {
        const dim3 grid((unsigned)(planes < kMaxBlocks * 16 ? planes : kMaxBlocks * 16));
        hipLaunchKernelGGL(peaks_block_kernel, grid, dim3(kBlock), 0, state().stream, x, planes, rule, positions, score_bits, point_bits);
    }
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
