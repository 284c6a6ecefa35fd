// The point rule of the heatmap answers (include/pvhip.h: rules 3 and 4 of pvhip_heatmap_peaks_f32, rule 5 of pvhip_heatmap_maxima_f32),
// shared by pvhip_keypoints.hip and pvhip_maxima.hip so that it exists once: the quarter-pixel refinement toward the larger neighbour on
// each axis, the fp32 sum, and for the normalised space one fp32 addition, one correctly rounded binary64 division and one rounding.
#pragma once
#include "pvhip_common.h"

namespace pvhip {

constexpr unsigned kQuietNaN = 0x7FC00000u;

__device__ __forceinline__ float quarter(float before, float after) {
    return after > before ? 0.25f : (after < before ? -0.25f : 0.0f);           // (equal, zeros of either sign, a NaN: 0)
}

// The point (x, y), as bits, of position p of the plane v[0..h)[0..w): one lane; under PVHIP_PEAKS_QUARTER it reads the at most four
// neighbours of p.
__device__ __forceinline__ void point_of(const float* __restrict__ plane, int p, int h, int w, int refine, int space, unsigned& ux, unsigned& uy) {
    const int py = p / w, px = p - py * w;
    float ox = 0.0f, oy = 0.0f;
    if (refine == PVHIP_PEAKS_QUARTER) {
        if (px >= 1 && px <= w - 2) ox = quarter(plane[p - 1], plane[p + 1]);
        if (py >= 1 && py <= h - 2) oy = quarter(plane[p - w], plane[p + w]);
    }
    float fx = (float)px + ox, fy = (float)py + oy;
    if (space == PVHIP_PEAKS_NORMALISED) {
        fx = (float)((double)(fx + 0.5f) / (double)w);
        fy = (float)((double)(fy + 0.5f) / (double)h);
    }
    ux = __float_as_uint(fx);
    uy = __float_as_uint(fy);
}

}  // namespace pvhip
