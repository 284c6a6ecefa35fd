// The candidate of a greedy suppression and the overlap rule of pvhip_detections_merge_tiles (include/pvhip.h), shared by the kernels that
// suppress by it: tiles_frames_kernel (pvhip_tiles.hip) and boxes_images_kernel (pvhip_boxes.hip).
#pragma once
#include "pvhip_common.h"

namespace pvhip {

// The score's bits as an unsigned that orders like the float, +0.0 and -0.0 equal (no NaN passes the screen); never 0.
__device__ __forceinline__ unsigned ordered_score(unsigned bits) {
    if ((bits & 0x7FFFFFFFu) == 0u) return 0x80000000u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

struct Box {
    int x0, y0, w, h, label;
};

// Candidate i (later in the order) is suppressed by the kept candidate j: the rule's comparison, int64 areas, one float64 product.
__device__ __forceinline__ bool suppresses(const Box& j, const Box& i, int kind, bool per_label, double threshold) {
    if (per_label && i.label != j.label) return false;
    const long long ix0 = i.x0, iy0 = i.y0, ix1 = ix0 + i.w, iy1 = iy0 + i.h;
    const long long jx0 = j.x0, jy0 = j.y0, jx1 = jx0 + j.w, jy1 = jy0 + j.h;
    const long long iw = min(ix1, jx1) - max(ix0, jx0), ih = min(iy1, jy1) - max(iy0, jy0);
    const long long inter = (iw > 0 && ih > 0) ? iw * ih : 0;
    const long long ai = (long long)i.w * i.h, aj = (long long)j.w * j.h;
    const long long den = kind == PVHIP_OVERLAP_IOS ? min(ai, aj) : ai + aj - inter;
    return (double)inter > threshold * (double)den;
}

}  // namespace pvhip
