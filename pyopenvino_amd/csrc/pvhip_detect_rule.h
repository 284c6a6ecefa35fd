// The screen and the rectangle of one live DetectionOutput record: the one place where pvhip_detections_to_rois and
// pvhip_detections_compact (include/pvhip.h states the rule of both) decide whether a record survives and what its rectangle is.
// Whether a record is live -- in front of its image's first row whose column 0 is not >= 0 -- is the caller's business: the two
// kernels find the list end in different ways.
#pragma once

#include "pvhip_common.h"

namespace pvhip {

constexpr int kScreenLabels = 64;   // entries of a label filter

struct DetectionRect {
    int x0, y0, w, h;
};

// True when the live record q = [rank, label, score, xmin, ymin, xmax, ymax] is selected: score >= conf (false for NaN), four finite
// corners, (when `filtered`) label == (float)labels[j] for some j < num_labels, and a rectangle over (fh, fw) of at least (min_h, min_w),
// which is left in `r`.  `labels` may hold ints (global memory) or the same values as floats (LDS); fp32 throughout, never contracted.
template <typename L>
__device__ __forceinline__ bool detection_screen(const float* __restrict__ q, float conf, const L* labels, bool filtered, int num_labels,
                                                 float fh, float fw, int min_h, int min_w, DetectionRect& r) {
    const float label = q[1], score = q[2], xa = q[3], ya = q[4], xb = q[5], yb = q[6];
    bool keep = score >= conf && isfinite(xa) && isfinite(ya) && isfinite(xb) && isfinite(yb);
    if (keep && filtered) {
        bool listed = false;
        for (int j = 0; j < num_labels; ++j) listed = listed || label == (float)labels[j];
        keep = listed;
    }
    if (keep) {
        r.x0 = (int)floorf(fminf(fmaxf(xa * fw, 0.0f), fw));
        r.y0 = (int)floorf(fminf(fmaxf(ya * fh, 0.0f), fh));
        r.w  = (int)ceilf(fminf(fmaxf(xb * fw, 0.0f), fw)) - r.x0;
        r.h  = (int)ceilf(fminf(fmaxf(yb * fh, 0.0f), fh)) - r.y0;
        keep = r.w >= min_w && r.h >= min_h;
    }
    return keep;
}

}  // namespace pvhip
