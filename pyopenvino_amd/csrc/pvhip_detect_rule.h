// The screen and the rectangle of one live DetectionOutput record: the one place where pvhip_detections_to_rois and
// pvhip_detections_compact (include/pvhip.h states the rule of both) decide whether a record survives and what its rectangle is.
// Whether a record is live -- in front of its image's first row whose column 0 is not >= 0 -- is the caller's business: the
// kernels find the list end in different ways.  walk_image below is the wave-per-image way of pvhip_detections_compact,
// pvhip_detections_merge_tiles and pvhip_detections_merge_regions.
#pragma once

#include "pvhip_common.h"

namespace pvhip {

constexpr int kScreenLabels = 64;   // entries of a label filter

struct DetectionRect {
    int x0, y0, w, h;
};

// The geometry of a fitted detector input (pvhip_input_preprocess_fit_f32): the detector saw the frame in the rectangle
// [dy, dy + ih) x [dx, dx + iw) of its (Hn, Wn) input, so a normalised corner v of its records is u = (v Wn - dx) / iw of the frame (Hn, dy,
// ih for a y): three fp32 roundings, never contracted.
struct DetectionFit {
    int Hn, Wn, dx, dy, iw, ih;
};

__device__ __forceinline__ float unfit(float v, int N, int d, int i) { return (v * (float)N - (float)d) / (float)i; }

// True when the live record q = [rank, label, score, xmin, ymin, xmax, ymax] is selected: score >= conf (false for NaN), four finite
// corners, (when `filtered`) label == (float)labels[j] for some j < num_labels, and a rectangle over (fh, fw) of at least (min_h, min_w),
// which is left in `r`.  `labels` may hold ints (global memory) or the same values as floats (LDS); fp32 throughout, never contracted.
// FIT: the rectangle is that of the corners mapped back through `g` (the finite check is on the record's own corners); a box in the padding
// clamps to the frame's edge, one wholly in it has extent 0 and is dropped.
template <bool FIT = false, typename L>
__device__ __forceinline__ bool detection_screen(const float* __restrict__ q, float conf, const L* labels, bool filtered, int num_labels,
                                                 float fh, float fw, int min_h, int min_w, DetectionRect& r,
                                                 const DetectionFit& g = DetectionFit{}) {
    const float label = q[1], score = q[2];
    float xa = q[3], ya = q[4], xb = q[5], yb = q[6];
    bool keep = score >= conf && isfinite(xa) && isfinite(ya) && isfinite(xb) && isfinite(yb);
    if (FIT) {
        xa = unfit(xa, g.Wn, g.dx, g.iw); xb = unfit(xb, g.Wn, g.dx, g.iw);
        ya = unfit(ya, g.Hn, g.dy, g.ih); yb = unfit(yb, g.Hn, g.dy, g.ih);
    }
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

// What walk_image screens with: the records, P of them per image, and the screen's values.
struct ScreenWalk {
    const float* rec;      // [images * P][7]
    const int*   labels;   // [num_labels], or NULL: any label
    int   P, num_labels, min_h, min_w;
    float conf;
};

// A geometry the _fit entries accept: extents exact as fp32, the rectangle inside the input.
inline bool detection_fit_ok(const DetectionFit& g) {
    return g.Hn >= 1 && g.Hn <= (1 << 24) && g.Wn >= 1 && g.Wn <= (1 << 24) && g.iw >= 1 && g.ih >= 1 && g.dx >= 0 && g.dy >= 0 &&
           g.iw <= g.Wn - g.dx && g.ih <= g.Hn - g.dy;
}

__device__ __forceinline__ int lanes_below(unsigned long long votes) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(votes >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)votes, 0u));
}

// Walks image b over a frame of (H, W), 64 records at a time, and hands every survivor with rank < limit to `emit(rank, record, rectangle,
// q)`.  Returns the number of survivors seen (all of them when limit >= P).  The whole wave calls it; everything that steers the loop is
// wave-uniform.
template <bool FIT = false, typename Emit>
__device__ __forceinline__ int walk_image(const ScreenWalk& a, int b, int H, int W, int limit, Emit emit, const DetectionFit& g = DetectionFit{}) {
    const int   lane = threadIdx.x & (kWave - 1);
    const float fh = (float)H, fw = (float)W;
    int seen = 0;
    for (int p0 = 0; p0 < a.P && seen < limit; p0 += kWave) {
        const int    p     = p0 + lane;
        const bool   valid = p < a.P;
        const int    r     = b * a.P + p;                                       // (images * P < 2^31 / 7: the launchers check)
        const float* q     = a.rec + (size_t)r * 7;
        const unsigned long long ends = __ballot(valid && !(q[0] >= 0.0f));
        const int  first = ends ? __builtin_ctzll(ends) : kWave;               // the list ends at this lane's record
        DetectionRect rect{0, 0, 0, 0};
        const bool keep = valid && lane < first &&
                          detection_screen<FIT>(q, a.conf, a.labels, a.labels != nullptr, a.num_labels, fh, fw, a.min_h, a.min_w, rect, g);
        const unsigned long long votes = __ballot(keep);
        const int rank = seen + lanes_below(votes);
        if (keep && rank < limit) emit(rank, r, rect, q);
        seen += __popcll(votes);
        if (ends) break;
    }
    return seen;
}

// The label word of a table row: (int32) of column 1 when that is finite and in [-2^31, 2^31), else -1.
__device__ __forceinline__ int detection_label(float l) {
    return (l >= -2147483648.0f && l < 2147483648.0f) ? (int)l : -1;           // (NaN and +-inf fail the comparisons)
}

}  // namespace pvhip
