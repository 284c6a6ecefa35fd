// The geometry of an aspect-preserving fit (preprocess_info.resize_fit 'LETTERBOX' / 'TOP_LEFT'): the one function that says where a source
// lands in a destination.  The launch that places the pixels (pvhip_preprocess.hip, per workgroup) and the launch that maps a region's
// boxes back (pvhip_tiles.hip, per wave) both call it, so the two cannot drift apart.  Integers only: nothing here rounds as a float.
#pragma once

namespace pvhip {

// The fitted rectangle of a source (or ROI rectangle) of (hs, ws) in a destination of (hd, wd): one scale factor for both axes, the short
// side rounded half up and kept in [1, D]; integers only (include/pvhip.h states the rule, tests/letterbox_ref.py is the same in numpy).
// Extents up to 2^24 each: every product fits an int64.
struct FitRect {
    int dx, dy, iw, ih;
};

__host__ __device__ inline FitRect fit_rect(int hs, int ws, int hd, int wd, int fit) {
    long long iw = wd, ih = hd;
    if ((long long)ws * hd >= (long long)hs * wd) {
        ih = (2LL * hs * wd + ws) / (2LL * ws);
        ih = ih < 1 ? 1 : (ih > hd ? hd : ih);
    } else {
        iw = (2LL * ws * hd + hs) / (2LL * hs);
        iw = iw < 1 ? 1 : (iw > wd ? wd : iw);
    }
    FitRect r;
    r.iw = (int)iw; r.ih = (int)ih;
    r.dx = fit == 1 ? (wd - r.iw) / 2 : 0;
    r.dy = fit == 1 ? (hd - r.ih) / 2 : 0;
    return r;
}

}  // namespace pvhip
