// The position rule of the answers that sample a Result bilinearly at the centres of frame pixels, straight through the letterbox
// geometry (include/pvhip.h: rule 2 of pvhip_frame_masks_f32, rule 1 of pvhip_segment_frame_labels_f32), stated once for the kernels
// that answer by it (pvhip_frame_masks.hip, pvhip_segments_frame.hip).
//   position  for frame position X of one axis, in exact integers: N = (2 d F + (2 X + 1) i) P - F N_net and D = 2 F N_net;
//             p = floor(65536 N / D), floor toward minus infinity; the taps p >> 16 and (p >> 16) + 1 clamped to [0, P - 1], the
//             fraction (p & 65535) / 65536.
//   packed    one 32-bit word per position for LDS: the first tap relative to a window's first, the second the same or the next, the
//             Q16 fraction.
#pragma once
#include "pvhip_common.h"

namespace pvhip {

// One axis of the rule: N(X) = c0 + X * step over den, all exact integers below 2^43, so that 65536 N stays below 2^59.
struct Axis {
    long long c0, step, den;
    int ext;                                    // the extent the taps clamp to
};
__host__ __device__ __forceinline__ Axis axis_of(int d, int i, int F, int P, int N) {
    return Axis{(2LL * d * F + i) * P - (long long)F * N, 2LL * i * P, 2LL * F * N, P};
}
struct Tap {
    int a, b;                                   // the clamped taps
    unsigned f;                                 // the Q16 fraction
};
__device__ __forceinline__ Tap tap_of(const Axis& ax, int X) {
    const long long num = (ax.c0 + (long long)X * ax.step) * 65536LL;
    long long p = num / ax.den;
    if (num % ax.den < 0) --p;                  // floor toward minus infinity
    const long long x0 = p >> 16, last = ax.ext - 1;
    return Tap{(int)min(max(x0, 0LL), last), (int)min(max(x0 + 1, 0LL), last), (unsigned)(p & 65535)};
}
__device__ __forceinline__ unsigned packed(const Tap& t, int first) { return (unsigned)(t.a - first) | ((unsigned)(t.b - t.a) << 15) | (t.f << 16); }

}  // namespace pvhip
