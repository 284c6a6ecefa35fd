// The 64-bit keys and the selection rounds of the total order of pvhip_topk_rows_f32 (include/pvhip.h), shared by the kernels that
// answer in that order (pvhip_topk.hip, pvhip_gallery.hip).
//   key     high word = the float's bits made order-preserving as an unsigned, -0.0 folded onto +0.0 and every NaN mapped to the maximum;
//           low word = 0x7FFFFFFF - index.  All keys of a row are distinct and nonzero, and the rule's order is the descending order of
//           the keys.
//   rounds  round j takes the maximum of the keys strictly below round j - 1's winner; nothing is mutated.
#pragma once
#include "pvhip_common.h"

namespace pvhip {

constexpr unsigned kIndexTop = 0x7FFFFFFFu;   // low word of the key of index 0 (indices < 2^31): no key is all ones, the bound of round 0

__device__ __forceinline__ unsigned long long topk_key(unsigned bits, unsigned index) {
    const unsigned mag = bits & 0x7FFFFFFFu;
    unsigned ord;
    if (mag > 0x7F800000u) ord = 0xFFFFFFFFu;                                   // NaN, any sign and payload: before every number
    else if (mag == 0u) ord = 0x80000000u;                                      // +0.0 and -0.0 are equal
    else ord = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);             // (+inf: 0xFF800000; -inf: 0x007FFFFF)
    return ((unsigned long long)ord << 32) | (unsigned long long)(kIndexTop - index);
}

// best = max(best, key) among the keys strictly below `below`
__device__ __forceinline__ void topk_take(unsigned long long& best, unsigned long long key, unsigned long long below) {
    best = (key < below && key > best) ? key : best;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m, kWave);
        v = o > v ? o : v;
    }
    return v;
}

}  // namespace pvhip
