// Keep the largest: the bounded buffer of 64-bit keys in LDS that pvhip_maxima.hip (both launches) and pvhip_boxes.hip (the images launch)
// find the best `keep` keys of a long run with.  Keys above the floor are appended through an LDS counter; before a trip could overflow
// the buffer it is sorted descending (the bitonic pattern of tiles_frames_kernel, over the next power of two of its fill: `cap` is a power
// of two) and cut to `keep`, and the keep-th key becomes the floor.  The keys are distinct and the sort is total, so the order in which
// lanes add them does not show in the result.
#pragma once
#include "pvhip_common.h"

namespace pvhip {

// ---- keep the largest: a buffer `keys` of `cap` keys in LDS, its fill `*count`
__device__ __forceinline__ void keep_add(unsigned long long* keys, int* count, int cap, unsigned long long key) {
    const int slot = atomicAdd(count, 1);                       // (LDS)
    if (slot < cap) keys[slot] = key;                           // (always: the callers cut before a trip could overflow)
}

// Sorts the buffer descending and cuts it to `keep`: the new floor.  Every thread of the team calls it, behind a barrier that follows the
// last keep_add; it ends with a barrier.
template <int TEAM>
__device__ __forceinline__ unsigned long long keep_cut(unsigned long long* keys, int* count, int cap, int keep, unsigned long long floor) {
    const int tid = threadIdx.x;
    const int n = min(*count, cap);                             // (*count itself: see keep_add)
    if (n > 1) {
        int sort_n = 2;
        while (sort_n < n) sort_n <<= 1;
        for (int i = n + tid; i < sort_n; i += TEAM) keys[i] = 0ull;
        __syncthreads();
        for (int k = 2; k <= sort_n; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < (sort_n >> 1); i += TEAM) {
                    const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                    const unsigned long long u = keys[lo], v = keys[hi];
                    if (((lo & k) == 0) ? (u < v) : (u > v)) {
                        keys[lo] = v;
                        keys[hi] = u;
                    }
                }
                __syncthreads();
            }
        }
    }
    if (n >= keep) floor = keys[keep - 1];
    if (tid == 0 && n > keep) *count = keep;
    __syncthreads();
    return floor;
}

}  // namespace pvhip
