// The k best entries of every row of a classifier's Result, on the device: what the reference's sample does on the host with
// np.argsort(res[output_node_name][0])[::-1] after reading the whole tensor back.  include/pvhip.h states the rule
// (pvhip_topk_rows_f32), tests/topk_ref.py is the same in numpy.
//
// A latency kernel (the Result of a batch of 256 is 1 MB): one wave per row, four rows per workgroup, no LDS, no sorting network.
//   key     (pvhip_topk_keys.h) every element becomes a 64-bit key: high word = its float bits made order-preserving as an unsigned, -0.0 folded onto +0.0
//           and every NaN mapped to the maximum; low word = 0x7FFFFFFF - index.  All keys of a row are distinct and nonzero, and the
//           rule's order is the descending order of the keys.
//   rounds  round j takes the wave-wide maximum of the keys strictly below round j - 1's winner; nothing is mutated.  Lane j keeps
//           winner j, so the (rows, k) outputs are written once, k consecutive lanes per row.
//   loads   a key carries its index, so any lane may hold any element: the row is split at its 16-byte boundaries into a head of 0-3
//           elements, a body of 16-byte pieces and a tail of 0-3 elements (lanes 0-5 load head and tail one element each).  A row of
//           1001 columns, or one that starts one element into a tensor, reads its body in 16-byte loads like an aligned one.
//   rows    of up to 1024 columns are turned into keys once and stay in registers (17 keys per lane); longer rows are read again in
//           every round and hit in L2.
#include "pvhip_common.h"
#include "pvhip_topk_keys.h"

using namespace pvhip;

namespace {

constexpr int      kTopKMax   = 64;            // one winner per lane
constexpr int      kRegPieces = 4;             // 16-byte pieces per lane of a register-resident row: 64 * 4 * 4 = 1024 columns
constexpr int      kRegCols   = kWave * kRegPieces * 4;

template <bool kInRegs>
__global__ __launch_bounds__(kBlock) void topk_rows_kernel(const unsigned* __restrict__ x, int rows, int cols, int k,
                                                           int* __restrict__ indices, unsigned* __restrict__ values) {
    const int lane = threadIdx.x & (kWave - 1);
    const int r    = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (r >= rows) return;                                                      // (the whole wave: nothing below meets a barrier)
    const unsigned* row = x + (size_t)r * cols;
    // head | body of 16-byte pieces | tail
    const int head = min(cols, (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2));
    const int npiece = (cols - head) >> 2, tail = (cols - head) & 3;
    const uint4* body = reinterpret_cast<const uint4*>(row + head);
    const bool has_edge = lane < head + tail;                                   // lanes 0-5: one element of the head or the tail
    const int  edge     = lane < head ? lane : head + 4 * npiece + (lane - head);

    unsigned long long keys[4 * kRegPieces + 1];
    if constexpr (kInRegs) {
        keys[4 * kRegPieces] = has_edge ? topk_key(row[edge], (unsigned)edge) : 0ull;
#pragma unroll
        for (int i = 0; i < kRegPieces; ++i) {
            const int p = lane + kWave * i;
            uint4 q = make_uint4(0u, 0u, 0u, 0u);
            if (p < npiece) q = body[p];
            const unsigned at = (unsigned)(head + 4 * p);
            keys[4 * i + 0] = p < npiece ? topk_key(q.x, at + 0u) : 0ull;
            keys[4 * i + 1] = p < npiece ? topk_key(q.y, at + 1u) : 0ull;
            keys[4 * i + 2] = p < npiece ? topk_key(q.z, at + 2u) : 0ull;
            keys[4 * i + 3] = p < npiece ? topk_key(q.w, at + 3u) : 0ull;
        }
    }
    unsigned long long below = ~0ull, mine = 0ull;
    for (int j = 0; j < k; ++j) {
        unsigned long long best = 0ull;
        if constexpr (kInRegs) {
#pragma unroll
            for (int i = 0; i < 4 * kRegPieces + 1; ++i) topk_take(best, keys[i], below);
        } else {
            if (has_edge) topk_take(best, topk_key(row[edge], (unsigned)edge), below);
#pragma unroll 4
            for (int p = lane; p < npiece; p += kWave) {
                const uint4    q  = body[p];
                const unsigned at = (unsigned)(head + 4 * p);
                topk_take(best, topk_key(q.x, at + 0u), below);
                topk_take(best, topk_key(q.y, at + 1u), below);
                topk_take(best, topk_key(q.z, at + 2u), below);
                topk_take(best, topk_key(q.w, at + 3u), below);
            }
        }
        best = wave_max_u64(best);
        if (lane == j) mine = best;
        below = best;
    }
    if (lane < k && mine != 0ull) {                                             // (k <= cols: every round has a winner)
        const unsigned index = kIndexTop - (unsigned)mine;
        indices[(size_t)r * k + lane] = (int)index;
        values[(size_t)r * k + lane]  = row[index];                             // the element's own bits
    }
}

}  // namespace

extern "C" {

int pvhip_topk_rows_f32(const float* x, int rows, int cols, int k, int* indices, float* values) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(x != nullptr && indices != nullptr && values != nullptr);
    PVHIP_CHECK_ARG(((uintptr_t)x & 3u) == 0 && ((uintptr_t)indices & 3u) == 0 && ((uintptr_t)values & 3u) == 0);
    PVHIP_CHECK_ARG(rows >= 1 && cols >= 1);
    PVHIP_CHECK_ARG(k >= 1 && k <= cols && k <= kTopKMax);
    PVHIP_CHECK_ARG((long long)rows * cols < (1LL << 31));
    const unsigned* bits = reinterpret_cast<const unsigned*>(x);
    unsigned*       out  = reinterpret_cast<unsigned*>(values);
    const dim3 grid((rows + kBlock / kWave - 1) / (kBlock / kWave));
    if (cols <= kRegCols)
        hipLaunchKernelGGL(topk_rows_kernel<true>, grid, dim3(kBlock), 0, state().stream, bits, rows, cols, k, indices, out);
    else
        hipLaunchKernelGGL(topk_rows_kernel<false>, grid, dim3(kBlock), 0, state().stream, bits, rows, cols, k, indices, out);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
