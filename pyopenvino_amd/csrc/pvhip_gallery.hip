// The k best rows of a gallery of enrolled embeddings for every row of an embedding network's Result, on the device: what its users do
// on the host with `gallery @ x.T` and an argpartition after reading the whole tensor back.  include/pvhip.h states the rule
// (pvhip_gallery_match_f32), pyopenvino_amd/gallery.py and tests/gallery_ref.py are the same in numpy.
//
// Two launches, and no (n, g) score matrix anywhere:
//   scores  a skinny fp32 GEMM that streams the gallery from HBM once per block of 32 query rows.  The gallery is stored in the B-operand
//           order of v_mfma_f32_32x32x2_f32 (one 16-byte load per lane feeds four matrix steps, 1 KB contiguous per wave), the query
//           block sits in LDS in the A-operand order of the same four steps (one ds_read_b128 per lane, conflict-free).  The f32-input
//           MFMA is bit for bit a k-ordered fmaf chain with one rounding per product, and its issue interval equals its dependent
//           latency, so ONE accumulator tile per 32-row gallery block is both the rule's chain and the full matrix rate of the SIMD.
//           A wave owns a chunk of kChunk gallery rows = kTiles tiles, which stay in registers; a ring of kRing 16-byte loads per lane
//           (16 KB per wave) is kept in flight across tile boundaries to cover the HBM latency.
//   top-k   the tiles become the 64-bit keys of pvhip_topk_keys.h (low word: the gallery row).  A tile has its gallery row on the lane
//           and its query rows in the 16 registers x 2 lane halves, so one register index serves two query rows at once, each reduced
//           over its own half wave; round j's winner goes to scratch[row][chunk][j].  Exhausted rounds write key 0 (no key is 0).
//   merge   one wave per query row: the norm of the rule in binary64 (a sequential sum, every lane computes it), the same rounds over the
//           heads of the row's chunk lists (each list is sorted: its candidate is its first key below the last winner), then score,
//           threshold and the leading run.
#include "pvhip_common.h"
#include "pvhip_topk_keys.h"

using namespace pvhip;

namespace {

constexpr int kChunk   = PVHIP_GALLERY_CHUNK;   // gallery rows of one wave: one list of k keys per (query row, chunk)
constexpr int kTiles   = kChunk / 32;           // accumulator tiles a wave keeps: 8 x 16 registers
constexpr int kWaves   = kBlock / kWave;        // chunks per workgroup
constexpr int kRing    = 16;                    // 16-byte loads in flight per lane
constexpr int kMergeLoads = 8;               // list heads (8-byte loads) in flight per lane of the merge
constexpr int kMaxD    = 1024;                  // 32 x 1024 x 4 = 128 KB of the 160 KB of LDS
constexpr int kMaxG    = 1 << 24;
constexpr int kMaxK    = 64;
constexpr unsigned kQuietNaN = 0x7FC00000u;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool not_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u; }

__global__ __launch_bounds__(kBlock) void gallery_scores_kernel(const float* __restrict__ x, int n, int d, int nq,
                                                                const f32x4* __restrict__ packed, int g, int nblocks, int nchunks, int k,
                                                                int nrowblocks, unsigned long long* __restrict__ scratch) {
    extern __shared__ __align__(16) float lds[];
    f32x4* xs  = reinterpret_cast<f32x4*>(lds);                 // [nq][64]: lane (h << 5) | i holds x[row0 + i][8 q + 2 t + h], t = 0..3
    int*   bad = reinterpret_cast<int*>(lds + (size_t)nq * 256); // [32]: the row has an element that is not finite
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Workgroups go to the 8 XCDs round-robin by their number, and each XCD has an L2 of its own: XCD c takes a contiguous run of the
    // (gallery piece, row block) pairs, row block fastest, so that the workgroups that stream one gallery piece for different query blocks
    // run side by side on one XCD, where all but the first should find it in that L2 (not measured apart from the whole launch).
    const int pairs = nrowblocks * ((nchunks + kWaves - 1) / kWaves), per_xcd = (pairs + 7) / 8;
    const int pair  = (int)(blockIdx.x & 7u) * per_xcd + (int)(blockIdx.x >> 3);
    if ((int)(blockIdx.x >> 3) >= per_xcd || pair >= pairs) return;     // (the whole workgroup, before any barrier)
    const int piece = pair / nrowblocks;
    const int row0  = (pair - piece * nrowblocks) * 32;

    if (tid < 32) bad[tid] = 0;
    __syncthreads();
    for (int idx = tid; idx < 32 * nq; idx += kBlock) {
        const int i = idx / nq, q = idx - i * nq, row = row0 + i;
        float v[8];
        bool  nf = false;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int dd = 8 * q + e;
            v[e] = (row < n && dd < d) ? x[(size_t)row * d + dd] : 0.0f;
            nf |= not_finite(v[e]);
        }
        if (nf) bad[i] = 1;                                     // (every writer writes 1)
        f32x4 lo, hi;
        lo.x = v[0]; lo.y = v[2]; lo.z = v[4]; lo.w = v[6];
        hi.x = v[1]; hi.y = v[3]; hi.z = v[5]; hi.w = v[7];
        xs[q * 64 + i]      = lo;
        xs[q * 64 + 32 + i] = hi;
    }
    __syncthreads();
    for (int idx = tid; idx < 32 * nq; idx += kBlock) {         // a void row is a row of zeros: its chains stay +0 and the merge drops them
        const int i = idx / nq, q = idx - i * nq;
        if (bad[i]) {
            f32x4 z; z.x = 0.0f; z.y = 0.0f; z.z = 0.0f; z.w = 0.0f;
            xs[q * 64 + i]      = z;
            xs[q * 64 + 32 + i] = z;
        }
    }
    __syncthreads();

    const int chunk = piece * kWaves + wave;
    if (chunk >= nchunks) return;                               // (the whole wave; no barrier below)
    const int blk0  = chunk * kTiles;
    const int nblk  = min(kTiles, nblocks - blk0);
    const int total = nblk * nq;                                // 1 KB groups of this wave: one contiguous stream
    const f32x4* src = packed + (size_t)blk0 * nq * 64 + lane;

    f32x4 ring[kRing];                                          // group t0 + u in ring[u]; a load behind the stream reads its last group again
#pragma unroll
    for (int u = 0; u < kRing; ++u) ring[u] = src[(size_t)min(u, total - 1) * 64];

    f32x16 tiles[kTiles];
#pragma unroll
    for (int c = 0; c < kTiles; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) tiles[c][e] = 0.0f;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;

    int   q = 0, b = 0;                                         // wave-uniform: the group inside the block, the block inside the chunk
    f32x4 a_cur = xs[lane];
    auto step = [&](const f32x4 bv) {
        const int   qn    = (q + 1 == nq) ? 0 : q + 1;
        const f32x4 a_nxt = xs[qn * 64 + lane];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.x, bv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.y, bv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.z, bv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.w, bv.w, acc, 0, 0, 0);
        a_cur = a_nxt;
        q     = qn;
        if (qn == 0) {                                          // the tile of block b is complete
#pragma unroll
            for (int c = 0; c < kTiles; ++c)
                if (b == c) tiles[c] = acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
            ++b;
        }
    };
    int t0 = 0;
    for (; t0 + kRing <= total; t0 += kRing) {                  // whole rings: no branch but the tile's end between a load and its use
#pragma unroll
        for (int u = 0; u < kRing; ++u) {
            const f32x4 bv = ring[u];
            ring[u] = src[(size_t)min(t0 + u + kRing, total - 1) * 64];
            step(bv);
        }
    }
#pragma unroll
    for (int u = 0; u < kRing; ++u)
        if (t0 + u < total) step(ring[u]);

    // tile element [register e][lane (h << 5) | j] = a[row0 + (e & 3) + 8 (e >> 2) + 4 h][32 (blk0 + c) + j]
    const int h = lane >> 5, j = lane & 31;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int i0 = (e & 3) + 8 * (e >> 2);
        if (row0 + i0 >= n) continue;                           // (both halves' rows: the other is four further)
        const int row = row0 + i0 + 4 * h;
        unsigned long long keys[kTiles];
#pragma unroll
        for (int c = 0; c < kTiles; ++c) {
            const unsigned at = (unsigned)((blk0 + c) * 32 + j);
            keys[c] = (c < nblk && at < (unsigned)g) ? topk_key(__float_as_uint(tiles[c][e]), at) : 0ull;
        }
        unsigned long long* out = scratch + ((size_t)min(row, n - 1) * nchunks + chunk) * k;
        unsigned long long below = ~0ull;
        for (int jj = 0; jj < k; ++jj) {
            unsigned long long best = 0ull;
#pragma unroll
            for (int c = 0; c < kTiles; ++c) topk_take(best, keys[c], below);
#pragma unroll
            for (int m = 16; m >= 1; m >>= 1) {                 // the maximum of the lane's half wave
                const unsigned long long o = __shfl_xor(best, m, kWave);
                best = o > best ? o : best;
            }
            if (j == 0 && row < n) out[jj] = best;
            below = best;
        }
    }
}

__global__ __launch_bounds__(kBlock) void gallery_merge_kernel(const float* __restrict__ x, int n, int d, int nchunks, int k, int metric,
                                                               int has_min_score, float min_score,
                                                               const unsigned long long* __restrict__ scratch, int* __restrict__ counts,
                                                               int* __restrict__ indices, unsigned* __restrict__ scores,
                                                               double* __restrict__ norms) {
    const int lane = threadIdx.x & (kWave - 1);
    const int r    = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= n) return;                                         // (the whole wave: nothing below meets a barrier)
    const float* row = x + (size_t)r * d;
    double s = 0.0;
    bool   finite = true;
#pragma unroll 8
    for (int i = 0; i < d; ++i) {                               // every lane the same sum, in order: one rounding per addition
        const float  v  = row[i];
        const double dv = (double)v;
        finite = finite && !not_finite(v);
        s = __dadd_rn(s, __dmul_rn(dv, dv));
    }
    const double rr = __dsqrt_rn(s);
    const bool void_row = !finite || (metric == PVHIP_GALLERY_COSINE && s == 0.0);
    if (norms != nullptr && lane == 0) norms[r] = finite ? rr : __longlong_as_double(0x7FF8000000000000LL);

    const unsigned long long* keys = scratch + (size_t)r * nchunks * k;
    unsigned long long below = ~0ull, mine = 0ull;
    if (!void_row) {
        for (int jj = 0; jj < k; ++jj) {
            unsigned long long best = 0ull;
            // A chunk's list is sorted, so its candidate is its first key below `below`: the list's head, behind the winners of earlier
            // rounds that came from this chunk (jj of them over all chunks).  The heads are independent loads; the steps behind them are few.
            for (int c = lane; c < nchunks; c += kWave * kMergeLoads) {
                unsigned long long v[kMergeLoads];
#pragma unroll
                for (int i = 0; i < kMergeLoads; ++i) v[i] = c + kWave * i < nchunks ? keys[(size_t)(c + kWave * i) * k] : 0ull;
#pragma unroll
                for (int i = 0; i < kMergeLoads; ++i) {
                    const int cc = c + kWave * i;
                    unsigned long long key = v[i];
                    int p = 0;
                    while (cc < nchunks && key >= below && ++p < k) key = keys[(size_t)cc * k + p];
                    topk_take(best, key, below);
                }
            }
            best = wave_max_u64(best);
            if (lane == jj) mine = best;
            below = best;
        }
    }
    unsigned score = kQuietNaN;
    int      index = -1;
    bool     kept  = false;
    if (!void_row && lane < k && mine != 0ull) {
        const unsigned ord = (unsigned)(mine >> 32);
        index = (int)(kIndexTop - (unsigned)mine);
        if (ord != 0xFFFFFFFFu) {                               // (a NaN chain value: the quiet NaN)
            const float a  = __uint_as_float((ord & 0x80000000u) ? (ord & 0x7FFFFFFFu) : ~ord);
            const float sc = metric == PVHIP_GALLERY_DOT ? a : (float)((double)a / rr);
            score = (sc != sc) ? kQuietNaN : __float_as_uint(sc);
        }
        kept = has_min_score == 0 || __uint_as_float(score) >= min_score;
    }
    const unsigned long long run = ~__ballot(kept);
    const int count = run == 0ull ? kWave : (int)__ffsll((long long)run) - 1;
    if (lane < k) {
        indices[(size_t)r * k + lane] = lane < count ? index : -1;
        scores[(size_t)r * k + lane]  = lane < count ? score : kQuietNaN;
    }
    if (lane == 0) counts[r] = count;
}

}  // namespace

extern "C" {

int pvhip_gallery_match_f32(const float* x, int n, int d, const float* packed, int g, int k, int metric, int has_min_score,
                            float min_score, void* scratch, int* counts, int* indices, float* scores, double* norms) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(x != nullptr && packed != nullptr && scratch != nullptr && counts != nullptr && indices != nullptr && scores != nullptr);
    PVHIP_CHECK_ARG(((uintptr_t)x & 3u) == 0 && ((uintptr_t)packed & 15u) == 0 && ((uintptr_t)scratch & 7u) == 0);
    PVHIP_CHECK_ARG(((uintptr_t)counts & 3u) == 0 && ((uintptr_t)indices & 3u) == 0 && ((uintptr_t)scores & 3u) == 0 && ((uintptr_t)norms & 7u) == 0);
    PVHIP_CHECK_ARG(n >= 1 && d >= 1 && d <= kMaxD && (long long)n * d < (1LL << 31));
    PVHIP_CHECK_ARG(g >= 1 && g <= kMaxG);
    PVHIP_CHECK_ARG(k >= 1 && k <= g && k <= kMaxK);
    PVHIP_CHECK_ARG(metric == PVHIP_GALLERY_COSINE || metric == PVHIP_GALLERY_DOT);
    PVHIP_CHECK_ARG(has_min_score == 0 || (has_min_score == 1 && min_score == min_score && min_score - min_score == 0.0f));
    const int nq = (d + 7) / 8, nblocks = (g + 31) / 32, nchunks = (g + kChunk - 1) / kChunk;
    const size_t lds = (size_t)nq * 64 * 16 + 32 * sizeof(int);
    const int nrowblocks = (n + 31) / 32;
    const long long pairs = (long long)nrowblocks * ((nchunks + kWaves - 1) / kWaves);
    PVHIP_CHECK_ARG(pairs < (1LL << 30));                       // (the last refusal: nothing is done before it)
    static bool attr_set = false;                               // once, for the largest d: no runtime call per pass
    if (!attr_set) {
        PVHIP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&gallery_scores_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)((size_t)(kMaxD / 8) * 64 * 16 + 32 * sizeof(int))));
        attr_set = true;
    }
    hipLaunchKernelGGL(gallery_scores_kernel, dim3((unsigned)((pairs + 7) / 8 * 8)), dim3(kBlock), lds, state().stream,
                       x, n, d, nq, reinterpret_cast<const f32x4*>(packed), g, nblocks, nchunks, k, nrowblocks,
                       reinterpret_cast<unsigned long long*>(scratch));
    hipLaunchKernelGGL(gallery_merge_kernel, dim3((n + kWaves - 1) / kWaves), dim3(kBlock), 0, state().stream, x, n, d, nchunks, k, metric,
                       has_min_score, min_score, reinterpret_cast<const unsigned long long*>(scratch), counts, indices,
                       reinterpret_cast<unsigned*>(scores), norms);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
