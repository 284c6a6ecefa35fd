// Multi-person poses from the candidates of ``maxima=`` and a stack of part-affinity fields (n, 2L, H, W), on the device: what users of
// OpenPose-style heads do on the host after reading the fields back -- score every candidate pair of every limb along the segment between
// them, match greedily, walk the limbs to assemble persons.  include/pvhip.h states the rule (pvhip_pose_groups_f32),
// pyopenvino_amd/poses.py and tests/poses_ref.py are the same in numpy and in plain loops.  One entry, two launches, no initialising
// launch, no global-memory atomics: three calls give the same bits.
//
// Launch 1, limbs (pose_limbs_kernel): one workgroup of 256 lanes per (row, limb).
//   stage   wave 0 reads the limb's two candidate lists from the keys pvhip_heatmap_maxima_f32 left in its scratch, a's in lanes 0 .. 31
//           and b's in lanes 32 .. 63, and leaves (x, y, the plane's own bits there) in LDS; the run of non-zero keys in front is one
//           ballot per list.
//   score   the limb's ma * mb pairs go through LDS in chunks of at most kItems samples (16 KB): a lane per pair forms the unit vector
//           (one correctly rounded root, two divisions) once, then the chunk's (pair, sample) items are flattened over all 256 lanes,
//           sample-major -- an image with three people has nine pairs of ten samples, which is still one and a half waves of taps in
//           flight -- and every item reads its two taps straight from global memory and leaves v_s at v[s * pairs + q]: consecutive lanes
//           write and, in the reduction, read consecutive words.  A lane per pair then adds the passing samples in order of s.
//   match   a valid pair's key is (score bits, ~(i * 32 + j)): the score is positive, so its bits order like the number, and the lower i,
//           then the lower j, stands in front among equals.  The keys go through keep_add / keep_cut of pvhip_keep.h (all 1024 fit: one
//           sort, no cut).  Wave 0 walks them 64 at a time with the two used-sets as wave-uniform 32-bit masks: a ballot of the lanes
//           whose i and j are both free, find-first, take, again -- the lanes in front of a taken one are dead for good, since the sets
//           only grow -- at most min(ma, mb) takes.
//   out     the limb's taken connections, 16 bytes each (the key, the two heat values as bits), and their number.
// Launch 2, persons (pose_persons_kernel): one wave per row; lanes are persons.  The slot table (joint, person) -> candidate is bytes in
// LDS, a person's total and joint count are its lane's registers.  A limb's 32 records are one 16-byte load per lane, issued one limb
// ahead; a connection is one ballot on slot[a] == i and one lane's update.  Then the screen, a ballot-prefix compaction, and lanes over
// (person, joint) write every slot of the answer once, filler included; the points go through pvhip_point_rule.h.
#include "pvhip_common.h"
#include "pvhip_keep.h"
#include "pvhip_point_rule.h"
#include "pvhip_topk_keys.h"

using namespace pvhip;

namespace {

constexpr int kCand  = PVHIP_POSES_MAX_CANDIDATES;      // candidates of a plane at most: a used-set is one 32-bit mask
constexpr int kPairs = kCand * kCand;                   // pairs of a limb at most
constexpr int kItems = 4096;                            // samples of a chunk of pairs in LDS

struct Limbs {                                          // the skeleton, a kernel argument (328 bytes)
    int count;
    unsigned long long founds;                          // bit l: limb l may found a person
    unsigned char a[PVHIP_POSES_MAX_LIMBS], b[PVHIP_POSES_MAX_LIMBS], cx[PVHIP_POSES_MAX_LIMBS], cy[PVHIP_POSES_MAX_LIMBS];
};

struct ScorePlan {
    int k, h, w, m, channels, samples, min_samples;
    float min_field;
};

struct GroupPlan {
    int k, h, w, m, persons, min_joints, refine, space;
    float min_mean;
};

__device__ __forceinline__ int floor_div(int a, int b) {        // b > 0
    const int q = a / b;
    return q - ((a - q * b) < 0 ? 1 : 0);
}

// The run of non-zero keys in front of a list, given the ballot of "my key is not zero" of its 32 lanes.
__device__ __forceinline__ int leading_run(unsigned have) { return have == 0xFFFFFFFFu ? 32 : __ffs((int)~have) - 1; }

__global__ __launch_bounds__(kBlock) void pose_limbs_kernel(const float* __restrict__ heat, const unsigned long long* __restrict__ cands,
                                                            const float* __restrict__ pafs, ScorePlan p, Limbs limbs,
                                                            uint4* __restrict__ conns, int* __restrict__ conn_counts) {
    __shared__ unsigned long long keys[kPairs];
    __shared__ float v[kItems];
    __shared__ float ux[kPairs], uy[kPairs];
    __shared__ int cand_x[2 * kCand], cand_y[2 * kCand];        // a's candidates at 0 .. 31, b's at 32 .. 63
    __shared__ unsigned cand_bits[2 * kCand];
    __shared__ int count, fill[2];
    const int tid = threadIdx.x;
    const int r = blockIdx.x / limbs.count, l = blockIdx.x - r * limbs.count;
    const unsigned size = (unsigned)(p.h * p.w);
    if (tid < kWave) {
        const int side = tid >> 5, c = tid & 31;
        const size_t plane = (size_t)r * (size_t)p.k + (size_t)(side ? limbs.b[l] : limbs.a[l]);
        const unsigned long long key = c < p.m ? cands[plane * (size_t)p.m + (size_t)c] : 0ull;
        const unsigned long long have = __ballot(key != 0ull);
        if (key != 0ull) {
            const unsigned at = min(kIndexTop - (unsigned)key, size - 1u);     // (a key of the maxima launch: below size)
            cand_y[tid] = (int)(at / (unsigned)p.w);
            cand_x[tid] = (int)(at - (at / (unsigned)p.w) * (unsigned)p.w);
            cand_bits[tid] = reinterpret_cast<const unsigned*>(heat)[plane * (size_t)size + at];
        }
        if (tid == 0) {
            fill[0] = leading_run((unsigned)have);
            fill[1] = leading_run((unsigned)(have >> 32));
            count = 0;
        }
    }
    __syncthreads();
    const int ma = fill[0], mb = fill[1], pairs = ma * mb, S = p.samples;
    const int per = min(kPairs, kItems / S);
    const float* fx = pafs + ((size_t)r * (size_t)p.channels + (size_t)limbs.cx[l]) * (size_t)size;
    const float* fy = pafs + ((size_t)r * (size_t)p.channels + (size_t)limbs.cy[l]) * (size_t)size;
    for (int base = 0; base < pairs; base += per) {             // (the same trips in every lane)
        const int np = min(per, pairs - base);
        for (int q = tid; q < np; q += kBlock) {
            const int i = (base + q) / mb, j = (base + q) - i * mb;
            const int dx = cand_x[kCand + j] - cand_x[i], dy = cand_y[kCand + j] - cand_y[i];
            const float len = sqrtf((float)((long long)dx * dx + (long long)dy * dy));
            ux[q] = (float)dx / len;                            // (dx == dy == 0: 0 / 0, a NaN, which passes no sample)
            uy[q] = (float)dy / len;
        }
        __syncthreads();
        for (int t = tid; t < np * S; t += kBlock) {
            const int s = t / np, q = t - s * np;
            const int i = (base + q) / mb, j = (base + q) - i * mb;
            const int ax = cand_x[i], ay = cand_y[i];
            const int x = ax + floor_div(2 * s * (cand_x[kCand + j] - ax) + (S - 1), 2 * (S - 1));
            const int y = ay + floor_div(2 * s * (cand_y[kCand + j] - ay) + (S - 1), 2 * (S - 1));
            const size_t at = (size_t)y * (size_t)p.w + (size_t)x;     // (between a and b: inside the plane)
            v[t] = fx[at] * ux[q] + fy[at] * uy[q];
        }
        __syncthreads();
        for (int q = tid; q < np; q += kBlock) {
            int c = 0;
            float sum = 0.0f;
            for (int s = 0; s < S; ++s) {
                const float vs = v[s * np + q];
                if (vs > p.min_field) {
                    ++c;
                    sum = sum + vs;
                }
            }
            if (c >= p.min_samples) {
                const int i = (base + q) / mb, j = (base + q) - i * mb;
                const float score = sum / (float)c;
                keep_add(keys, &count, kPairs, ((unsigned long long)__float_as_uint(score) << 32) | (unsigned long long)~(unsigned)(i * kCand + j));
            }
        }
        __syncthreads();                                        // v, ux and uy are written again; the last keep_add is behind
    }
    keep_cut<kBlock>(keys, &count, kPairs, kPairs, 0ull);       // sorts; nothing is cut
    if (tid >= kWave) return;
    const int nk = min(count, kPairs), most = min(ma, mb);
    uint4* out = conns + (size_t)blockIdx.x * (size_t)kCand;
    unsigned used_a = 0u, used_b = 0u;
    int taken = 0;
    for (int base = 0; base < nk && taken < most; base += kWave) {
        const bool have = base + tid < nk;
        const unsigned long long key = have ? keys[base + tid] : 0ull;
        const unsigned index = ~(unsigned)key, i = (index >> 5) & 31u, j = index & 31u;
        for (;;) {
            const unsigned long long open = __ballot(have && ((used_a >> i) & 1u) == 0u && ((used_b >> j) & 1u) == 0u);
            if (open == 0ull) break;
            const int first = __ffsll((long long)open) - 1;
            used_a |= 1u << __shfl(i, first, kWave);
            used_b |= 1u << __shfl(j, first, kWave);
            if (tid == first) out[taken] = make_uint4((unsigned)key, (unsigned)(key >> 32), cand_bits[i], cand_bits[kCand + j]);
            ++taken;
        }
    }
    if (tid == 0) conn_counts[blockIdx.x] = taken;
}

__global__ __launch_bounds__(kWave) void pose_persons_kernel(const float* __restrict__ heat, const unsigned long long* __restrict__ cands,
                                                             const uint4* __restrict__ conns, const int* __restrict__ conn_counts,
                                                             GroupPlan p, Limbs limbs, int* __restrict__ counts, int* __restrict__ joints,
                                                             unsigned* __restrict__ scores, unsigned* __restrict__ points,
                                                             unsigned* __restrict__ totals) {
    extern __shared__ signed char slots[];                      // [joint][person]: the candidate, -1 for none
    __shared__ unsigned char order[kWave];
    __shared__ unsigned total_of[kWave];
    const int lane = threadIdx.x, r = blockIdx.x, P = p.persons, K = p.k, L = limbs.count;
    const unsigned size = (unsigned)(p.h * p.w);
    for (int q = lane; q < K * P; q += kWave) slots[q] = -1;
    __syncthreads();
    const int my_count = lane < L ? conn_counts[(size_t)r * L + lane] : 0;
    const uint4* mine = conns + (size_t)r * (size_t)L * (size_t)kCand;
    const uint4 none = make_uint4(0u, 0u, 0u, 0u);
    uint4 next = lane < kCand ? mine[lane] : none;
    float total = 0.0f;
    int have = 0, persons = 0;
    for (int l = 0; l < L; ++l) {
        const uint4 rec = next;
        if (l + 1 < L && lane < kCand) next = mine[(size_t)(l + 1) * kCand + lane];
        const int cnt = min(__shfl(my_count, l, kWave), kCand);
        const int a = limbs.a[l], b = limbs.b[l];
        const bool founds = ((limbs.founds >> l) & 1ull) != 0ull;
        for (int t = 0; t < cnt; ++t) {
            const unsigned index = ~__shfl(rec.x, t, kWave);
            const int i = (int)((index >> 5) & 31u), j = (int)(index & 31u);
            const float score = __uint_as_float(__shfl(rec.y, t, kWave));
            const float ha = __uint_as_float(__shfl(rec.z, t, kWave)), hb = __uint_as_float(__shfl(rec.w, t, kWave));
            const unsigned long long holds = __ballot(lane < persons && slots[a * P + lane] == i);
            if (holds != 0ull) {
                const int first = __ffsll((long long)holds) - 1;
                if (lane == first && slots[b * P + lane] < 0) {
                    slots[b * P + lane] = (signed char)j;
                    total = (total + hb) + score;
                    ++have;
                }
            } else if (founds && persons < P) {
                if (lane == persons) {
                    slots[a * P + lane] = (signed char)i;
                    slots[b * P + lane] = (signed char)j;
                    total = (ha + hb) + score;
                    have = 2;
                }
                ++persons;
            }
            __syncthreads();                                    // (one wave: the table's writes stand before the next ballot's reads)
        }
    }
    const bool keep = lane < persons && have >= p.min_joints && total / (float)have >= p.min_mean;
    const unsigned long long kept = __ballot(keep);
    const int count = __popcll(kept);
    if (keep) {
        const int rank = __popcll(kept & ((1ull << lane) - 1ull));
        order[rank] = (unsigned char)lane;
        total_of[rank] = __float_as_uint(total);
    }
    __syncthreads();
    if (lane == 0) counts[r] = count;
    if (lane < P) totals[(size_t)r * P + lane] = lane < count ? total_of[lane] : kQuietNaN;
    for (int q = lane; q < P * K; q += kWave) {
        const int person = q / K, k = q - person * K;
        int at = -1;
        unsigned bits = kQuietNaN, fx = kQuietNaN, fy = kQuietNaN;
        const int c = person < count ? slots[k * P + order[person]] : -1;
        if (c >= 0) {
            const size_t plane = (size_t)r * (size_t)K + (size_t)k;
            at = (int)min(kIndexTop - (unsigned)cands[plane * (size_t)p.m + (size_t)c], size - 1u);
            const float* values = heat + plane * (size_t)size;
            bits = reinterpret_cast<const unsigned*>(values)[at];               // the plane's own bits
            point_of(values, at, p.h, p.w, p.refine, p.space, fx, fy);
        }
        const size_t slot = (size_t)r * (size_t)(P * K) + (size_t)q;
        joints[slot]         = at;
        scores[slot]         = bits;
        points[2 * slot]     = fx;
        points[2 * slot + 1] = fy;
    }
}

}  // namespace

extern "C" {

int pvhip_pose_groups_f32(const float* heat, const unsigned long long* candidates, const float* pafs, int n, int k, int h, int w,
                          int max_per_plane, int channels, const int* skeleton, int limbs, int refine, int space, int samples,
                          float min_field, int min_samples, int max_persons, int min_joints, float min_mean, void* scratch, int* counts,
                          int* joints, float* scores, float* points, float* totals) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(heat != nullptr && candidates != nullptr && pafs != nullptr && skeleton != nullptr && scratch != nullptr && counts != nullptr &&
                    joints != nullptr && scores != nullptr && points != nullptr && totals != nullptr);
    PVHIP_CHECK_ARG(((uintptr_t)heat & 3u) == 0 && ((uintptr_t)candidates & 7u) == 0 && ((uintptr_t)pafs & 3u) == 0 && ((uintptr_t)scratch & 15u) == 0 &&
                    ((uintptr_t)counts & 3u) == 0 && ((uintptr_t)joints & 3u) == 0 && ((uintptr_t)scores & 3u) == 0 && ((uintptr_t)points & 3u) == 0 &&
                    ((uintptr_t)totals & 3u) == 0);
    PVHIP_CHECK_ARG(n >= 1 && h >= 1 && w >= 1 && k >= 1 && k <= PVHIP_POSES_MAX_JOINTS);
    PVHIP_CHECK_ARG((long long)h * w >= 2 && (long long)h * w <= PVHIP_MAXIMA_MAX_PLANE);
    PVHIP_CHECK_ARG(limbs >= 1 && limbs <= PVHIP_POSES_MAX_LIMBS && channels >= 1 && channels <= 2 * PVHIP_POSES_MAX_LIMBS);
    PVHIP_CHECK_ARG((long long)n * k * h * w < (1LL << 31) && (long long)n * channels * h * w < (1LL << 31));
    PVHIP_CHECK_ARG(max_per_plane >= 1 && max_per_plane <= PVHIP_POSES_MAX_CANDIDATES);
    PVHIP_CHECK_ARG(refine == PVHIP_PEAKS_NONE || refine == PVHIP_PEAKS_QUARTER);
    PVHIP_CHECK_ARG(space == PVHIP_PEAKS_HEATMAP || space == PVHIP_PEAKS_NORMALISED);
    PVHIP_CHECK_ARG(samples >= 2 && samples <= PVHIP_POSES_MAX_SAMPLES && min_samples >= 1 && min_samples <= samples);
    PVHIP_CHECK_ARG(min_field - min_field == 0.0f && min_field >= 0.0f && min_mean - min_mean == 0.0f);     // finite
    PVHIP_CHECK_ARG(max_persons >= 1 && max_persons <= PVHIP_POSES_MAX_PERSONS && min_joints >= 1 && min_joints <= k);
    PVHIP_CHECK_ARG((long long)n * limbs < (1LL << 26));
    Limbs table{};
    table.count = limbs;
    for (int l = 0; l < limbs; ++l) {
        const int* row = skeleton + 5 * l;
        PVHIP_CHECK_ARG(row[0] >= 0 && row[0] < k && row[1] >= 0 && row[1] < k && row[0] != row[1]);
        PVHIP_CHECK_ARG(row[2] >= 0 && row[2] < channels && row[3] >= 0 && row[3] < channels && (row[4] == 0 || row[4] == 1));
        table.a[l]  = (unsigned char)row[0];
        table.b[l]  = (unsigned char)row[1];
        table.cx[l] = (unsigned char)row[2];
        table.cy[l] = (unsigned char)row[3];
        table.founds |= (unsigned long long)row[4] << l;
    }
    uint4* conns = static_cast<uint4*>(scratch);
    int* conn_counts = reinterpret_cast<int*>(conns + (size_t)n * (size_t)limbs * (size_t)kCand);
    const ScorePlan score{k, h, w, max_per_plane, channels, samples, min_samples, min_field};
    hipLaunchKernelGGL(pose_limbs_kernel, dim3((unsigned)(n * limbs)), dim3(kBlock), 0, state().stream, heat, candidates, pafs, score, table,
                       conns, conn_counts);
    PVHIP_LAUNCH_CHECK();
    const GroupPlan group{k, h, w, max_per_plane, max_persons, min_joints, refine, space, min_mean};
    hipLaunchKernelGGL(pose_persons_kernel, dim3((unsigned)n), dim3(kWave), (size_t)k * (size_t)max_persons, state().stream, heat, candidates,
                       conns, conn_counts, group, table, counts, joints, reinterpret_cast<unsigned*>(scores),
                       reinterpret_cast<unsigned*>(points), reinterpret_cast<unsigned*>(totals));
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
