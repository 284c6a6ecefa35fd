// The connected components of one plane of a probability map (n, K, H, W), on the device: what users of DBNet, PixelLink-style and
// PSENet text detectors, CRAFT's region map and blob heads do on the host with a threshold and cv2.connectedComponentsWithStats after
// reading the whole map back.  include/pvhip.h states the rule (pvhip_components_f32), pyopenvino_amd/components.py and
// tests/components_ref.py are the same in numpy and in plain loops.
//
// Union-find over three plane-sized int32 arrays in `scratch` -- parent, area, peak word: 12 bytes a pixel -- in five launches on the
// current stream (profiles/components.md has their times and the four places where this differs from the first plan):
//   1 tiles    a workgroup of 256 lanes owns a tile of 32 rows x 128 columns.  A lane loads four quads of four pixels by 16-byte loads at
//              whatever 4-byte phase the plane stands and leaves their foreground flags as bytes in LDS; a wave then forms each of its eight
//              rows' foreground as two 64-bit ballots, so that a row is a wave-uniform 128-bit mask and the horizontal work is done on bits:
//              a pixel's first label is the position of its run's start, the bit behind the last zero below it, and a run costs no union.
//              Runs of adjacent rows are united by atomicMin in LDS, one union per run of `up & m` (an upper and a lower run overlap in one
//              interval) and, with 8-connectivity, one per diagonal touch that no overlap covers: upper b over lower b + 1 with upper b + 1
//              and lower b clear, and its mirror image.  Every pixel then finds its tile root and writes it as a global flat index, -1 for
//              background, and zeroes its area and peak words.
//   2 seams    a lane per pixel of every tile's top row and left column unites it with its foreground neighbours across the seam -- up,
//              left and, with 8-connectivity, the two upper diagonals and the lower left -- where the pixel before it in the same tile
//              does not already make the same union.  The union is lock-free: find both roots, hang the larger under the smaller with atomicMin, and where
//              the value returned shows that someone else has moved it, go on from that value.  Parents only decrease: it ends, and no
//              workgroup waits for another.
//   3 flatten  every foreground pixel follows its parent to the root and stores it; the lanes of a wave that hold a run of equal roots
//              reduce their count and their largest order word (pvhip_topk_keys.h) by segmented shuffles, and the run's first lane adds
//              them at the root's slot of the area and peak arrays (atomicAdd, atomicMax).
//   4 select   one workgroup per image walks its roots (parent[g] == g), counts them, and keeps the R largest keys
//              area << 24 | (2^24 - 1 - seed) with pvhip_keep.h.  It writes the (n, R) table -- seeds, areas, peaks, -1 behind the count --,
//              initialises the winners' statistics and leaves -(rank + 1) in the area array at each winner's root: areas are positive, so a
//              negative word says "ranked" and no second walk has to mark the other roots.
//   5 stats    every foreground pixel looks up root -> rank; ranked pixels add rectangle bounds, the Q16 sum and the five moments, reduced
//              over the wave's runs as in 3, into a table of R slots x 64 bytes in LDS, which leaves by integer atomics when the workgroup's
//              image changes and when it ends (pvhip_segments.hip's pattern).  A component whose peak is a zero asks for the sign of its
//              first zero in raster order: atomicMin of (index << 1 | sign) into `zeros`.
// Every sum is an integer, every other result a minimum or maximum over a total order: the order of lanes, waves and workgroups does not show.
#include "pvhip_common.h"
#include "pvhip_keep.h"
#include "pvhip_topk_keys.h"

using namespace pvhip;

namespace {

constexpr int kRows = PVHIP_COMPONENTS_TILE_ROWS, kCols = PVHIP_COMPONENTS_TILE_COLS;
constexpr int kTile = kRows * kCols;
static_assert(kRows == 32 && kCols == 128 && kBlock == 256, "four waves of eight rows, a row two ballots, a lane four quads");
constexpr unsigned kNaNWord  = 0xFFFFFFFFu;
constexpr unsigned kZeroWord = 0x80000000u;
constexpr int      kSeedTop  = PVHIP_COMPONENTS_MAX_PLANE - 1;
constexpr int      kSelKeys  = 2048;                // the key buffer of components_select_kernel
constexpr int      kSelTrip  = 1024;                // pixels it takes per trip: kSelKeys - PVHIP_COMPONENTS_MAX_PER_IMAGE
constexpr int      kNone     = 0x7FFFFFFF;

struct __attribute__((aligned(4))) F4 { unsigned x, y, z, w; };     // 16 bytes at any 4-byte phase
struct __attribute__((aligned(4))) I4 { int x, y, z, w; };

struct Plan {
    int       n, k, h, w, size, channel, eight;
    unsigned  min_word;                             // the order word of min_score
    int       min_area, keep, tiles_x, tiles_y;
    long long total;                                // n * h * w
    FastDiv   by_size, by_w;
};

__device__ __forceinline__ unsigned order_of(unsigned bits) { return (unsigned)(topk_key(bits, 0u) >> 32); }
__device__ __forceinline__ unsigned foreground(unsigned bits, unsigned min_word) {
    const unsigned o = order_of(bits);
    return (o != kNaNWord && o >= min_word) ? 1u : 0u;
}

// ---- 128-bit row masks
struct M128 { unsigned long long lo, hi; };
__device__ __forceinline__ M128 operator&(M128 a, M128 b) { return {a.lo & b.lo, a.hi & b.hi}; }
__device__ __forceinline__ M128 operator~(M128 a) { return {~a.lo, ~a.hi}; }
__device__ __forceinline__ M128 shl1(M128 a) { return {a.lo << 1, (a.hi << 1) | (a.lo >> 63)}; }     // bit b := bit b - 1
__device__ __forceinline__ M128 shr1(M128 a) { return {(a.lo >> 1) | (a.hi << 63), a.hi >> 1}; }     // bit b := bit b + 1

// ---- union-find: parents only decrease; a root is its own parent
template <int SCOPE>
__device__ __forceinline__ int find_root(int* parent, int a) {
    for (;;) {
        const int p = __hip_atomic_load(parent + a, __ATOMIC_RELAXED, SCOPE);
        if (p == a) return a;
        a = p;
    }
}

template <int SCOPE>
__device__ __forceinline__ void unite(int* parent, int a, int b) {
    for (;;) {
        a = find_root<SCOPE>(parent, a);
        b = find_root<SCOPE>(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }                  // a: the larger root, hung under b
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;                                                        // someone else moved it: what it hangs under now joins b
    }
}

// ---- the reduction of a value over each run of lanes: `heads` has the bit of every run's first lane; the first lane gets the result
template <class T, class Op>
__device__ __forceinline__ T run_reduce(T v, unsigned long long heads, int lane, Op op) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const T o = __shfl_down(v, d, kWave);
        const bool same = lane + d < kWave && (((heads >> lane) >> 1) & ((1ull << d) - 1ull)) == 0ull;
        if (same) v = op(v, o);
    }
    return v;
}
__device__ __forceinline__ unsigned long long run_heads(int id, int lane) {
    const int before = __shfl_up(id, 1, kWave);
    return __ballot(lane == 0 || before != id);
}
__device__ __forceinline__ int run_length(unsigned long long heads, int lane) {
    const unsigned long long rest = (heads >> lane) >> 1;
    return rest ? __ffsll((long long)rest) : kWave - lane;
}

// ---------------------------------------------------------------------------------------------------------------- 1 tiles
__global__ __launch_bounds__(kBlock) void components_tiles_kernel(const unsigned* __restrict__ x, Plan a, int* __restrict__ parent,
                                                                  int* __restrict__ area, unsigned* __restrict__ peak) {
    __shared__ unsigned           flags[kTile / 4];                     // a byte per pixel: 1 foreground
    __shared__ unsigned long long mask[kRows][2];
    __shared__ int                lab[kTile];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const unsigned per_image = (unsigned)(a.tiles_x * a.tiles_y);
    const int r   = (int)(blockIdx.x / per_image);
    const int rem = (int)(blockIdx.x - (unsigned)r * per_image);
    const int y0 = (rem / a.tiles_x) * kRows, x0 = (rem % a.tiles_x) * kCols;
    const unsigned* plane = x + ((size_t)r * a.k + a.channel) * (size_t)a.size;
#pragma unroll
    for (int it = 0; it < kTile / 4 / kBlock; ++it) {
        const int q = it * kBlock + tid, y = y0 + (q >> 5), xx = x0 + (q & 31) * 4;
        unsigned f = 0u;
        if (y < a.h && xx < a.w) {
            const unsigned* at = plane + (size_t)y * a.w + xx;
            if (xx + 3 < a.w) {
                const F4 v = *reinterpret_cast<const F4*>(at);
                f = foreground(v.x, a.min_word) | (foreground(v.y, a.min_word) << 8) | (foreground(v.z, a.min_word) << 16) |
                    (foreground(v.w, a.min_word) << 24);
            } else {
                for (int i = 0; xx + i < a.w; ++i) f |= foreground(at[i], a.min_word) << (8 * i);
            }
        }
        flags[q] = f;
    }
    __syncthreads();
    const unsigned char* flag = reinterpret_cast<const unsigned char*>(flags);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int i = 0; i < kRows / 4; ++i) {                               // a row's masks and every pixel's first label: its run's start
        const int row = wave * (kRows / 4) + i;
        const unsigned long long m0 = __ballot(flag[row * kCols + lane] != 0), m1 = __ballot(flag[row * kCols + kWave + lane] != 0);
        if (lane == 0) { mask[row][0] = m0; mask[row][1] = m1; }
        const unsigned long long z0 = ~m0 & below, z1 = ~m1 & below, zall = ~m0;
        const int low = zall ? kWave - __clzll((long long)zall) : 0;    // where a run that reaches bit 64 from above starts
        if ((m0 >> lane) & 1ull) lab[row * kCols + lane] = row * kCols + (z0 ? kWave - __clzll((long long)z0) : 0);
        if ((m1 >> lane) & 1ull) lab[row * kCols + kWave + lane] = row * kCols + (z1 ? 2 * kWave - __clzll((long long)z1) : low);
    }
    __syncthreads();
    for (int i = 0; i < kRows / 4; ++i) {                               // the runs of adjacent rows
        const int row = wave * (kRows / 4) + i;
        if (row == 0) continue;
        const M128 up{mask[row - 1][0], mask[row - 1][1]}, m{mask[row][0], mask[row][1]};
        const M128 both = up & m;
        const M128 s = both & ~shl1(both);                              // the first bit of each overlap
        M128 dr{0ull, 0ull}, dl{0ull, 0ull};
        if (a.eight) {
            dr = up & shr1(m) & ~shr1(up) & ~m;                         // upper b over lower b + 1, not joined by an overlap
            dl = up & shl1(m) & ~shl1(up) & ~m;                         // upper b over lower b - 1
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int col = half * kWave + lane, above = (row - 1) * kCols + col, here = row * kCols + col;
            if (((half ? s.hi : s.lo) >> lane) & 1ull) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, above, here);
            if (((half ? dr.hi : dr.lo) >> lane) & 1ull) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, above, here + 1);
            if (((half ? dl.hi : dl.lo) >> lane) & 1ull) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, above, here - 1);
        }
    }
    __syncthreads();
    const int base = r * a.size;
#pragma unroll
    for (int it = 0; it < kTile / 4 / kBlock; ++it) {
        const int q = it * kBlock + tid, row = q >> 5, col = (q & 31) * 4, y = y0 + row, xx = x0 + col;
        if (y >= a.h || xx >= a.w) continue;
        const unsigned f = flags[q];
        int out[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            out[i] = -1;
            if ((f >> (8 * i)) & 1u) {
                const int root = find_root<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, row * kCols + col + i);
                out[i] = base + (y0 + (root >> 7)) * a.w + x0 + (root & (kCols - 1));
            }
        }
        const size_t g = (size_t)base + (size_t)y * a.w + xx;
        if (xx + 3 < a.w) {
            *reinterpret_cast<I4*>(parent + g) = I4{out[0], out[1], out[2], out[3]};
            *reinterpret_cast<I4*>(area + g)   = I4{0, 0, 0, 0};
            *reinterpret_cast<I4*>(peak + g)   = I4{0, 0, 0, 0};
        } else {
            for (int i = 0; xx + i < a.w; ++i) {
                parent[g + i] = out[i];
                area[g + i]   = 0;
                peak[g + i]   = 0u;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- 2 seams
// Item j of an image: the (tiles_y - 1) * w pixels of the rows 32, 64, ... first, then the (tiles_x - 1) * h pixels of the columns 128, 256, ...
__global__ __launch_bounds__(kBlock) void components_seams_kernel(Plan a, int* __restrict__ parent, long long items, int per_image) {
    constexpr int kScope = __HIP_MEMORY_SCOPE_AGENT;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < items; i += (long long)gridDim.x * kBlock) {
        const int r = (int)(i / per_image);
        int j = (int)(i - (long long)r * per_image);
        int* p = parent + (size_t)r * a.size;                           // the image's own parents; their values are global: + base
        const int base = r * a.size, across = (a.tiles_y - 1) * a.w;
        auto fg = [&](int xx, int y) { return xx >= 0 && xx < a.w && y >= 0 && y < a.h && p[y * a.w + xx] >= 0; };   // (never changes sign)
        auto join = [&](int xa, int ya, int xb, int yb) { unite<kScope>(parent, base + ya * a.w + xa, base + yb * a.w + xb); };
        if (j < across) {                                               // a tile's top row: up and the two upper diagonals
            const int y = (j / a.w + 1) * kRows, xx = j % a.w;
            if (!fg(xx, y)) continue;
            const bool up = fg(xx, y - 1), left = fg(xx - 1, y), right = fg(xx + 1, y);
            if (up && !(xx % kCols != 0 && left && fg(xx - 1, y - 1))) join(xx, y, xx, y - 1);      // (at a tile corner nobody else joins the two)
            if (a.eight && !up) {
                if (!left && fg(xx - 1, y - 1)) join(xx, y, xx - 1, y - 1);
                if (!right && fg(xx + 1, y - 1)) join(xx, y, xx + 1, y - 1);
            }
        } else {                                                        // a tile's left column: left, upper left and lower left
            j -= across;
            const int xx = (j / a.h + 1) * kCols, y = j % a.h;
            if (!fg(xx, y)) continue;
            const bool left = fg(xx - 1, y), up = fg(xx, y - 1), down = fg(xx, y + 1);
            if (left && !(y % kRows != 0 && up && fg(xx - 1, y - 1))) join(xx, y, xx - 1, y);
            if (a.eight && !left) {
                if (!up && fg(xx - 1, y - 1)) join(xx, y, xx - 1, y - 1);
                if (!down && fg(xx - 1, y + 1)) join(xx, y, xx - 1, y + 1);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- 3 flatten
__global__ __launch_bounds__(kBlock) void components_flatten_kernel(const unsigned* __restrict__ x, Plan a, int* __restrict__ parent,
                                                                    int* __restrict__ area, unsigned* __restrict__ peak) {
    const int lane = threadIdx.x & (kWave - 1);
    for (long long at = (long long)blockIdx.x * kBlock; at < a.total; at += (long long)gridDim.x * kBlock) {      // (the whole workgroup)
        const long long g = at + threadIdx.x;
        int root = -1;
        unsigned word = 0u;
        if (g < a.total) {
            const int first = parent[g];
            if (first >= 0) {
                root = find_root<__HIP_MEMORY_SCOPE_AGENT>(parent, first);
                if (root != first) __hip_atomic_store(parent + g, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned r = fdiv((unsigned)g, a.by_size);
                word = order_of(x[((size_t)r * a.k + a.channel) * (size_t)a.size + ((unsigned)g - r * (unsigned)a.size)]);
            }
        }
        const unsigned long long heads = run_heads(root, lane);
        const unsigned most = run_reduce(word, heads, lane, [](unsigned u, unsigned v) { return u > v ? u : v; });
        if (((heads >> lane) & 1ull) && root >= 0) {
            atomicAdd(area + root, run_length(heads, lane));
            atomicMax(peak + root, most);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- 4 select
struct Table {
    int *counts, *found, *seeds, *areas;
    unsigned* peaks;
    int *zeros, *rects;
    unsigned long long *sums, *moments;
};

__device__ __forceinline__ unsigned bits_of(unsigned word) {           // the float of an order word; a zero's sign is `zeros`' to say
    return word == kZeroWord ? 0u : ((word & 0x80000000u) ? (word & 0x7FFFFFFFu) : ~word);
}

__global__ __launch_bounds__(kBlock) void components_select_kernel(Plan a, const int* __restrict__ parent, int* __restrict__ area,
                                                                   const unsigned* __restrict__ peak, Table t) {
    __shared__ unsigned long long keys[kSelKeys];
    __shared__ int count, roots;
    const int tid = threadIdx.x;
    for (int r = blockIdx.x; r < a.n; r += gridDim.x) {
        const int base = r * a.size;
        if (tid == 0) { count = 0; roots = 0; }
        unsigned long long floor = 0ull;
        int mine = 0;
        for (int start = 0; start < a.size; start += kSelTrip) {
            __syncthreads();
            const int fill = count;
            __syncthreads();                                            // (nobody adds before everybody has read the fill: all cut or none)
            if (fill + kSelTrip > kSelKeys) floor = keep_cut<kBlock>(keys, &count, kSelKeys, a.keep, floor);
            const int end = min(a.size, start + kSelTrip);
            for (int p = start + tid; p < end; p += kBlock) {
                if (parent[base + p] != base + p) continue;
                ++mine;
                const int pixels = area[base + p];
                const unsigned long long key = ((unsigned long long)pixels << 24) | (unsigned long long)(kSeedTop - p);
                if (pixels >= a.min_area && key > floor) keep_add(keys, &count, kSelKeys, key);
            }
        }
        if (mine) atomicAdd(&roots, mine);
        __syncthreads();
        floor = keep_cut<kBlock>(keys, &count, kSelKeys, a.keep, floor);
        const int kept = min(count, a.keep);
        if (tid == 0) { t.counts[r] = kept; t.found[r] = roots; }
        for (int j = tid; j < a.keep; j += kBlock) {
            const size_t at = (size_t)r * a.keep + j;
            int seed = -1, pixels = -1;
            unsigned bits = 0xFFFFFFFFu;
            if (j < kept) {
                seed   = kSeedTop - (int)(keys[j] & (unsigned long long)kSeedTop);
                pixels = (int)(keys[j] >> 24);
                bits   = bits_of(peak[base + seed]);
                area[base + seed] = -(j + 1);                           // root -> rank, for the statistics launch
            }
            t.seeds[at] = seed;
            t.areas[at] = pixels;
            t.peaks[at] = bits;
            t.zeros[at] = kNone;
            t.rects[4 * at + 0] = a.w;
            t.rects[4 * at + 1] = a.h;
            t.rects[4 * at + 2] = -1;
            t.rects[4 * at + 3] = -1;
            t.sums[at] = 0ull;
#pragma unroll
            for (int m = 0; m < 5; ++m) t.moments[5 * at + m] = 0ull;
        }
        __syncthreads();                                                // count, roots and keys[] are written again for the next image
    }
}

// ---------------------------------------------------------------------------------------------------------------- 5 stats
struct Stat {
    int                x0, y0, x1, y1;
    unsigned long long sum, m[5];
};
static_assert(sizeof(Stat) == 64, "a slot of the LDS table");
// The largest table is the 64 KB of dynamic LDS that a launch may ask for without hipFuncAttributeMaxDynamicSharedMemorySize: no attribute
// is set, so nothing here is per process or per device.  A larger R needs the attribute, set for the device of every launch.
static_assert(sizeof(Stat) * PVHIP_COMPONENTS_MAX_PER_IMAGE <= 64 * 1024, "the statistics launch sets no LDS attribute");

__device__ __forceinline__ void stat_add(int* rect, unsigned long long* sum, unsigned long long* m, const Stat& s) {   // (LDS or global)
    atomicMin(rect + 0, s.x0);
    atomicMin(rect + 1, s.y0);
    atomicMax(rect + 2, s.x1);
    atomicMax(rect + 3, s.y1);
    atomicAdd(sum, s.sum);
#pragma unroll
    for (int i = 0; i < 5; ++i) atomicAdd(m + i, s.m[i]);
}

// A trip is kBlock consecutive pixels; workgroup b takes the trips [b * per_block, (b + 1) * per_block) and keeps the statistics of one
// image, `held`, in LDS between them.
__global__ __launch_bounds__(kBlock) void components_stats_kernel(const unsigned* __restrict__ x, Plan a, const int* __restrict__ parent,
                                                                  const int* __restrict__ area, const unsigned* __restrict__ peak,
                                                                  long long trips, int per_block, Table t) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    Stat* table = reinterpret_cast<Stat*>(lds);
    const int lane = threadIdx.x & (kWave - 1);
    auto flush = [&](int r) {                                           // (every thread of the workgroup: `r` is the same in all)
        __syncthreads();
        for (int k = threadIdx.x; k < a.keep; k += kBlock) {
            Stat& s = table[k];
            if (r >= 0 && s.x1 >= 0) {
                const size_t at = (size_t)r * a.keep + k;
                stat_add(t.rects + 4 * at, t.sums + at, t.moments + 5 * at, s);
            }
            s.x0 = a.w; s.y0 = a.h; s.x1 = -1; s.y1 = -1; s.sum = 0ull;
#pragma unroll
            for (int i = 0; i < 5; ++i) s.m[i] = 0ull;
        }
        __syncthreads();
    };
    int held = -1;
    const long long first_trip = (long long)blockIdx.x * per_block;
    const long long last_trip  = first_trip + per_block < trips ? first_trip + per_block : trips;
    for (long long trip = first_trip; trip < last_trip; ++trip) {      // (the same trips in every thread of the workgroup)
        const int r0 = (int)fdiv((unsigned)(trip * kBlock), a.by_size);
        if (r0 != held) {
            flush(held);
            held = r0;
        }
        const long long g = trip * kBlock + threadIdx.x;
        int id = -1, rank = -1, r = 0;
        Stat s{a.w, a.h, -1, -1, 0ull, {0ull, 0ull, 0ull, 0ull, 0ull}};
        if (g < a.total) {
            const int root = parent[g];
            const int mark = root >= 0 ? area[root] : 0;
            if (mark < 0) {
                rank = -mark - 1;
                id = root;
                r = (int)fdiv((unsigned)g, a.by_size);
                const unsigned p = (unsigned)g - (unsigned)r * (unsigned)a.size;
                const unsigned y = fdiv(p, a.by_w), xx = p - y * (unsigned)a.w;
                const unsigned bits = x[((size_t)r * a.k + a.channel) * (size_t)a.size + p];
                if (order_of(bits) == kZeroWord && peak[root] == kZeroWord)
                    atomicMin(t.zeros + (size_t)r * a.keep + rank, (int)((p << 1) | (bits >> 31)));
                double v = (double)__uint_as_float(bits);
                v = v < -32768.0 ? -32768.0 : (v > 32768.0 ? 32768.0 : v);
                s.x0 = s.x1 = (int)xx;
                s.y0 = s.y1 = (int)y;
                s.sum  = (unsigned long long)__double2ll_rn(v * 65536.0);
                s.m[0] = xx;
                s.m[1] = y;
                s.m[2] = (unsigned long long)xx * xx;
                s.m[3] = (unsigned long long)xx * y;
                s.m[4] = (unsigned long long)y * y;
            }
        }
        const unsigned long long heads = run_heads(id, lane);
        auto least = [](int u, int v) { return u < v ? u : v; };
        auto most  = [](int u, int v) { return u > v ? u : v; };
        auto plus  = [](unsigned long long u, unsigned long long v) { return u + v; };
        s.x0  = run_reduce(s.x0, heads, lane, least);
        s.x1  = run_reduce(s.x1, heads, lane, most);
        s.y1  = run_reduce(s.y1, heads, lane, most);              // (y0: a run stands in flat order, its first lane has its least y)
        s.sum = run_reduce(s.sum, heads, lane, plus);
#pragma unroll
        for (int i = 0; i < 5; ++i) s.m[i] = run_reduce(s.m[i], heads, lane, plus);
        if (((heads >> lane) & 1ull) && rank >= 0) {
            if (r == held) {
                Stat& cell = table[rank];
                stat_add(&cell.x0, &cell.sum, cell.m, s);
            } else {                                                    // the pixels of a trip behind the seam of two images
                const size_t at = (size_t)r * a.keep + rank;
                stat_add(t.rects + 4 * at, t.sums + at, t.moments + 5 * at, s);
            }
        }
    }
    flush(held);
}

bool components_shape(int n, int k, int h, int w) {
    if (n < 1 || k < 1 || k > PVHIP_COMPONENTS_MAX_PLANES || h < 1 || w < 1) return false;
    const long long size = (long long)h * w;
    return size >= 2 && size <= PVHIP_COMPONENTS_MAX_PLANE && (long long)n * size < (1LL << 31);
}

}  // namespace

extern "C" {

unsigned long long pvhip_components_scratch_bytes(int n, int h, int w, int max_per_image) {
    if (!components_shape(n, 1, h, w) || max_per_image < 1 || max_per_image > PVHIP_COMPONENTS_MAX_PER_IMAGE) return 0ull;
    return 12ull * (unsigned long long)n * (unsigned long long)h * (unsigned long long)w;
}

int pvhip_components_f32(const float* x, int n, int k, int h, int w, int channel, int connectivity, float min_score, int min_area,
                         int max_per_image, void* scratch, int* counts, int* found, int* seeds, int* areas, float* peaks, int* zeros,
                         int* rects, long long* sums, long long* moments) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(x != nullptr && scratch != nullptr && counts != nullptr && found != nullptr && seeds != nullptr && areas != nullptr &&
                    peaks != nullptr && zeros != nullptr && rects != nullptr && sums != nullptr && moments != nullptr);
    PVHIP_CHECK_ARG(((uintptr_t)x & 3u) == 0 && ((uintptr_t)scratch & 15u) == 0 && ((uintptr_t)counts & 3u) == 0 && ((uintptr_t)found & 3u) == 0 &&
                    ((uintptr_t)seeds & 3u) == 0 && ((uintptr_t)areas & 3u) == 0 && ((uintptr_t)peaks & 3u) == 0 && ((uintptr_t)zeros & 3u) == 0 &&
                    ((uintptr_t)rects & 3u) == 0 && ((uintptr_t)sums & 7u) == 0 && ((uintptr_t)moments & 7u) == 0);
    PVHIP_CHECK_ARG(n >= 1 && k >= 1 && h >= 1 && w >= 1);
    PVHIP_CHECK_ARG(k <= PVHIP_COMPONENTS_MAX_PLANES);
    PVHIP_CHECK_ARG(components_shape(n, k, h, w));                              // 2 <= h * w <= 2^24, n * h * w < 2^31
    PVHIP_CHECK_ARG(channel >= -k && channel < k);
    PVHIP_CHECK_ARG(connectivity == 4 || connectivity == 8);
    PVHIP_CHECK_ARG(min_score - min_score == 0.0f);                             // finite
    PVHIP_CHECK_ARG(min_area >= 1 && min_area <= PVHIP_COMPONENTS_MAX_PLANE);
    PVHIP_CHECK_ARG(max_per_image >= 1 && max_per_image <= PVHIP_COMPONENTS_MAX_PER_IMAGE);
    unsigned min_bits;
    __builtin_memcpy(&min_bits, &min_score, sizeof min_bits);
    const unsigned mag = min_bits & 0x7FFFFFFFu;                                // the order word of pvhip_topk_keys.h, of a finite value
    const unsigned min_word = mag == 0u ? 0x80000000u : ((min_bits & 0x80000000u) ? ~min_bits : (min_bits | 0x80000000u));
    const int size = h * w;
    Plan a{n, k, h, w, size, channel < 0 ? channel + k : channel, connectivity == 8 ? 1 : 0, min_word, min_area, max_per_image,
           (w + kCols - 1) / kCols, (h + kRows - 1) / kRows, (long long)n * size, make_fastdiv((unsigned)size), make_fastdiv((unsigned)w)};
    int*      parent = static_cast<int*>(scratch);
    int*      area   = parent + a.total;
    unsigned* peak   = reinterpret_cast<unsigned*>(area + a.total);
    const unsigned* bits = reinterpret_cast<const unsigned*>(x);
    const Table t{counts, found, seeds, areas, reinterpret_cast<unsigned*>(peaks), zeros, rects,
                  reinterpret_cast<unsigned long long*>(sums), reinterpret_cast<unsigned long long*>(moments)};
    const size_t lds = sizeof(Stat) * (size_t)max_per_image;
    hipStream_t stream = state().stream;
    const long long tiles = (long long)n * a.tiles_x * a.tiles_y;               // (n * h * w < 2^31: below 2^31 tiles)
    hipLaunchKernelGGL(components_tiles_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, stream, bits, a, parent, area, peak);
    PVHIP_LAUNCH_CHECK();
    const long long per_image = (long long)(a.tiles_y - 1) * w + (long long)(a.tiles_x - 1) * h;
    if (per_image > 0) {
        const long long items = per_image * n;
        hipLaunchKernelGGL(components_seams_kernel, dim3((unsigned)grid_for((size_t)items)), dim3(kBlock), 0, stream, a, parent, items, (int)per_image);
        PVHIP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(components_flatten_kernel, dim3((unsigned)grid_for((size_t)a.total)), dim3(kBlock), 0, stream, bits, a, parent, area, peak);
    PVHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(components_select_kernel, dim3((unsigned)(n < kMaxBlocks * 4 ? n : kMaxBlocks * 4)), dim3(kBlock), 0, stream, a, parent,
                       area, peak, t);
    PVHIP_LAUNCH_CHECK();
    const long long trips = (a.total + kBlock - 1) / kBlock;
    const int per_block = (int)((trips + kNumCU * 4 - 1) / (kNumCU * 4));       // a bounded grid: a table is flushed once per workgroup and image
    hipLaunchKernelGGL(components_stats_kernel, dim3((unsigned)((trips + per_block - 1) / per_block)), dim3(kBlock), lds, stream, bits, a,
                       parent, area, peak, trips, per_block, t);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
