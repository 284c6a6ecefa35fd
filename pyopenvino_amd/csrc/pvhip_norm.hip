// SoftMax (row-wise, wave-shuffle reductions), cross-channel LRN (register sliding window), and the launches that fuse LRN with a 3x3
// MaxPool: LRN -> MaxPool, MaxPool -> LRN and MaxPool -> LRN -> 1x1 convolution.  The fused kernels are assembled from parts that exist
// once: the band of a workgroup (LrnBand), the pooling geometry of an owned output (PoolTap, pool3x3_from_lds), the LRN arithmetic
// (lrn_value, ChannelWindow) and the raw-plane walk of the MaxPool-first kernels (pooled_lrn_walk); on the host, one plan
// (plan_lrn_pool) that says what will be launched.
#include <type_traits>

#include "pvhip_common.h"

using namespace pvhip;

namespace {

// Global accesses of the LRN / pooling streams are NONTEMPORAL: every element is read once and written once, and on this chip a 16-byte
// stream with nt loads and stores runs at 6.0-6.4 TB/s against 5.1-5.4 plain (profiles/r03_stream_sweep.md).  One switch for A/B builds.
constexpr bool kStreamNT = true;
template <class T>
__device__ __forceinline__ T ldnt(const T* p) { return kStreamNT ? __builtin_nontemporal_load(p) : *p; }
template <class T>
__device__ __forceinline__ void stnt(T* p, T v) { if (kStreamNT) __builtin_nontemporal_store(v, p); else *p = v; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// One workgroup per row: exp once into registers (cols <= kBlock * kPerThread) or recompute.
// y = exp(x) / sum(exp(x)) with no max shift, exactly the reference expression (SoftMax.py:12-13).
constexpr int kSoftmaxPerThread = 8;

__global__ __launch_bounds__(kBlock) void softmax_rows_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                               int rows, int cols) {
    __shared__ float wave_part[kBlock / kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wid  = threadIdx.x / kWave;
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* __restrict__ xr = x + (size_t)r * cols;
        float* __restrict__       yr = y + (size_t)r * cols;
        float e[kSoftmaxPerThread];
        float part = 0.0f;
        const bool in_regs = cols <= kBlock * kSoftmaxPerThread;
        if (in_regs) {
#pragma unroll
            for (int j = 0; j < kSoftmaxPerThread; ++j) {
                const int c = threadIdx.x + j * kBlock;
                e[j]        = (c < cols) ? expf(xr[c]) : 0.0f;
                part += e[j];
            }
        } else {
            for (int c = threadIdx.x; c < cols; c += kBlock) part += expf(xr[c]);
        }
        part = wave_sum(part);
        __syncthreads();  // wave_part free from the previous row
        if (lane == 0) wave_part[wid] = part;
        __syncthreads();
        float total = 0.0f;
#pragma unroll
        for (int wv = 0; wv < kBlock / kWave; ++wv) total += wave_part[wv];
        if (in_regs) {
#pragma unroll
            for (int j = 0; j < kSoftmaxPerThread; ++j) {
                const int c = threadIdx.x + j * kBlock;
                if (c < cols) yr[c] = e[j] / total;
            }
        } else {
            for (int c = threadIdx.x; c < cols; c += kBlock) yr[c] = expf(xr[c]) / total;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The LRN arithmetic, ONCE: the squares of window[0 .. SIZE) summed in ascending channel order, the order np.sum(axis=1) uses
// (LRN.py:19), then centre / (bias + alpha * sum)^beta.  Every kernel below -- the plain one and the three fused ones -- calls this, on
// one float or on the VEC pixels of a lane: that is what makes every fused form carry the bits of the separate launches.
template <int VEC>
using lrn_vec = float __attribute__((ext_vector_type(VEC)));
constexpr int kLrnT = 8;      // channels per chunk of the channel walks (C must be a multiple)

template <int SIZE, int BETA_MODE, class V>
__device__ __forceinline__ V lrn_value(const V* window, V centre, float alpha, float beta, float bias) {
    V s = window[0] * window[0];
#pragma unroll
    for (int q = 1; q < SIZE; ++q) s = s + window[q] * window[q];
    if constexpr (std::is_same<V, float>::value) {
        return lrn_div(centre, bias + alpha * s, beta, BETA_MODE);
    } else {
        V o;
#pragma unroll
        for (int v = 0; v < (int)(sizeof(V) / sizeof(float)); ++v) o[v] = lrn_div(centre[v], bias + alpha * s[v], beta, BETA_MODE);
        return o;
    }
}

// The last SIZE values of one pixel along the channel axis (channels outside the tensor are an exact 0): after push(v) of channel ch
// the window is centred on channel ch - SIZE / 2.
template <int SIZE>
struct ChannelWindow {
    float v[SIZE];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int q = 0; q < SIZE; ++q) v[q] = 0.0f;
    }
    __device__ __forceinline__ void push(float x) {
#pragma unroll
        for (int q = 0; q + 1 < SIZE; ++q) v[q] = v[q + 1];
        v[SIZE - 1] = x;
    }
};

// One lane owns VEC adjacent pixels of one image and walks the channel axis in chunks of T = 8 channels
// (C must be a multiple of 8; other channel counts take the generic kernel).  The T loads of chunk k+1 are
// issued before the outputs that chunk k completes are computed, so T independent 16-byte loads per lane are
// in flight; every element is read once and written once.  After chunk k has landed the computable outputs
// are channels [T*k - HALF, T*k + T - HALF).  The loop body is branch-free: the first chunk, the last chunk and
// the trailing HALF outputs are peeled.  Window for channel c is [c - SIZE/2, c + SIZE/2] clipped to [0, C);
// channels outside the tensor contribute an exact 0.
// (This walk and lrn_maxpool3x3_kernel's are the same skeleton written twice: as ONE inline function with the store as a sink it cost
// registers in both kernels, profiles/norm_refactor.md.)
template <int SIZE, int VEC, int BETA_MODE>
__global__ __launch_bounds__(kBlock) void lrn_window_kernel(const float* __restrict__ x, float* __restrict__ y, int n,
                                                             int c, int hw, float alpha, float beta, float bias) {
    constexpr int HALF = SIZE / 2;
    constexpr int T    = kLrnT;
    constexpr int E    = 2 * HALF + T;      // ext[]: channels [T*k - 2*HALF, T*k + T)
    static_assert(2 * HALF <= T, "window halo must fit in one chunk");
    typedef lrn_vec<VEC> vec_t;
    const int      cols_per_img = hw / VEC;
    const unsigned total        = (unsigned)n * (unsigned)cols_per_img;
    const unsigned stride       = gridDim.x * blockDim.x;
    const int      n_chunks     = c / T;
    const size_t   cstride      = (size_t)hw / VEC;   // channel stride in vec_t units

    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const unsigned img  = t / (unsigned)cols_per_img;
        const unsigned col  = t - img * (unsigned)cols_per_img;
        const size_t   base = (size_t)img * c * hw + (size_t)col * VEC;
        const vec_t* __restrict__ xv = reinterpret_cast<const vec_t*>(x + base);
        vec_t* __restrict__       yv = reinterpret_cast<vec_t*>(y + base);
        vec_t ext[E], nxt[T];
        // one output: centre ext[j + HALF], window ext[j .. j + SIZE)
        auto norm = [&](const vec_t* w) { return lrn_value<SIZE, BETA_MODE>(w, w[HALF], alpha, beta, bias); };
        auto put  = [&](vec_t o, int ch) { stnt(yv + (size_t)ch * cstride, o); };
#pragma unroll
        for (int j = 0; j < 2 * HALF; ++j) ext[j] = (vec_t)(0.0f);
#pragma unroll
        for (int j = 0; j < T; ++j) ext[2 * HALF + j] = ldnt(xv + (size_t)j * cstride);
        // chunks 0 .. n_chunks-2: prefetch the next chunk, emit what this one completes
        for (int k = 0; k + 1 < n_chunks; ++k) {
            const vec_t* __restrict__ xn = xv + (size_t)(k + 1) * T * cstride;
#pragma unroll
            for (int j = 0; j < T; ++j) nxt[j] = ldnt(xn + (size_t)j * cstride);
            if (k == 0) {
#pragma unroll
                for (int j = HALF; j < T; ++j) put(norm(ext + j), j - HALF);
            } else {
                const int ch0 = k * T - HALF;
#pragma unroll
                for (int j = 0; j < T; ++j) put(norm(ext + j), ch0 + j);
            }
#pragma unroll
            for (int j = 0; j < 2 * HALF; ++j) ext[j] = ext[T + j];
#pragma unroll
            for (int j = 0; j < T; ++j) ext[2 * HALF + j] = nxt[j];
        }
        // last chunk (no prefetch), then the trailing HALF channels whose windows run past the tensor
        {
            const int k = n_chunks - 1, ch0 = k * T - HALF;
            if (k == 0) {
#pragma unroll
                for (int j = HALF; j < T; ++j) put(norm(ext + j), j - HALF);
            } else {
#pragma unroll
                for (int j = 0; j < T; ++j) put(norm(ext + j), ch0 + j);
            }
#pragma unroll
            for (int j = 0; j < 2 * HALF; ++j) ext[j] = ext[T + j];
#pragma unroll
            for (int j = 0; j < T; ++j) ext[2 * HALF + j] = (vec_t)(0.0f);
#pragma unroll
            for (int j = 0; j < HALF; ++j) put(norm(ext + j), c - HALF + j);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The fused LRN / 3x3 MaxPool kernels.  A workgroup owns one image and a band of pooled rows; its input band (the rows those windows
// touch, full width) is one dense run per channel plane, one lane per VEC adjacent pixels of it, and a chunk of T = 8 channel planes
// of the band lies in LDS ([T][plane_l]) while the workgroup pools out of it.
struct LrnPoolArgs {
    const float* x;
    float*       y;
    int   n, c, h, w, oh, ow;
    int   pt, pl, hp, wp;
    int   band_rows, n_bands;
    int   plane_l;               // floats per normalised plane in LDS
    float alpha, beta, bias;
    int   pool4;                 // lrn_maxpool3x3_kernel: a lane pools FOUR adjacent outputs of a row (stride 2, no padding on top / left, ow % 4 == 0), the planes dealt over the waves
    int   abl;                   // diagnostic build (PVHIP_CONV_ABLATE bits, wrong results): 1 no LRN arithmetic, 2 no pooling, 4 no stores, 8 loads hit L2
};

// What a workgroup and a lane own of the input: the band prologue of the three fused kernels.
struct LrnBand {
    int    img;                  // the image
    int    oy0, rows_t;          // first pooled row of the band, pooled rows in it (the last band may be short)
    int    iy_lo;                // first input row of the band
    int    hw, ohw;
    int    out_pp;               // pooled outputs per plane and full band
    bool   active;               // this lane owns VEC pixels of the input band
    size_t cstride;              // channel stride of the input in units of VEC floats
    const float* x0;             // the lane's pixels in channel 0 of the image
    float* mine;                 // ... and their place in LDS plane 0
};

template <int ST, int VEC>
__device__ __forceinline__ LrnBand lrn_band(const LrnPoolArgs& a, const FastDiv& d_bands, float* planes) {
    LrnBand b;
    const int tid = threadIdx.x;
    b.img = (int)fdiv(blockIdx.x, d_bands);
    const int band = (int)blockIdx.x - b.img * a.n_bands;
    b.oy0 = band * a.band_rows;
    const int oy1 = min(a.oh, b.oy0 + a.band_rows);
    b.rows_t = oy1 - b.oy0;
    b.iy_lo  = max(0, b.oy0 * ST - a.pt);
    const int iy_hi   = min(a.h, (oy1 - 1) * ST + 3 - a.pt);
    const int band_px = (iy_hi - b.iy_lo) * a.w;
    b.hw = a.h * a.w, b.ohw = a.oh * a.ow;
    b.active  = tid * VEC < band_px;
    b.cstride = (size_t)b.hw / VEC;
    b.x0      = a.x + (size_t)b.img * a.c * b.hw + (size_t)b.iy_lo * a.w + (b.active ? tid * VEC : 0);
    b.mine    = planes + tid * VEC;
    b.out_pp  = a.band_rows * a.ow;
    return b;
}

// Pooling geometry of ONE owned output, computed ONCE per lane: a lane owns the same output pixels of the band in every plane of every
// chunk (the first version redid two divisions, six clamps and the pad tests per output, plane and chunk: ~60 vector instructions per
// output against ~15 of LRN arithmetic per four inputs -- the kernel ran at 3.6 TB/s, VALU-bound).  Nine LDS byte offsets (taps outside
// the tensor clamped onto a tap inside the same window), the output offset in its plane, and whether the window touches zero-pad cells
// (then max(m, 0)).  rem: the output's index in the band.
struct PoolTap {
    unsigned tap[9];
    unsigned outo;
    bool     live, zpad;
};
// The NI owned outputs of a lane, field by field, each filled from the PoolTap that pool_tap() returns.  lrn_maxpool3x3_kernel, whose
// pooling lambdas capture this struct, copies the fields in its own body instead of calling set(): any function that is handed the
// captured struct to fill took up to twelve registers more there (164 against 155 in <5, 4, 4, 2, 1>; profiles/norm_refactor.md).
template <int NI>
struct PoolTaps {
    unsigned tap[NI][9];
    unsigned outo[NI];
    bool     live[NI], zpad[NI];
    __device__ __forceinline__ void set(int i, const PoolTap& o) {
#pragma unroll
        for (int q = 0; q < 9; ++q) tap[i][q] = o.tap[q];
        outo[i] = o.outo, live[i] = o.live, zpad[i] = o.zpad;
    }
};

template <int ST>
__device__ __forceinline__ PoolTap pool_tap(const LrnPoolArgs& a, const LrnBand& b, unsigned rem, const FastDiv& d_ow) {
    PoolTap t;
    const unsigned oyl = fdiv(rem, d_ow), ox = rem - oyl * (unsigned)a.ow;
    t.live = (int)rem < b.out_pp && (int)oyl < b.rows_t;
    const int oy = b.oy0 + (int)oyl;
    const int py0 = oy * ST - a.pt, px0 = (int)ox * ST - a.pl;
    const int c0 = min(max(px0, 0), a.w - 1), c1 = min(max(px0 + 1, 0), a.w - 1), c2 = min(max(px0 + 2, 0), a.w - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int r = (min(max(py0 + k, 0), a.h - 1) - b.iy_lo) * a.w;
        t.tap[3 * k + 0] = t.live ? (unsigned)(r + c0) * 4u : 0u;
        t.tap[3 * k + 1] = t.live ? (unsigned)(r + c1) * 4u : 0u;
        t.tap[3 * k + 2] = t.live ? (unsigned)(r + c2) * 4u : 0u;
    }
    const bool zc = (px0 < 0) || (min((int)ox * ST + 2, a.wp - 1) - a.pl >= a.w);
    const bool zr = (py0 < 0) || (min(oy * ST + 2, a.hp - 1) - a.pt >= a.h);
    t.zpad = zc || zr;
    t.outo = (unsigned)(oy * a.ow) + ox;
    return t;
}

// The 3x3 maximum of one output out of one LDS plane: nine reads, row maxima first; a NaN IS the maximum (max3_nan), as for np.max --
// the rules of maxpool3x3_cols_kernel.
template <int NI>
__device__ __forceinline__ float pool3x3_from_lds(const char* plane, const PoolTaps<NI>& t, int i) {
    float h[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v0 = *reinterpret_cast<const float*>(plane + t.tap[i][3 * k + 0]);
        const float v1 = *reinterpret_cast<const float*>(plane + t.tap[i][3 * k + 1]);
        const float v2 = *reinterpret_cast<const float*>(plane + t.tap[i][3 * k + 2]);
        h[k] = max3_nan(v0, v1, v2);
    }
    const float m = max3_nan(h[0], h[1], h[2]);
    return t.zpad[i] ? max3_nan(m, 0.0f, 0.0f) : m;
}

// ---------------------------------------------------------------------------------------------------------------
// LRN followed by a 3x3 MaxPool (GoogLeNet's conv2/norm2 -> pool2/3x3_s2) in ONE pass over the input: the LRN
// tensor (1.2 GB of traffic at batch 256: written once, read once) never exists.
//
// The workgroup walks the channel axis exactly like lrn_window_kernel -- chunks of T = 8 channels, the loads of chunk k+1 in flight while
// chunk k is normalised -- but the normalised values of a chunk go to LDS plane `slot` instead of HBM, and at the end of a chunk, after a
// barrier, the workgroup pools those planes (9 LDS reads per output, or pool4) and stores n_pl x band_rows x ow outputs.  The LRN
// arithmetic is lrn_window_kernel's (lrn_value), so the result carries the bits of the two separate launches.
template <int SIZE, int VEC, int BETA_MODE, int ST, int NI>     // NI: pooled outputs of a band and plane per lane (ceil(band_rows * ow / 256))
__global__ __launch_bounds__(kBlock) void lrn_maxpool3x3_kernel(LrnPoolArgs a, FastDiv d_bands, FastDiv d_ow) {
    constexpr int HALF = SIZE / 2;
    constexpr int T    = kLrnT;
    constexpr int E    = 2 * HALF + T;
    static_assert(2 * HALF <= T, "window halo must fit in one chunk");
    typedef lrn_vec<VEC> vec_t;
    extern __shared__ __attribute__((aligned(16))) float planes[];   // [T][plane_l]
#ifdef PVHIP_DIAG
    const int abl = a.abl;          // scripts/time_lrnpool_abl.py: parts switched off
#else
    constexpr int abl = 0;
#endif
    const int tid = threadIdx.x;
    const LrnBand b = lrn_band<ST, VEC>(a, d_bands, planes);
    PoolTaps<NI> t;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const PoolTap o = pool_tap<ST>(a, b, (unsigned)(tid + i * kBlock), d_ow);     // copied HERE, not by t.set(): see PoolTaps
#pragma unroll
        for (int q = 0; q < 9; ++q) t.tap[i][q] = o.tap[q];
        t.outo[i] = o.outo, t.live[i] = o.live, t.zpad[i] = o.zpad;
    }
    float* const yimg = a.y + (size_t)b.img * a.c * b.ohw;
    const char* const planes_b = reinterpret_cast<const char*>(planes);
    const unsigned plane_bytes = (unsigned)a.plane_l * 4u;
    const int      n_chunks    = a.c / T;

    // ---- the same pooling with FOUR adjacent outputs of a row per lane (round 5; a.pool4): their windows are nine columns of three rows -- two 16-byte
    // and one 4-byte LDS read per row instead of 36 4-byte ones, sixteen v_maximum3_f32 as before, ONE 16-byte store instead of four 4-byte ones; the
    // quads of a band fit one wave's lanes (rows_t x ow / 4 <= 64), so the planes of a chunk are dealt over the four waves (plane p: wave p % 4).
    // A different read pattern from PoolTap's, so a path of its own; the band is the same LrnBand.
    unsigned p4_row[3] = {0u, 0u, 0u}, p4_c8 = 0u, p4_out = 0u, p4_z = 0u;
    bool     p4_live = false;
    const int wv4 = tid >> 6;
    if constexpr (VEC == 4 && ST == 2) {
        if (a.pool4 != 0) {
            const int ql = tid & 63, qpr = a.ow >> 2;
            const int oyl = ql / qpr, oxq = ql - oyl * qpr;
            p4_live = oyl < b.rows_t;
            const int oy = b.oy0 + (p4_live ? oyl : 0);
            const int py0 = oy * ST, c0 = 8 * oxq;                    // (pt = pl = 0)
#pragma unroll
            for (int k = 0; k < 3; ++k) p4_row[k] = (unsigned)((min(py0 + k, a.h - 1) - b.iy_lo) * a.w + c0) * 4u;
            p4_c8 = (unsigned)(min(c0 + 8, a.w - 1) - c0) * 4u;        // the ninth column, clamped into the window (a duplicate does not change a maximum)
            const bool zr = min(oy * ST + 2, a.hp - 1) >= a.h;
#pragma unroll
            for (int j = 0; j < 4; ++j) p4_z |= ((zr || min((4 * oxq + j) * ST + 2, a.wp - 1) >= a.w) ? 1u : 0u) << j;
            p4_out = (unsigned)(oy * a.ow + 4 * oxq);
        }
    }
    auto pool4 = [&](int n_pl, int ch0) {
        __syncthreads();
        if (p4_live && !(abl & 2)) {
            typedef float f4_t __attribute__((ext_vector_type(4)));
            for (int p = wv4; p < n_pl; p += 4) {
                const char* const pb = reinterpret_cast<const char*>(planes) + (unsigned)p * ((unsigned)a.plane_l * 4u);
                float hm[3][4];                  // row maxima of the four windows: a NaN IS the maximum (max3_nan), as for np.max
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const f4_t lo = *reinterpret_cast<const f4_t*>(pb + p4_row[k]), hi = *reinterpret_cast<const f4_t*>(pb + p4_row[k] + 16);
                    const float c8 = *reinterpret_cast<const float*>(pb + p4_row[k] + p4_c8);
                    hm[k][0] = max3_nan(lo[0], lo[1], lo[2]);
                    hm[k][1] = max3_nan(lo[2], lo[3], hi[0]);
                    hm[k][2] = max3_nan(hi[0], hi[1], hi[2]);
                    hm[k][3] = max3_nan(hi[2], hi[3], c8);
                }
                f4_t m;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float mj = max3_nan(hm[0][j], hm[1][j], hm[2][j]);
                    m[j] = ((p4_z >> j) & 1u) ? max3_nan(mj, 0.0f, 0.0f) : mj;
                }
                if (!(abl & 4)) *reinterpret_cast<f4_t*>(a.y + (size_t)b.img * a.c * (a.oh * a.ow) + (size_t)(ch0 + p) * (a.oh * a.ow) + p4_out) = m;
            }
        }
        __syncthreads();
    };
    // pool the first n_pl planes of LDS into channels [ch0, ch0 + n_pl)
    auto pool = [&](int n_pl, int ch0) {
        if constexpr (VEC == 4 && ST == 2) {
            if (a.pool4 != 0) { pool4(n_pl, ch0); return; }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (!t.live[i] || (abl & 2)) continue;
            float* yo = yimg + (size_t)ch0 * b.ohw + t.outo[i];
            unsigned pb = 0u;
            for (int p = 0; p < n_pl; ++p, pb += plane_bytes, yo += b.ohw) {
                const float m = pool3x3_from_lds(planes_b + pb, t, i);
                // PLAIN stores: a lane writes one float per plane, 896-byte runs per plane and band -- nontemporal stores of such pieces
                // cost 4 % here and 9 % in maxpool3x3_lrn_kernel (the dense 16-byte runs of the MaxPool kernel are the opposite case)
                if (!(abl & 4)) *yo = m;
            }
        }
        __syncthreads();
    };

    // ---- the channel walk of lrn_window_kernel, with LDS plane `slot` as the destination and the pooling at the end of each chunk
    const vec_t* __restrict__ xv = reinterpret_cast<const vec_t*>(b.x0);
    vec_t ext[E], nxt[T];
    // normalise ext[j + HALF] with the window ext[j .. j + SIZE) into LDS plane slot
    auto norm   = [&](const vec_t* w) { return (abl & 1) ? w[HALF] : lrn_value<SIZE, BETA_MODE>(w, w[HALF], a.alpha, a.beta, a.bias); };
    auto to_lds = [&](vec_t o, int slot) { if (b.active) *reinterpret_cast<vec_t*>(b.mine + slot * a.plane_l) = o; };
#pragma unroll
    for (int j = 0; j < 2 * HALF; ++j) ext[j] = (vec_t)(0.0f);
#pragma unroll
    for (int j = 0; j < T; ++j) ext[2 * HALF + j] = ldnt(xv + (size_t)j * b.cstride);
    for (int k = 0; k + 1 < n_chunks; ++k) {
        const vec_t* __restrict__ xn = xv + (size_t)((abl & 8) ? 0 : (k + 1) * T) * b.cstride;        // abl 8: the first chunk again (L2 hits)
#pragma unroll
        for (int j = 0; j < T; ++j) nxt[j] = ldnt(xn + (size_t)j * b.cstride);
        if (k == 0) {
#pragma unroll
            for (int j = HALF; j < T; ++j) to_lds(norm(ext + j), j - HALF);
            pool(T - HALF, 0);
        } else {
#pragma unroll
            for (int j = 0; j < T; ++j) to_lds(norm(ext + j), j);
            pool(T, k * T - HALF);
        }
#pragma unroll
        for (int j = 0; j < 2 * HALF; ++j) ext[j] = ext[T + j];
#pragma unroll
        for (int j = 0; j < T; ++j) ext[2 * HALF + j] = nxt[j];
    }
    {
        const int k = n_chunks - 1;
        if (k == 0) {
#pragma unroll
            for (int j = HALF; j < T; ++j) to_lds(norm(ext + j), j - HALF);
            pool(T - HALF, 0);
        } else {
#pragma unroll
            for (int j = 0; j < T; ++j) to_lds(norm(ext + j), j);
            pool(T, k * T - HALF);
        }
#pragma unroll
        for (int j = 0; j < 2 * HALF; ++j) ext[j] = ext[T + j];
#pragma unroll
        for (int j = 0; j < T; ++j) ext[2 * HALF + j] = (vec_t)(0.0f);
#pragma unroll
        for (int j = 0; j < HALF; ++j) to_lds(norm(ext + j), j);
        pool(HALF, a.c - HALF);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// A new pooled value v of channel ch enters the window w of the owned output at offset outo of its plane; the window is then centred on
// channel ch - SIZE / 2, whose normalised value goes to sink(outo, value, channel).  (A free function, not a lambda of the walk below: a
// closure that captures the windows -- register arrays -- doubled maxpool3x3_lrn_kernel's registers at NI = 2, profiles/norm_refactor.md.)
template <int SIZE, int BETA_MODE, class Sink>
__device__ __forceinline__ void push_pooled(ChannelWindow<SIZE>& w, const LrnPoolArgs& a, unsigned outo, float v, int ch, Sink&& sink) {
    w.push(v);
    if (ch >= SIZE / 2) sink(outo, lrn_value<SIZE, BETA_MODE>(w.v, w.v[SIZE / 2], a.alpha, a.beta, a.bias), ch - SIZE / 2);
}

// The other order, MaxPool then LRN: the RAW planes of a chunk of 8 channels go to LDS (the loads of chunk k+1 in flight meanwhile), every
// lane pools its own NI output pixels out of them, and the pooled values of consecutive channels ARE the stream the LRN window slides
// over: SIZE of them in registers per owned pixel (ChannelWindow), the arithmetic of lrn_window_kernel.  The normalised value of the
// output at offset outo of its plane and channel ch goes to sink(outo, value, ch).  ALL_LANES: lanes without an output walk along (their
// taps read offset 0) instead of skipping the pooling -- for a sink in which every lane of the wave must take part.
// maxpool3x3_lrn_conv1x1_kernel walks this way (its sink is the MFMA); maxpool3x3_lrn_kernel keeps the loop written out, see there.
template <int SIZE, int VEC, int BETA_MODE, int NI, bool ALL_LANES, class Sink>
__device__ __forceinline__ void pooled_lrn_walk(const LrnPoolArgs& a, const LrnBand& b, const float* planes, const PoolTaps<NI>& t, Sink&& sink) {
    constexpr int HALF = SIZE / 2;
    constexpr int T    = kLrnT;
    typedef lrn_vec<VEC> vec_t;
    const vec_t* __restrict__ xv = reinterpret_cast<const vec_t*>(b.x0);
    const char* const planes_b = reinterpret_cast<const char*>(planes);
    const unsigned plane_bytes = (unsigned)a.plane_l * 4u;
    const int      n_chunks    = a.c / T;
    ChannelWindow<SIZE> win[NI];           // pooled values of channels ch - SIZE + 1 .. ch of the owned pixels
#pragma unroll
    for (int i = 0; i < NI; ++i) win[i].clear();
    vec_t cur[T], nxt[T];
#pragma unroll
    for (int j = 0; j < T; ++j) cur[j] = ldnt(xv + (size_t)j * b.cstride);
    for (int k = 0; k < n_chunks; ++k) {
        if (k + 1 < n_chunks) {
            const vec_t* __restrict__ xn = xv + (size_t)(k + 1) * T * b.cstride;
#pragma unroll
            for (int j = 0; j < T; ++j) nxt[j] = ldnt(xn + (size_t)j * b.cstride);
        }
        if (b.active) {
#pragma unroll
            for (int j = 0; j < T; ++j) *reinterpret_cast<vec_t*>(b.mine + j * a.plane_l) = cur[j];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (!ALL_LANES && !t.live[i]) continue;
            unsigned pb = 0u;
#pragma unroll
            for (int p = 0; p < T; ++p, pb += plane_bytes) push_pooled<SIZE, BETA_MODE>(win[i], a, t.outo[i], pool3x3_from_lds(planes_b + pb, t, i), k * T + p, sink);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < T; ++j) cur[j] = nxt[j];
    }
    // the trailing HALF channels: their windows run past the tensor (zeros)
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        if (!ALL_LANES && !t.live[i]) continue;
#pragma unroll
        for (int j = 0; j < HALF; ++j) push_pooled<SIZE, BETA_MODE>(win[i], a, t.outo[i], 0.0f, a.c + j, sink);
    }
}

// 3x3 MaxPool followed by LRN (GoogLeNet's pool1/3x3_s2 -> pool1/norm1) in ONE pass: the pooled tensor (411 MB at batch 256: written
// once, read once) never exists.  Same bands and same lane <-> input pixels as lrn_maxpool3x3_kernel, the loop of pooled_lrn_walk with
// "store the normalised value" in the place of the sink -- the bits of the two separate launches.  The loop is WRITTEN OUT here, with the
// windows as plain arrays and the push as a local macro: as a call of pooled_lrn_walk with a store sink this kernel's GoogLeNet launch
// took 0.180 - 0.191 ms against 0.175 and its NI = 2 instantiations 16 to 21 registers more (profiles/norm_refactor.md).
template <int SIZE, int VEC, int BETA_MODE, int ST, int NI>
__global__ __launch_bounds__(kBlock) void maxpool3x3_lrn_kernel(LrnPoolArgs a, FastDiv d_bands, FastDiv d_ow) {
    constexpr int HALF = SIZE / 2;
    constexpr int T    = kLrnT;
    typedef lrn_vec<VEC> vec_t;
    extern __shared__ __attribute__((aligned(16))) float planes[];   // [T][plane_l]
    const LrnBand b = lrn_band<ST, VEC>(a, d_bands, planes);
    const vec_t* __restrict__ xv = reinterpret_cast<const vec_t*>(b.x0);
    const int n_chunks = a.c / T;
    PoolTaps<NI> t;
#pragma unroll
    for (int i = 0; i < NI; ++i) t.set(i, pool_tap<ST>(a, b, (unsigned)(threadIdx.x + i * kBlock), d_ow));
    float* const yimg = a.y + (size_t)b.img * a.c * b.ohw;
    const char* const planes_b = reinterpret_cast<const char*>(planes);
    const unsigned plane_bytes = (unsigned)a.plane_l * 4u;

    float win[NI][SIZE];                   // pooled values of channels ch - SIZE + 1 .. ch of the owned pixels
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int q = 0; q < SIZE; ++q) win[i][q] = 0.0f;

    // a new pooled value v_ of channel ch_ enters the window; the window is then centred on channel ch_ - HALF (plain store: see lrn_maxpool3x3_kernel)
#define PV_PUSH_STORE(i_, v_, ch_)                                                             \
    {                                                                                          \
        _Pragma("unroll") for (int q = 0; q + 1 < SIZE; ++q) win[i_][q] = win[i_][q + 1];      \
        win[i_][SIZE - 1] = (v_);                                                              \
        if ((ch_) >= HALF)                                                                     \
            yimg[(size_t)((ch_) - HALF) * b.ohw + t.outo[i_]] = lrn_value<SIZE, BETA_MODE>(win[i_], win[i_][HALF], a.alpha, a.beta, a.bias); \
    }

    vec_t cur[T], nxt[T];
#pragma unroll
    for (int j = 0; j < T; ++j) cur[j] = ldnt(xv + (size_t)j * b.cstride);
    for (int k = 0; k < n_chunks; ++k) {
        if (k + 1 < n_chunks) {
            const vec_t* __restrict__ xn = xv + (size_t)(k + 1) * T * b.cstride;
#pragma unroll
            for (int j = 0; j < T; ++j) nxt[j] = ldnt(xn + (size_t)j * b.cstride);
        }
        if (b.active) {
#pragma unroll
            for (int j = 0; j < T; ++j) *reinterpret_cast<vec_t*>(b.mine + j * a.plane_l) = cur[j];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (!t.live[i]) continue;
            unsigned pb = 0u;
#pragma unroll
            for (int p = 0; p < T; ++p, pb += plane_bytes) {
                const float pooled = pool3x3_from_lds(planes_b + pb, t, i);
                PV_PUSH_STORE(i, pooled, k * T + p)
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < T; ++j) cur[j] = nxt[j];
    }
    // the trailing HALF channels: their windows run past the tensor (zeros)
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        if (!t.live[i]) continue;
#pragma unroll
        for (int j = 0; j < HALF; ++j) PV_PUSH_STORE(i, 0.0f, a.c + j)
    }
#undef PV_PUSH_STORE
}

// ---------------------------------------------------------------------------------------------------------------
// MaxPool 3x3 -> LRN -> 1x1 convolution (GoogLeNet's pool1/3x3_s2 -> pool1/norm1 -> conv2/3x3_reduce, 64 -> 64 channels, + bias + ReLU) in ONE
// pass (round 5): the LRN tensor (205 MB at batch 256: written once, read once by a convolution that runs at its byte bound, 0.098 ms) never
// exists either.  maxpool3x3_lrn_kernel already holds, lane by lane, the normalised value of ITS pixel for one channel after the other -- which is
// exactly the B operand of the k = 1 matrix instruction: v_mfma_f32_32x32x1_2b_f32 adds the outer product A (32 x 1) x B (1 x 32) of each of its two
// blocks, and block b's B is one value per lane of lanes 32 b .. 32 b + 31.  So a wave does, per input channel c and per 32 output channels,
// ONE MFMA with A = W[k][c] (a broadcast LDS read of the transposed weights, 16 KB) and B = what it would have stored: D[k][pixel] += W[k][c] *
// lrn[c][pixel], channel after channel in ascending order -- the reduction order of the pointwise kernel (the bits of the two launches).  No
// transposition, no staging of an operand tile, no barrier beyond the two the pooling has.  Epilogue: register v of block b at lane (j, h) is
// output channel 8 (v / 4) + 4 h + v % 4 of the pixel lane 32 b + j owns: that lane's output offset comes over once by a wave shuffle.
typedef float floatx32 __attribute__((ext_vector_type(32)));

struct PoolLrnConvArgs {
    LrnPoolArgs  p;           // the pooling / LRN geometry (p.y unused)
    const float* cw;          // (k_out, c, 1, 1)
    const float* cbias;       // k_out, or null
    float*       y;           // (n, k_out, oh, ow)
    int   k_out, act;
    float act_lo, act_hi;
};

template <int BETA_MODE, int ST, int KT>        // KT: 32-channel tiles of the convolution's output (k_out <= 32 KT)
__global__ __launch_bounds__(kBlock) void maxpool3x3_lrn_conv1x1_kernel(PoolLrnConvArgs ca, FastDiv d_bands, FastDiv d_ow) {
    constexpr int SIZE = 5, T = kLrnT, VEC = 4;
    extern __shared__ __attribute__((aligned(16))) float planes[];   // [T][plane_l], then the weights [c][32 KT]
    const LrnPoolArgs& a = ca.p;
    float* const wl = planes + T * a.plane_l;

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const LrnBand b = lrn_band<ST, VEC>(a, d_bands, planes);

    // the transposed weights: wl[c][k] = W[k][c], zeros past k_out
    for (int e = tid; e < a.c * 32 * KT; e += kBlock) {
        const int c = e / (32 * KT), k = e - c * (32 * KT);
        wl[e] = k < ca.k_out ? ca.cw[(size_t)k * a.c + c] : 0.0f;
    }

    PoolTaps<1> t;                                             // one output per lane
    t.set(0, pool_tap<ST>(a, b, (unsigned)tid, d_ow));
    if (!t.live[0]) t.outo[0] = 0xffffffffu;                         // a dead lane: the epilogue stores nothing for it
    const float* const wl_lane = wl + (lane & 31);
    floatx32 acc[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int r = 0; r < 32; ++r) acc[kt][r] = 0.0f;

    // the normalised value of channel ch -- what maxpool3x3_lrn_kernel stores -- is this lane's column of the outer product with that channel's
    // weights: one k = 1 MFMA per 32 output channels (every lane takes part: no branch; a dead lane contributes a zero column).  The pooled
    // value reaches the MFMA through max3_nan's builtin and plain C++ only: no inline asm on the way (stale MFMA operands, see max3_nan)
    pooled_lrn_walk<SIZE, VEC, BETA_MODE, 1, true>(a, b, planes, t, [&](unsigned, float v, int ch) {
        const float o = t.live[0] ? v : 0.0f;
        const float* const wc = wl_lane + ch * (32 * KT);
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) acc[kt] = __builtin_amdgcn_mfma_f32_32x32x1f32(wc[32 * kt], o, acc[kt], 0, 0, 0);
    });

    // ---- epilogue: acc[kt][16 b + v] at lane (j = lane & 31, h = lane >> 5) = output channel 32 kt + 8 (v / 4) + 4 h + v % 4 of the pixel of lane 32 b + j
    const int h2 = lane >> 5;
    unsigned outo_b[2];
    outo_b[0] = (unsigned)__shfl((int)t.outo[0], lane & 31, kWave);
    outo_b[1] = (unsigned)__shfl((int)t.outo[0], 32 + (lane & 31), kWave);
    float* const yimg = ca.y + (size_t)b.img * ca.k_out * b.ohw;
    const ActBounds ab = act_bounds(ca.act, ca.act_lo, ca.act_hi);
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
        float bv[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int kk = 32 * kt + 8 * (v >> 2) + 4 * h2 + (v & 3);
            bv[v] = (ca.cbias != nullptr && kk < ca.k_out) ? ca.cbias[kk] : 0.0f;
        }
#pragma unroll
        for (int bl = 0; bl < 2; ++bl) {
            float vv[16];
#pragma unroll
            for (int v = 0; v < 16; ++v) vv[v] = acc[kt][16 * bl + v];
            bias_act_n<16>(vv, bv, ca.cbias != nullptr, ca.act, ab);
            if (outo_b[bl] != 0xffffffffu) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int kk = 32 * kt + 8 * (v >> 2) + 4 * h2 + (v & 3);
                    if (kk < ca.k_out) yimg[(size_t)kk * b.ohw + outo_b[bl]] = vv[v];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// LRN -> 1x1 convolution (+ bias, activation) in ONE pass, for a tensor that is pooled already (the stem convolution's second output): the walk of
// lrn_window_kernel -- a lane owns ONE pixel and walks the channel axis in chunks of kLrnT, the loads of chunk k + 1 in flight while chunk k is
// used, the five-channel window in registers (ChannelWindow, lrn_value: the bits of pvhip_lrn_f32) -- with the sink of maxpool3x3_lrn_conv1x1_kernel:
// the normalised value of channel c is the lane's column of the k = 1 outer product with W[.][c], channel after channel in ascending order (the
// bits of the pointwise convolution).  No planes in LDS and no barrier in the loop; LDS holds the transposed weights only, at a pitch of
// 32 KT + 1 floats so that the transposing writes of a wave (consecutive c) fall into different banks.
struct LrnConvArgs {
    const float* x;           // (n, c, hw)
    const float* cw;          // (k_out, c, 1, 1)
    const float* cbias;       // k_out, or null
    float*       y;           // (n, k_out, hw)
    int   n, c, hw, k_out, act;
    float alpha, beta, bias, act_lo, act_hi;
};

template <int BETA_MODE, int KT>
__global__ __launch_bounds__(kBlock, 4) void lrn_conv1x1_kernel(LrnConvArgs a, FastDiv d_hw, FastDiv d_c) {
    constexpr int SIZE = 5, HALF = SIZE / 2, T = kLrnT, WP = 32 * KT + 1;
    extern __shared__ __attribute__((aligned(16))) float wl[];      // [c][WP]: wl[c][k] = W[k][c], zeros past k_out
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const unsigned total = (unsigned)a.n * (unsigned)a.hw;
    const unsigned t = blockIdx.x * kBlock + tid;
    const bool     live = t < total;
    const unsigned tc = live ? t : total - 1;                       // a dead lane walks along on the last pixel (every lane of the wave takes part in the MFMAs)
    const unsigned img = fdiv(tc, d_hw), px = tc - img * (unsigned)a.hw;
    const float* __restrict__ xv = a.x + (size_t)img * a.c * a.hw + px;
    const size_t cstride = (size_t)a.hw;
    const int    n_chunks = a.c / T;
    float cur[T], nxt[T];
#pragma unroll
    for (int j = 0; j < T; ++j) cur[j] = ldnt(xv + (size_t)j * cstride);          // the first chunk is on its way while the weights are staged
    // the transposed weights (e = k * c + ci: the global reads of a wave are consecutive), all loads of a lane in flight together
    {
        constexpr int NW = 64 * 32 * KT / kBlock;
        float wv[NW];
        const int we = a.k_out * a.c;
#pragma unroll
        for (int j = 0; j < NW; ++j) wv[j] = tid + j * kBlock < we ? a.cw[tid + j * kBlock] : 0.0f;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int e = tid + j * kBlock;
            const int k = (int)fdiv((unsigned)e, d_c), ci = e - k * a.c;
            if (e < a.c * 32 * KT) wl[ci * WP + k] = wv[j];
        }
    }
    __syncthreads();

    const float* const wl_lane = wl + (lane & 31);
    floatx32 acc[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int r = 0; r < 32; ++r) acc[kt][r] = 0.0f;
    ChannelWindow<SIZE> win;
    win.clear();
    // channel ch enters the window, which is then centred on channel ch - HALF: its normalised value meets the weights of that channel
    auto push = [&](float v, int ch) {
        win.push(v);
        if (ch >= HALF) {
            const float o = live ? lrn_value<SIZE, BETA_MODE>(win.v, win.v[HALF], a.alpha, a.beta, a.bias) : 0.0f;
            const float* const wc = wl_lane + (ch - HALF) * WP;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) acc[kt] = __builtin_amdgcn_mfma_f32_32x32x1f32(wc[32 * kt], o, acc[kt], 0, 0, 0);
        }
    };
    for (int k = 0; k < n_chunks; ++k) {
        if (k + 1 < n_chunks) {
            const float* __restrict__ xn = xv + (size_t)(k + 1) * T * cstride;
#pragma unroll
            for (int j = 0; j < T; ++j) nxt[j] = ldnt(xn + (size_t)j * cstride);
        }
#pragma unroll
        for (int j = 0; j < T; ++j) push(cur[j], k * T + j);
#pragma unroll
        for (int j = 0; j < T; ++j) cur[j] = nxt[j];
    }
#pragma unroll
    for (int j = 0; j < HALF; ++j) push(0.0f, a.c + j);             // the trailing channels: their windows run past the tensor (zeros)

    // ---- epilogue (maxpool3x3_lrn_conv1x1_kernel's): acc[kt][16 b + v] at lane (j = lane & 31, h = lane >> 5) = output channel 32 kt + 8 (v / 4) + 4 h + v % 4
    // of the pixel of lane 32 b + j
    const int h2 = lane >> 5;
    const ActBounds ab = act_bounds(a.act, a.act_lo, a.act_hi);
#pragma unroll
    for (int bl = 0; bl < 2; ++bl) {
        const unsigned tb = blockIdx.x * kBlock + (tid & ~(kWave - 1)) + 32 * bl + (lane & 31);      // the pixel of lane 32 b + j of this wave
        const bool     ok = tb < total;
        const unsigned ib = fdiv(ok ? tb : 0u, d_hw), pb = (ok ? tb : 0u) - ib * (unsigned)a.hw;
        float* const   yimg = a.y + (size_t)ib * a.k_out * a.hw + pb;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            float bv[16], vv[16];
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int kk = 32 * kt + 8 * (v >> 2) + 4 * h2 + (v & 3);
                bv[v] = (a.cbias != nullptr && kk < a.k_out) ? a.cbias[kk] : 0.0f;
                vv[v] = acc[kt][16 * bl + v];
            }
            bias_act_n<16>(vv, bv, a.cbias != nullptr, a.act, ab);
            if (ok) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int kk = 32 * kt + 8 * (v >> 2) + 4 * h2 + (v & 3);
                    if (kk < a.k_out) yimg[(size_t)kk * a.hw] = vv[v];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// LRN + MaxPool 3x3 / stride 2 / no padding, WITHOUT A BARRIER (round 4; GoogLeNet's conv2/norm2 -> pool2/3x3_s2).  The workgroup form
// above spends a third of its time in its pooling phase and 0.076 of its 0.184 ms in the loop and its two barriers per eight channels
// (scripts/time_lrnpool_abl.py); its loads alone take 0.112 ms.  Here a WAVE is the unit: it owns four pooled rows of one image and a
// group of channels, i.e. nine input rows of W pixels as W / 8 lanes per row with eight adjacent pixels each (W = 56: 63 lanes), walks
// the channel axis in steps of four (the five-channel window in registers, squares summed in ascending channel order: the arithmetic of
// lrn_window_kernel -- the same bits), leaves four normalised planes in ITS OWN 8 KB of LDS, and pools them itself: a lane owns two
// adjacent outputs of a row, whose windows are five columns of three rows = three 16-byte and three 4-byte LDS reads instead of
// eighteen.  LDS executes a wave's instructions in order: no barrier, no counter, the other waves of the workgroup are strangers.
// The channel groups overlap by the window's reach (two channels each side: 52 loads per 48 channels).
// MEASURED, NOT THE DEFAULT (PVHIP_LRNPOOL_WAVE=1): 0.180 ms against 0.171 for the workgroup form on the same box, the same bits (scripts/
// time_lrnpool.py) -- 140 registers (three waves per SIMD) and ~20 issue slots of LRN arithmetic per element: the barriers were not it.
struct LrnPoolWaveArgs {
    const float* x;
    float*       y;
    int   n, c, h, w, oh, ow;
    int   R, n_bands, rows_in;     // pooled rows per wave, bands per image, input rows of a band (2 R + 1)
    int   cg, n_groups;            // channels per wave (a multiple of four), groups per image
    int   lpr, op;                 // lanes per input row (w / 8); output pairs per pooled row (ceil(ow / 2))
    long  n_items;
    float alpha, beta, bias;
};

template <int BETA_MODE>
__global__ __launch_bounds__(kBlock) void lrn_maxpool3x3_wave_kernel(LrnPoolWaveArgs a) {
    constexpr int T = 4;
    typedef float vec4 __attribute__((ext_vector_type(4)));
    struct V8 { vec4 lo, hi; };
    extern __shared__ __attribute__((aligned(16))) float wave_planes[];              // [4 waves][T][rows_in][w]
    const int lane = threadIdx.x & (kWave - 1);
    const int wid  = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const long item = (long)blockIdx.x * (kBlock / kWave) + wid;
    if (item >= a.n_items) return;
    // item -> (image, band, channel group): the groups of a band back to back (they share the input rows' neighbourhood in L2)
    const int g    = (int)(item % a.n_groups);
    const long ib  = item / a.n_groups;
    const int band = (int)(ib % a.n_bands), img = (int)(ib / a.n_bands);
    const int oy0  = band * a.R;
    const int iy0  = 2 * oy0;
    const int c0   = g * a.cg;
    const int hw = a.h * a.w, ohw = a.oh * a.ow;
    const int plane_l = a.rows_in * a.w;
    float* const lds = wave_planes + (size_t)wid * T * plane_l;

    // ---- load side: lane -> (input row of the band, eight columns)
    const int  lrow = lane / a.lpr, lcol = (lane - lrow * a.lpr) * 8;
    const bool lact = lrow < a.rows_in && iy0 + lrow < a.h;               // a row past the image: zeros (never pooled: the windows are clipped)
    const float* const xl = a.x + (size_t)img * a.c * hw + (size_t)(lact ? (iy0 + lrow) * a.w + lcol : 0);
    float* const lmine = lds + lrow * a.w + lcol;
    const bool lwrite = lrow < a.rows_in;

    // ---- pool side: lane -> (pooled row of the band, two adjacent outputs)
    const int  prow = lane / a.op, pj = lane - prow * a.op;
    const int  oy = oy0 + prow, ox = 2 * pj;
    const bool pact = prow < a.R && oy < a.oh && ox < a.ow;
    const bool second = ox + 1 < a.ow;
    // window rows 2 prow + k (clipped at the image: a row past it repeats the first), columns 4 pj .. 4 pj + 4 (the fifth may be past the row)
    unsigned roff[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int r = 2 * prow + k;
        roff[k] = (unsigned)(((pact && iy0 + r < a.h) ? r : 2 * (pact ? prow : 0)) * a.w + 4 * (pact ? pj : 0));
    }
    const bool col4 = 4 * pj + 4 < a.w;                                   // the fifth column exists
    float* const yout = a.y + ((size_t)img * a.c) * ohw + (size_t)(pact ? oy * a.ow + ox : 0);

    auto load8 = [&](int ch) -> V8 {
        V8 v;
        if (lact && ch >= 0 && ch < a.c) {
            const vec4* p = reinterpret_cast<const vec4*>(xl + (size_t)ch * hw);
            v.lo = ldnt(p); v.hi = ldnt(p + 1);
        } else {
            v.lo = (vec4)(0.0f); v.hi = (vec4)(0.0f);
        }
        return v;
    };
    V8 win[5], nxt[T];
#pragma unroll
    for (int q = 0; q < 5; ++q) { win[q].lo = (vec4)(0.0f); win[q].hi = (vec4)(0.0f); }
    const int n_chunks = a.cg / T + 1;                                    // incoming chunks of four channels: c0 - 2 + 4 i ..; chunk i >= 1 completes channels c0 + 4 (i - 1) ..
#pragma unroll
    for (int j = 0; j < T; ++j) nxt[j] = load8(c0 - 2 + j);
    for (int i = 0; i < n_chunks; ++i) {
        V8 cur[T];
#pragma unroll
        for (int j = 0; j < T; ++j) cur[j] = nxt[j];
        if (i + 1 < n_chunks) {
#pragma unroll
            for (int j = 0; j < T; ++j) nxt[j] = load8(c0 - 2 + T * (i + 1) + j);
        }
#pragma unroll
        for (int j = 0; j < T; ++j) {
            // channel c0 - 2 + 4 i + j enters the window; the window is then centred on the channel two below it
#pragma unroll
            for (int q = 0; q < 4; ++q) win[q] = win[q + 1];
            win[4] = cur[j];
            if (i >= 1) {
                vec4 slo = win[0].lo * win[0].lo, shi = win[0].hi * win[0].hi;
#pragma unroll
                for (int q = 1; q < 5; ++q) { slo = slo + win[q].lo * win[q].lo; shi = shi + win[q].hi * win[q].hi; }
                vec4 olo, ohi;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    olo[v] = lrn_div(win[2].lo[v], a.bias + a.alpha * slo[v], a.beta, BETA_MODE);
                    ohi[v] = lrn_div(win[2].hi[v], a.bias + a.alpha * shi[v], a.beta, BETA_MODE);
                }
                if (lwrite) {
                    *reinterpret_cast<vec4*>(lmine + j * plane_l) = olo;
                    *reinterpret_cast<vec4*>(lmine + j * plane_l + 4) = ohi;
                }
            }
        }
        if (i == 0) continue;
        __builtin_amdgcn_wave_barrier();                                  // (a scheduling fence: LDS runs this wave's writes before its reads)
        const int ch0 = c0 + T * (i - 1);
        if (pact) {
#pragma unroll
            for (int p = 0; p < T; ++p) {
                const float* const pl = lds + p * plane_l;
                float m0[3], m1[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const vec4  v  = *reinterpret_cast<const vec4*>(pl + roff[k]);
                    const float v4 = col4 ? pl[roff[k] + 4] : v[3];
                    m0[k] = max3_nan(v[0], v[1], v[2]);
                    m1[k] = max3_nan(v[2], v[3], v4);
                }
                const float r0 = max3_nan(m0[0], m0[1], m0[2]), r1 = max3_nan(m1[0], m1[1], m1[2]);
                float* const yo = yout + (size_t)(ch0 + p) * ohw;
                if (second && (a.ow & 1) == 0) *reinterpret_cast<float2*>(yo) = make_float2(r0, r1);
                else { yo[0] = r0; if (second) yo[1] = r1; }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Geometry of the wave form, or false when the pair is outside it (then the workgroup form above is asked).
bool plan_lrn_pool_wave(int n, int c, int h, int w, int size, float beta, float bias, int oh, int ow, int kh, int kw, int sh, int sw, int pt, int pl,
                        int pb, int pr, LrnPoolWaveArgs& a, int& bm) {
    if (n <= 0 || c < 8 || c % 4 != 0 || h < 3 || w < 8 || w % 8 != 0 || oh <= 0 || ow <= 0) return false;
    if (size != 5 || kh != 3 || kw != 3 || sh != 2 || sw != 2 || pt != 0 || pl != 0 || pb != 0 || pr != 0) return false;
    if (2 * (oh - 1) > h - 1 || 2 * (ow - 1) > w - 1 || 2 * (ow - 1) + 2 > w) return false;      // the first cell of every window is in the image; at most the third column / row is clipped
    if ((unsigned long long)n * c * h * w >= (1ull << 31)) return false;
    bm = lrn_beta_mode(beta, bias);
    if (bm != 4 && bm != 1) return false;
    const int lpr = w / 8;
    const int R = (kWave / lpr - 1) / 2;                  // rows_in = 2 R + 1 input rows in 64 lanes
    const int op = (ow + 1) / 2;
    if (R < 1 || R * op > kWave) return false;
    int cg = 0;
    for (int cand = 64; cand >= 16; cand -= 4)            // the largest group of at most 64 channels that divides C (48 for C = 192)
        if (c % cand == 0) { cg = cand; break; }
    if (cg == 0) return false;
    a.n = n; a.c = c; a.h = h; a.w = w; a.oh = oh; a.ow = ow;
    a.R = R; a.n_bands = (oh + R - 1) / R; a.rows_in = 2 * R + 1;
    a.cg = cg; a.n_groups = c / cg; a.lpr = lpr; a.op = op;
    a.n_items = (long)n * a.n_bands * a.n_groups;
    return (size_t)4 * 4 * a.rows_in * w * sizeof(float) <= 64 * 1024;
}

// What a fused LRN / MaxPool launch will be, decided HERE and nowhere else: the _supported queries report `ok`, the entries launch
// what the plan says.  The geometry is the pooling's, whichever node comes first.
struct LrnPoolPlan {
    bool        ok = false;      // the pair is inside what the workgroup kernels cover
    LrnPoolArgs a{};             // geometry (x, y, alpha, beta, bias are the entry's to fill); a.pool4: which body of lrn_maxpool3x3_kernel runs
    int         vec = 0;         // pixels per lane: 4 where a row is a whole number of 16-byte pieces
    int         bm  = 0;         // beta mode: 4 or 1
    int         st  = 0;         // pooling stride: 1 or 2
    int         ni  = 0;         // pooled outputs of a band and plane per lane: instantiations for 1, 2 and 4
    size_t      lds = 0;
};

LrnPoolPlan plan_lrn_pool(int n, int c, int h, int w, int size, float beta, float bias, int oh, int ow, int kh, int kw, int sh, int sw,
                          int pt, int pl, int pb, int pr) {
    LrnPoolPlan p;
    LrnPoolArgs& a = p.a;
    if (n <= 0 || c < 8 || c % 8 != 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0) return p;
    if (size != 5 || kh != 3 || kw != 3 || sh != sw || (sh != 1 && sh != 2)) return p;
    if (pt < 0 || pl < 0 || pb < 0 || pr < 0 || pt > 2 || pl > 2) return p;
    if ((oh - 1) * sh > pt + h - 1 || (ow - 1) * sw > pl + w - 1) return p;       // clamped taps stay inside their window
    if ((unsigned long long)n * c * h * w >= (1ull << 31)) return p;
    p.bm = lrn_beta_mode(beta, bias);
    if (p.bm != 4 && p.bm != 1) return p;
    p.st  = sh;
    p.vec = (w % 4 == 0) ? 4 : 1;
    int rows = (kBlock * p.vec / w - 3) / sh + 1;                 // largest band whose input rows fit the 256 lanes
    if (kBlock * p.vec / w < 3 && h >= 3) return p;
    if (rows < 1) return p;
    if (rows > oh) rows = oh;
    int bands = (oh + rows - 1) / rows;
    rows  = (oh + bands - 1) / bands;
    bands = (oh + rows - 1) / rows;
    int in_rows = (rows - 1) * sh + 3;
    if (in_rows > h) in_rows = h;
    if (in_rows * w > kBlock * p.vec) return p;
    a.n = n; a.c = c; a.h = h; a.w = w; a.oh = oh; a.ow = ow; a.pt = pt; a.pl = pl; a.hp = h + pt + pb; a.wp = w + pl + pr;
    a.band_rows = rows; a.n_bands = bands;
    // the kernels are instantiated for up to four pooled outputs per lane and plane (1 at stride 2: a band holds <= 1024 input pixels; up
    // to 4 at stride 1); a pooled row wider than the input row (ow > w) with a tall band needs more: the QUERY must say no there, so that
    // the caller falls back to two launches instead of failing at run time
    p.ni = (rows * ow + kBlock - 1) / kBlock;
    if (p.ni > 4) return p;
    // four pooled outputs per lane (pool4 in lrn_maxpool3x3_kernel); 2 ow <= w: the eight columns a quad reads whole lie in the row, only
    // the ninth is clamped.  PVHIP_TUNE6=1 keeps one per lane (A/B runs)
    a.pool4 = (p.vec == 4 && sh == 2 && pt == 0 && pl == 0 && ow % 4 == 0 && 2 * ow <= w && (ow / 4) * rows <= kWave && settings().tune[6] != 1) ? 1 : 0;
    a.plane_l = (in_rows * w + 3) & ~3;
    p.lds     = (size_t)kLrnT * a.plane_l * sizeof(float);
    p.ok      = p.lds <= 64 * 1024 && (long long)n * bands < (1ll << 31);
    return p;
}

// MaxPool then LRN then a 1x1 / stride 1 / unpadded convolution: the plan above with one pooled output per lane (bands of at most 256
// outputs), rows of a multiple of four pixels, and at most 64 input and 64 output channels (the transposed weights stay in LDS).
LrnPoolPlan plan_pool_lrn_conv(int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh, int sw, int pt, int pl, int pb, int pr, int size,
                               float beta, float bias, int k_out) {
    LrnPoolPlan p = plan_lrn_pool(n, c, h, w, size, beta, bias, oh, ow, kh, kw, sh, sw, pt, pl, pb, pr);
    if (!p.ok) return p;
    p.ok = false;
    if (p.vec != 4 || p.a.band_rows * ow > kBlock || k_out <= 0 || k_out > 64 || c > 64) return p;
    if ((unsigned long long)n * k_out * oh * ow >= (1ull << 31)) return p;
    p.lds += (size_t)c * 32 * ((k_out + 31) / 32) * sizeof(float);
    p.ok = p.lds <= 64 * 1024;
    return p;
}

// The launch of a two-node kernel K_<5, vec, bm, st, NI> as the plan P_ says; the macro defines one launcher per kernel, right below.
#define PV_LRN_POOL_NI(K_, P_, VEC_, BM_, ST_, NI_) \
    hipLaunchKernelGGL((K_<5, VEC_, BM_, ST_, NI_>), dim3((unsigned)(P_.a.n * P_.a.n_bands)), dim3(kBlock), P_.lds, state().stream, P_.a, \
                       make_fastdiv((unsigned)P_.a.n_bands), make_fastdiv((unsigned)P_.a.ow))
#define PV_LRN_POOL_ST(K_, P_, VEC_, BM_, ST_)                          \
    {                                                                   \
        if (P_.ni <= 1) PV_LRN_POOL_NI(K_, P_, VEC_, BM_, ST_, 1);      \
        else if (P_.ni <= 2) PV_LRN_POOL_NI(K_, P_, VEC_, BM_, ST_, 2); \
        else PV_LRN_POOL_NI(K_, P_, VEC_, BM_, ST_, 4);                 \
    }
#define PV_LRN_POOL_BM(K_, P_, VEC_, BM_) \
    { if (P_.st == 1) PV_LRN_POOL_ST(K_, P_, VEC_, BM_, 1) else PV_LRN_POOL_ST(K_, P_, VEC_, BM_, 2) }
#define PV_LRN_POOL_LAUNCHER(NAME_, K_)                                                                   \
    void NAME_(const LrnPoolPlan& plan) {                                                                 \
        if (plan.vec == 4) { if (plan.bm == 4) PV_LRN_POOL_BM(K_, plan, 4, 4) else PV_LRN_POOL_BM(K_, plan, 4, 1) } \
        else               { if (plan.bm == 4) PV_LRN_POOL_BM(K_, plan, 1, 4) else PV_LRN_POOL_BM(K_, plan, 1, 1) } \
    }
PV_LRN_POOL_LAUNCHER(launch_lrn_maxpool, lrn_maxpool3x3_kernel)
PV_LRN_POOL_LAUNCHER(launch_maxpool_lrn, maxpool3x3_lrn_kernel)
#undef PV_LRN_POOL_LAUNCHER
#undef PV_LRN_POOL_BM
#undef PV_LRN_POOL_ST
#undef PV_LRN_POOL_NI

// Fallback for window sizes without a register-window instantiation: every lane re-reads its window.
__global__ __launch_bounds__(kBlock) void lrn_generic_kernel(const float* __restrict__ x, float* __restrict__ y, int n,
                                                              int c, int hw, int size, float alpha, float beta,
                                                              float bias, int beta_mode) {
    const size_t total  = (size_t)n * c * hw;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int    half   = size / 2;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const size_t p   = e % hw;
        const size_t q   = e / hw;
        const int    ch  = (int)(q % c);
        const size_t img = q / c;
        int lo = ch - half, hi = ch + half + 1;
        if (lo < 0) lo = 0;
        if (hi > c) hi = c;
        float s = 0.0f;
        for (int k = lo; k < hi; ++k) {
            const float v = x[(img * c + k) * hw + p];
            s             = (k == lo) ? v * v : s + v * v;
        }
        const float d = bias + alpha * s;
        y[e]          = lrn_div(x[e], d, beta, beta_mode);
    }
}

// Which kernel an LRN launch takes, decided HERE and nowhere else: pvhip_lrn_f32 switches on the plan, pvhip_lrn_form (no device
// needed) reports it.  The register-window kernel is instantiated for windows of 3, 5 and 7 channels and wants whole chunks of
// eight channels; VEC = 4 pixels per lane where a plane is a whole number of 16-byte pieces.
struct LrnPlan {
    int kind, size, vec, bm, grid, loops;
};

LrnPlan plan_lrn(int n, int c, int hw, int size, float beta, float bias) {
    LrnPlan p;
    p.bm = lrn_beta_mode(beta, bias);
    if (c % 8 == 0 && c >= 8 && (size == 3 || size == 5 || size == 7)) {
        p.kind = PVHIP_LRN_WINDOW;
        p.size = size;
        p.vec  = (hw % 4 == 0) ? 4 : 1;
        p.grid = grid_for((size_t)n * (hw / p.vec));
        p.loops = (size_t)n * (hw / p.vec) > (size_t)p.grid * kBlock;
    } else {
        p.kind = PVHIP_LRN_GENERIC;
        p.size = size;
        p.vec  = 1;
        p.grid = grid_for((size_t)n * c * hw);
        p.loops = (size_t)n * c * hw > (size_t)p.grid * kBlock;
    }
    return p;
}

// SoftMax: a workgroup per row, at most kMaxBlocks of them (rows beyond that in the kernel's loop).
int plan_softmax_grid(int rows) { return rows < kMaxBlocks ? rows : kMaxBlocks; }

template <int SIZE, int BETA_MODE>
void launch_lrn_window_b(const LrnPlan& p, const float* x, float* y, int n, int c, int hw, float alpha, float beta, float bias) {
    if (p.vec == 4)
        hipLaunchKernelGGL((lrn_window_kernel<SIZE, 4, BETA_MODE>), dim3(p.grid), dim3(kBlock), 0, state().stream, x, y,
                           n, c, hw, alpha, beta, bias);
    else
        hipLaunchKernelGGL((lrn_window_kernel<SIZE, 1, BETA_MODE>), dim3(p.grid), dim3(kBlock), 0, state().stream, x, y,
                           n, c, hw, alpha, beta, bias);
}

template <int SIZE>
void launch_lrn_window(const LrnPlan& p, const float* x, float* y, int n, int c, int hw, float alpha, float beta, float bias) {
    switch (p.bm) {
        case 1: launch_lrn_window_b<SIZE, 1>(p, x, y, n, c, hw, alpha, beta, bias); break;
        case 2: launch_lrn_window_b<SIZE, 2>(p, x, y, n, c, hw, alpha, beta, bias); break;
        case 3: launch_lrn_window_b<SIZE, 3>(p, x, y, n, c, hw, alpha, beta, bias); break;
        case 4: launch_lrn_window_b<SIZE, 4>(p, x, y, n, c, hw, alpha, beta, bias); break;
        default: launch_lrn_window_b<SIZE, 0>(p, x, y, n, c, hw, alpha, beta, bias); break;
    }
}

}  // namespace

extern "C" {

int pvhip_softmax_rows_f32(const float* x, float* y, int rows, int cols) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(rows >= 0 && cols >= 0);
    if (rows == 0 || cols == 0) return PVHIP_OK;
    PVHIP_CHECK_ARG(x != nullptr && y != nullptr);
    const int g = plan_softmax_grid(rows);
    hipLaunchKernelGGL(softmax_rows_kernel, dim3(g), dim3(kBlock), 0, state().stream, x, y, rows, cols);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

int pvhip_softmax_rows_form(int rows, int cols, int* form) {
    PVHIP_CHECK_ARG(form != nullptr);
    for (int i = 0; i < PVHIP_FORM_INTS; ++i) form[i] = 0;
    form[PVHIP_FORM_KIND] = PVHIP_FORM_NONE;
    PVHIP_CHECK_ARG(rows >= 0 && cols >= 0);
    if (rows == 0 || cols == 0) return PVHIP_OK;                     // nothing is launched
    form[PVHIP_FORM_KIND]  = PVHIP_SOFTMAX_ROWS;
    form[PVHIP_FORM_GRID]  = plan_softmax_grid(rows);
    form[PVHIP_FORM_LOOPS] = rows > form[PVHIP_FORM_GRID] ? 1 : 0;
    return PVHIP_OK;
}

int pvhip_lrn_f32(const float* x, float* y, int n, int c, int hw, int size, float alpha, float beta, float bias) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(n >= 0 && c >= 0 && hw >= 0 && size >= 1);
    if ((size_t)n * c * hw == 0) return PVHIP_OK;
    PVHIP_CHECK_ARG(x != nullptr && y != nullptr);
    if ((unsigned long long)n * c * hw >= (1ull << 31))
        return fail(PVHIP_EUNSUPPORTED, "pvhip_lrn_f32: tensor exceeds 2^31 elements");
    const LrnPlan p = plan_lrn(n, c, hw, size, beta, bias);
    switch (p.kind == PVHIP_LRN_WINDOW ? p.size : 0) {
        case 3: launch_lrn_window<3>(p, x, y, n, c, hw, alpha, beta, bias); break;
        case 5: launch_lrn_window<5>(p, x, y, n, c, hw, alpha, beta, bias); break;
        case 7: launch_lrn_window<7>(p, x, y, n, c, hw, alpha, beta, bias); break;
        default:
            hipLaunchKernelGGL(lrn_generic_kernel, dim3(p.grid), dim3(kBlock), 0, state().stream, x, y,
                               n, c, hw, size, alpha, beta, bias, p.bm);
    }
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

int pvhip_lrn_form(int n, int c, int hw, int size, float beta, float bias, int* form) {
    PVHIP_CHECK_ARG(form != nullptr);
    for (int i = 0; i < PVHIP_FORM_INTS; ++i) form[i] = 0;
    form[PVHIP_FORM_KIND] = PVHIP_FORM_NONE;
    PVHIP_CHECK_ARG(n >= 0 && c >= 0 && hw >= 0 && size >= 1);
    if ((size_t)n * c * hw == 0) return PVHIP_OK;                    // nothing is launched
    if ((unsigned long long)n * c * hw >= (1ull << 31))
        return fail(PVHIP_EUNSUPPORTED, "pvhip_lrn_form: tensor exceeds 2^31 elements");
    const LrnPlan p = plan_lrn(n, c, hw, size, beta, bias);
    form[PVHIP_FORM_KIND] = p.kind;
    form[PVHIP_FORM_LRN_SIZE] = p.size;
    form[PVHIP_FORM_GRID] = p.grid;
    form[PVHIP_FORM_LOOPS] = p.loops;
    form[PVHIP_FORM_VEC] = p.vec;
    form[PVHIP_FORM_LRN_BETA_MODE] = p.bm;
    return PVHIP_OK;
}

int pvhip_lrn_maxpool_supported(int n, int c, int h, int w, int size, float beta, float bias, int oh, int ow, int kh, int kw,
                                int sh, int sw, int pad_top, int pad_left, int pad_bottom, int pad_right) {
    return plan_lrn_pool(n, c, h, w, size, beta, bias, oh, ow, kh, kw, sh, sw, pad_top, pad_left, pad_bottom, pad_right).ok ? 1 : 0;
}

int pvhip_lrn_maxpool_f32(const float* x, float* y, int n, int c, int h, int w, int size, float alpha, float beta, float bias,
                          int oh, int ow, int kh, int kw, int sh, int sw, int pad_top, int pad_left, int pad_bottom,
                          int pad_right) {
    PVHIP_REQUIRE_INIT();
    {
        LrnPoolWaveArgs wa{};
        int wbm = 0;
        if (settings().lrnpool_wave && plan_lrn_pool_wave(n, c, h, w, size, beta, bias, oh, ow, kh, kw, sh, sw, pad_top, pad_left, pad_bottom, pad_right, wa, wbm)) {
            PVHIP_CHECK_ARG(x != nullptr && y != nullptr);
            wa.x = x; wa.y = y; wa.alpha = alpha; wa.beta = beta; wa.bias = bias;
            const long blocks = (wa.n_items + kBlock / kWave - 1) / (kBlock / kWave);
            if (blocks <= 0x7fffffffL) {
                const size_t wlds = (size_t)(kBlock / kWave) * 4 * wa.rows_in * w * sizeof(float);
                if (wbm == 4) hipLaunchKernelGGL((lrn_maxpool3x3_wave_kernel<4>), dim3((unsigned)blocks), dim3(kBlock), wlds, state().stream, wa);
                else          hipLaunchKernelGGL((lrn_maxpool3x3_wave_kernel<1>), dim3((unsigned)blocks), dim3(kBlock), wlds, state().stream, wa);
                PVHIP_LAUNCH_CHECK();
                return PVHIP_OK;
            }
        }
    }
    LrnPoolPlan p = plan_lrn_pool(n, c, h, w, size, beta, bias, oh, ow, kh, kw, sh, sw, pad_top, pad_left, pad_bottom, pad_right);
    if (!p.ok)
        return fail(PVHIP_EUNSUPPORTED, "pvhip_lrn_maxpool_f32: shape outside the fused kernel (ask pvhip_lrn_maxpool_supported first)");
    PVHIP_CHECK_ARG(x != nullptr && y != nullptr);
    p.a.x = x; p.a.y = y; p.a.alpha = alpha; p.a.beta = beta; p.a.bias = bias;
#ifdef PVHIP_DIAG
    p.a.abl = settings().conv_ablate;
#endif
    launch_lrn_maxpool(p);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

// MaxPool (3x3) then LRN as one launch: same coverage rules as the other order (the geometry is the pooling's either way).
int pvhip_maxpool_lrn_supported(int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh, int sw, int pad_top, int pad_left,
                                int pad_bottom, int pad_right, int size, float beta, float bias) {
    return plan_lrn_pool(n, c, h, w, size, beta, bias, oh, ow, kh, kw, sh, sw, pad_top, pad_left, pad_bottom, pad_right).ok ? 1 : 0;
}

int pvhip_maxpool_lrn_f32(const float* x, float* y, int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh, int sw,
                          int pad_top, int pad_left, int pad_bottom, int pad_right, int size, float alpha, float beta, float bias) {
    PVHIP_REQUIRE_INIT();
    LrnPoolPlan p = plan_lrn_pool(n, c, h, w, size, beta, bias, oh, ow, kh, kw, sh, sw, pad_top, pad_left, pad_bottom, pad_right);
    if (!p.ok)
        return fail(PVHIP_EUNSUPPORTED, "pvhip_maxpool_lrn_f32: shape outside the fused kernel (ask pvhip_maxpool_lrn_supported first)");
    PVHIP_CHECK_ARG(x != nullptr && y != nullptr);
    p.a.x = x; p.a.y = y; p.a.alpha = alpha; p.a.beta = beta; p.a.bias = bias;
    launch_maxpool_lrn(p);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

// MaxPool (3x3) then LRN then a 1x1 / stride 1 / unpadded convolution (+ bias, activation) as ONE launch (round 5): see plan_pool_lrn_conv.
int pvhip_maxpool_lrn_conv1x1_supported(int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh, int sw, int pad_top, int pad_left,
                                        int pad_bottom, int pad_right, int size, float beta, float bias, int k_out) {
    return plan_pool_lrn_conv(n, c, h, w, oh, ow, kh, kw, sh, sw, pad_top, pad_left, pad_bottom, pad_right, size, beta, bias, k_out).ok ? 1 : 0;
}

int pvhip_maxpool_lrn_conv1x1_f32(const float* x, const float* w_oihw, float* y, int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh, int sw,
                                  int pad_top, int pad_left, int pad_bottom, int pad_right, int size, float alpha, float beta, float bias,
                                  int k_out, const float* conv_bias, int act, float act_lo, float act_hi) {
    PVHIP_REQUIRE_INIT();
    const LrnPoolPlan p = plan_pool_lrn_conv(n, c, h, w, oh, ow, kh, kw, sh, sw, pad_top, pad_left, pad_bottom, pad_right, size, beta, bias, k_out);
    if (!p.ok)
        return fail(PVHIP_EUNSUPPORTED, "pvhip_maxpool_lrn_conv1x1_f32: shape outside the fused kernel (ask pvhip_maxpool_lrn_conv1x1_supported first)");
    PVHIP_CHECK_ARG(x != nullptr && w_oihw != nullptr && y != nullptr && act >= 0 && act <= 2);
    PoolLrnConvArgs ca{};
    ca.p = p.a;
    ca.p.pool4 = 0;           // (lrn_maxpool3x3_kernel's)
    ca.p.x = x; ca.p.y = nullptr; ca.p.alpha = alpha; ca.p.beta = beta; ca.p.bias = bias;
    ca.cw = w_oihw; ca.cbias = conv_bias; ca.y = y; ca.k_out = k_out; ca.act = act; ca.act_lo = act_lo; ca.act_hi = act_hi;
    const dim3 grid((unsigned)(n * ca.p.n_bands));
    const FastDiv d_bands = make_fastdiv((unsigned)ca.p.n_bands), d_ow = make_fastdiv((unsigned)ow);
    const int kt = (k_out + 31) / 32;
#define PV_PLC(BM_, ST_, KT_) hipLaunchKernelGGL((maxpool3x3_lrn_conv1x1_kernel<BM_, ST_, KT_>), grid, dim3(kBlock), p.lds, state().stream, ca, d_bands, d_ow)
    if (p.bm == 4) {
        if (p.st == 1) { if (kt == 1) PV_PLC(4, 1, 1); else PV_PLC(4, 1, 2); }
        else           { if (kt == 1) PV_PLC(4, 2, 1); else PV_PLC(4, 2, 2); }
    } else {
        if (p.st == 1) { if (kt == 1) PV_PLC(1, 1, 1); else PV_PLC(1, 1, 2); }
        else           { if (kt == 1) PV_PLC(1, 2, 1); else PV_PLC(1, 2, 2); }
    }
#undef PV_PLC
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

// LRN (five channels, beta = 0.75; LRN.py:10-22) then a 1x1 / stride 1 / unpadded convolution (+ bias, activation; Convolution.py:57-87) as ONE launch
// on a tensor (n, c, hw) that is pooled already: whole chunks of eight and at most 64 channels in, at most 64 out.  The bits of pvhip_lrn_f32 followed
// by the pointwise convolution -- and so of pvhip_maxpool_lrn_conv1x1_f32 on the unpooled tensor.
int pvhip_lrn_conv1x1_supported(int n, int c, int hw, int size, float beta, float bias, int k_out) {
    if (n <= 0 || c < 8 || c % 8 != 0 || c > 64 || hw <= 0 || size != 5 || k_out <= 0 || k_out > 64) return 0;
    const int bm = lrn_beta_mode(beta, bias);
    if (bm != 4 && bm != 1) return 0;
    if ((unsigned long long)n * c * hw >= (1ull << 31) || (unsigned long long)n * k_out * hw >= (1ull << 31)) return 0;
    return 1;
}

int pvhip_lrn_conv1x1_f32(const float* x, const float* w_oihw, float* y, int n, int c, int hw, int size, float alpha, float beta, float bias, int k_out,
                          const float* conv_bias, int act, float act_lo, float act_hi) {
    PVHIP_REQUIRE_INIT();
    if (!pvhip_lrn_conv1x1_supported(n, c, hw, size, beta, bias, k_out))
        return fail(PVHIP_EUNSUPPORTED, "pvhip_lrn_conv1x1_f32: shape outside the fused kernel (ask pvhip_lrn_conv1x1_supported first)");
    PVHIP_CHECK_ARG(x != nullptr && w_oihw != nullptr && y != nullptr && act >= 0 && act <= 2);
    LrnConvArgs a{};
    a.x = x; a.cw = w_oihw; a.cbias = conv_bias; a.y = y;
    a.n = n; a.c = c; a.hw = hw; a.k_out = k_out; a.act = act;
    a.alpha = alpha; a.beta = beta; a.bias = bias; a.act_lo = act_lo; a.act_hi = act_hi;
    const int    kt = (k_out + 31) / 32;
    const dim3   grid((unsigned)(((unsigned long long)n * hw + kBlock - 1) / kBlock));
    const size_t lds = (size_t)c * (32 * kt + 1) * sizeof(float);
    const FastDiv d_hw = make_fastdiv((unsigned)hw), d_c = make_fastdiv((unsigned)c);
#define PV_LC(BM_, KT_) hipLaunchKernelGGL((lrn_conv1x1_kernel<BM_, KT_>), grid, dim3(kBlock), lds, state().stream, a, d_hw, d_c)
    if (lrn_beta_mode(beta, bias) == 4) { if (kt == 1) PV_LC(4, 1); else PV_LC(4, 2); }
    else                                { if (kt == 1) PV_LC(1, 1); else PV_LC(1, 2); }
#undef PV_LC
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
