// FP16 IRs: what stands between the convolutions of a network on fp16 tensors blocked by eight channels (the c8 tensor of
// pvhip_f16_c8.h) -- no convolution kernels, they are here because they read and write that layout, one 16-byte piece per pixel and
// channel block:
//   * MaxPool 3x3 of any stride and padding (pvhip_maxpool3x3_c8; a NaN wins, v_pk_maximum3_f16 through pk_max3_nan);
//   * GoogLeNet's stem behind conv1: MaxPool 3x3 + LRN (pvhip_maxpool3x3_lrn_c8), LRN + MaxPool 3x3 (pvhip_lrn_maxpool3x3_c8), and
//     MaxPool 3x3 + LRN + the 1x1 convolution behind them on the matrix cores (pvhip_maxpool3x3_lrn_conv1x1_c8), one launch each;
//   * AvgPool in front of the classifier (pvhip_avgpool_c8), fp32 NCHW out.
// The module-form convolution that reads and writes the same tensors is pvhip_f16c8m.hip.
#include "pvhip_f16_c8.h"

using namespace pvhip;

namespace {

// MaxPool 3x3 (any stride / padding, MaxPool.py:41-72) on fp16 c8 tensors: one lane = one (image, channel block, output pixel), nine
// 16-byte loads (cells of the zero padding: zeros; cells past the padded edge: not in the window), NaN wins, one 16-byte store.
__global__ __launch_bounds__(kBlock) void maxpool3x3_c8_kernel(const _Float16* __restrict__ x, _Float16* __restrict__ y, int n, int cb, int h, int w,
                                                               int oh, int ow, int sh, int sw, int pt, int pl, int hp, int wp) {
    const size_t total = (size_t)n * cb * oh * ow;
    const half8 zero = half8{0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int    ox = (int)(e % ow);
        size_t       f  = e / ow;
        const int    oy = (int)(f % oh);
        const size_t plane = f / oh;                                  // image * cb + block
        const half8* const xp = reinterpret_cast<const half8*>(x) + plane * (size_t)(h * w);
        half8 rowm[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int py = oy * sh + r;                               // row in the padded image
            half8 v[3];
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int px = ox * sw + s;
                const int iy = py - pt, ix = px - pl;
                const bool inwin = py < hp && px < wp;                // the window is clipped at the padded edge (MaxPool.py:63-66)
                const bool inimg = iy >= 0 && iy < h && ix >= 0 && ix < w;
                // a cell outside the window repeats the window's first cell (always inside: oy * sh < hp), a padding cell is zero
                const int cy = inwin ? iy : oy * sh - pt, cx = inwin ? ix : ox * sw - pl;
                const bool cimg = inwin ? inimg : (cy >= 0 && cy < h && cx >= 0 && cx < w);
                v[s] = cimg ? xp[(size_t)cy * w + cx] : zero;
            }
            rowm[r] = pk_max3_nan(v[0], v[1], v[2]);
        }
        reinterpret_cast<half8*>(y)[e] = pk_max3_nan(rowm[0], rowm[1], rowm[2]);
    }
}

// MaxPool 3x3 followed by LRN over five channels (MaxPool.py:41-72 then LRN.py:10-22; GoogLeNet's pool1/3x3_s2 -> pool1/norm1) on fp16 c8
// tensors, one launch: a lane owns one output pixel and walks the channel blocks -- nine 16-byte loads and the NaN-propagating maxima per
// block (the pooled tensor never exists), the pooled values of three consecutive blocks in registers as fp32, because the window of
// channel 8 b + q reaches two channels into the neighbour blocks; squares summed in ascending channel order, d^-beta as in lrn_div.
template <int BETA_MODE>
__global__ __launch_bounds__(kBlock) void maxpool3x3_lrn_c8_kernel(const _Float16* __restrict__ x, _Float16* __restrict__ y, int n, int cb, int c, int h, int w,
                                                                   int oh, int ow, int sh, int sw, int pt, int pl, int hp, int wp, float alpha,
                                                                   float beta, float bias) {
    const size_t total = (size_t)n * oh * ow;
    const half8 zero = half8{0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int ox = (int)(e % ow);
        const size_t f = e / ow;
        const int oy = (int)(f % oh), im = (int)(f / oh);
        // the nine cells of the window: offsets inside a plane, or -1 for a zero cell of the padding; a cell past the padded edge repeats the first
        int off[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int s2 = 0; s2 < 3; ++s2) {
                const int py = oy * sh + r, px = ox * sw + s2;
                const bool inwin = py < hp && px < wp;
                const int cy = (inwin ? py : oy * sh) - pt, cx = (inwin ? px : ox * sw) - pl;
                off[3 * r + s2] = (cy >= 0 && cy < h && cx >= 0 && cx < w) ? cy * w + cx : -1;
            }
        const half8* const xi = reinterpret_cast<const half8*>(x) + (size_t)im * cb * (h * w);
        half8* const yo = reinterpret_cast<half8*>(y) + (size_t)im * cb * (oh * ow) + (size_t)oy * ow + ox;
        auto pooled = [&](int b, float (&dst)[8]) {
            if (b < 0 || b >= cb) {
#pragma unroll
                for (int q = 0; q < 8; ++q) dst[q] = 0.0f;
                return;
            }
            const half8* const xp = xi + (size_t)b * (h * w);
            half8 v[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) v[t] = off[t] >= 0 ? xp[off[t]] : zero;
            const half8 m = pk_max3_nan(pk_max3_nan(v[0], v[1], v[2]), pk_max3_nan(v[3], v[4], v[5]), pk_max3_nan(v[6], v[7], v[8]));
#pragma unroll
            for (int q = 0; q < 8; ++q) dst[q] = (8 * b + q < c) ? (float)m[q] : 0.0f;
        };
        float prev[8], cur[8], nxt[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) prev[q] = 0.0f;
        pooled(0, cur);
        for (int b = 0; b < cb; ++b) {
            pooled(b + 1, nxt);
            float ext[12];                        // channels 8 b - 2 .. 8 b + 9
            ext[0] = prev[6]; ext[1] = prev[7];
#pragma unroll
            for (int q = 0; q < 8; ++q) ext[2 + q] = cur[q];
            ext[10] = nxt[0]; ext[11] = nxt[1];
            half8 o;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                float s_ = ext[q] * ext[q];
#pragma unroll
                for (int t = 1; t < 5; ++t) s_ = s_ + ext[q + t] * ext[q + t];
                o[q] = (_Float16)lrn_div(ext[q + 2], bias + alpha * s_, beta, BETA_MODE);
            }
            yo[(size_t)b * (oh * ow)] = o;
#pragma unroll
            for (int q = 0; q < 8; ++q) { prev[q] = cur[q]; cur[q] = nxt[q]; }
        }
    }
}

// LRN over five channels followed by MaxPool 3x3 (LRN.py:10-22 then MaxPool.py:41-72; GoogLeNet's conv2/norm2 -> pool2/3x3_s2) on fp16 c8
// tensors, one launch: the LRN tensor never exists.  A workgroup owns one image and a band of pooled rows, i.e. the input rows those
// windows touch; a lane owns up to PPT pixels of the band and walks the channel blocks with the values of three consecutive blocks in
// registers as fp32 (the window of channel 8 b + q reaches two channels into the neighbour blocks; squares summed in ascending channel
// order), leaves the normalised block of its pixels in LDS as fp16 (16 bytes per pixel: the fp16 rounding the reference's float16 LRN
// tensor has too), and after a barrier the workgroup pools the block: nine 16-byte LDS reads per output (a cell of the padding: zeros; a
// cell past the padded edge repeats the first), a NaN wins.
template <int BETA_MODE, int PPT>
__global__ __launch_bounds__(kBlock) void lrn_maxpool3x3_c8_kernel(const _Float16* __restrict__ x, _Float16* __restrict__ y, int n, int cb, int c, int h, int w,
                                                                   int oh, int ow, int sh, int sw, int pt, int pl, int hp, int wp, int R, int n_bands,
                                                                   float alpha, float beta, float bias) {
    extern __shared__ __attribute__((aligned(16))) char lp_lds[];
    half8* const tile = reinterpret_cast<half8*>(lp_lds);                // [band pixels]
    const half8 zero = half8{0, 0, 0, 0, 0, 0, 0, 0};
    const int tid  = threadIdx.x;
    const int img  = blockIdx.x / n_bands, band = blockIdx.x - img * n_bands;
    const int oy0  = band * R, oy1 = min(oh, oy0 + R);
    const int iy_lo = max(0, oy0 * sh - pt), iy_hi = min(h, (oy1 - 1) * sh + 3 - pt);
    const int band_px = (iy_hi - iy_lo) * w;
    const int hw = h * w, ohw = oh * ow;
    const half8* const xi = reinterpret_cast<const half8*>(x) + (size_t)img * cb * hw + (size_t)iy_lo * w;
    // ---- pooling geometry of this lane's output (one per lane: R * ow <= 256)
    const int  oyl = tid / ow, ox = tid - oyl * ow;
    const bool pact = oyl < oy1 - oy0;
    int off[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s2 = 0; s2 < 3; ++s2) {
            const int oy = oy0 + (pact ? oyl : 0), oxx = pact ? ox : 0;
            const int py = oy * sh + r, px = oxx * sw + s2;
            const bool inwin = py < hp && px < wp;
            const int cy = (inwin ? py : oy * sh) - pt, cx = (inwin ? px : oxx * sw) - pl;
            off[3 * r + s2] = (cy >= 0 && cy < h && cx >= 0 && cx < w) ? (cy - iy_lo) * w + cx : -1;
        }
    half8* const yo = reinterpret_cast<half8*>(y) + (size_t)img * cb * ohw + (size_t)(oy0 + (pact ? oyl : 0)) * ow + (pact ? ox : 0);

    float prev[PPT][8], cur[PPT][8], nxt[PPT][8];
    auto load_block = [&](int b, float (&dst)[PPT][8]) {
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int p = tid + i * kBlock;
            half8 v = zero;
            if (b < cb && p < band_px) v = xi[(size_t)b * hw + p];
#pragma unroll
            for (int q = 0; q < 8; ++q) dst[i][q] = (8 * b + q < c) ? (float)v[q] : 0.0f;
        }
    };
#pragma unroll
    for (int i = 0; i < PPT; ++i)
#pragma unroll
        for (int q = 0; q < 8; ++q) prev[i][q] = 0.0f;
    load_block(0, cur);
    for (int b = 0; b < cb; ++b) {
        load_block(b + 1, nxt);
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int p = tid + i * kBlock;
            float ext[12];
            ext[0] = prev[i][6]; ext[1] = prev[i][7];
#pragma unroll
            for (int q = 0; q < 8; ++q) ext[2 + q] = cur[i][q];
            ext[10] = nxt[i][0]; ext[11] = nxt[i][1];
            half8 o;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                float s_ = ext[q] * ext[q];
#pragma unroll
                for (int t = 1; t < 5; ++t) s_ = s_ + ext[q + t] * ext[q + t];
                o[q] = (_Float16)lrn_div(ext[q + 2], bias + alpha * s_, beta, BETA_MODE);
            }
            if (p < band_px) tile[p] = o;
        }
        __syncthreads();
        if (pact) {
            half8 v[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) v[t] = off[t] >= 0 ? tile[off[t]] : zero;
            yo[(size_t)b * ohw] = pk_max3_nan(pk_max3_nan(v[0], v[1], v[2]), pk_max3_nan(v[3], v[4], v[5]), pk_max3_nan(v[6], v[7], v[8]));
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PPT; ++i)
#pragma unroll
            for (int q = 0; q < 8; ++q) { prev[i][q] = cur[i][q]; cur[i][q] = nxt[i][q]; }
    }
}

// AvgPool (AvgPool.py:41-59: the mean of in[y s : min(h - 1, y s + kh), x s : min(w - 1, x s + kw)], no padding -- GoogLeNet's 7x7 pool
// averages the top-left 6x6) on an fp16 c8 tensor; the output is fp32 NCHW (the classifier behind it is dense): one lane per (image,
// channel block, output pixel), a sequential fp32 sum in the window's row-major order, as avgpool2d_kernel.
__global__ __launch_bounds__(kBlock) void avgpool_c8_kernel(const _Float16* __restrict__ x, float* __restrict__ y, int n, int cb, int c, int h, int w, int oh,
                                                            int ow, int kh, int kw, int sh, int sw) {
    const size_t total = (size_t)n * cb * oh * ow;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int ox = (int)(e % ow);
        size_t    f  = e / ow;
        const int oy = (int)(f % oh); f /= oh;
        const int b = (int)(f % cb), im = (int)(f / cb);
        const half8* const xp = reinterpret_cast<const half8*>(x) + ((size_t)im * cb + b) * (size_t)(h * w);
        const int y0 = oy * sh, x0 = ox * sw;
        const int y1 = min(y0 + kh, h - 1), x1 = min(x0 + kw, w - 1);
        float sum[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        int   cnt = 0;
        for (int iy = y0; iy < y1; ++iy)
            for (int ix = x0; ix < x1; ++ix) {
                const half8 v = xp[iy * w + ix];
#pragma unroll
                for (int q = 0; q < 8; ++q) sum[q] += (float)v[q];
                ++cnt;
            }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int ch = 8 * b + q;
            // (rounded to fp16: the reference's AvgPool of a float16 tensor returns float16 -- AvgPool.py:57-58, res dtype = input dtype; kept in an fp32 tensor)
            if (ch < c) y[(((size_t)im * c + ch) * oh + oy) * ow + ox] = cnt > 0 ? (float)(_Float16)(sum[q] / (float)cnt) : NAN;
        }
    }
}

// MaxPool 3x3 -> LRN -> 1x1 convolution (+ bias, ReLU) on blocked fp16 tensors as ONE launch (round 5; the FP16-IR twin of
// maxpool3x3_lrn_conv1x1_kernel of pvhip_norm.hip: GoogLeNet's pool1 -> norm1 -> conv2/3x3_reduce).  maxpool3x3_lrn_c8_kernel holds, block
// after block, the eight normalised channels of ITS pixel as one 16-byte piece -- two B operands of v_mfma_f32_32x32x4_2b_f16, whose two blocks
// take four k-values per LANE (lane l: column l & 31 of block l >> 5): D[k][pixel] += W[k][4 c'..4 c' + 3] . lrn[4 c'..][pixel], fp32
// accumulation.  A = the weights rounded to fp16 once (the constants of an FP16 IR are fp16 values) and transposed into LDS as
// wl[c / 4][k][4].  Epilogue as conv_f16_c8m_kernel's: bias, ReLU, fp16, v_permlane32_swap between the lane halves, one 16-byte blocked
// piece per lane -- for the pixel of lane 32 b + (l & 31), whose output index comes over by a wave shuffle.
template <int BETA_MODE, int KT>
__global__ __launch_bounds__(kBlock) void maxpool3x3_lrn_conv1x1_c8_kernel(const _Float16* __restrict__ x, _Float16* __restrict__ y, const float* __restrict__ cw,
                                                                           const float* __restrict__ cbias, int n, int cb, int c, int h, int w, int oh, int ow,
                                                                           int sh, int sw, int pt, int pl, int hp, int wp, float alpha, float beta, float bias,
                                                                           int k_out, int act) {
    typedef float floatx32 __attribute__((ext_vector_type(32)));
    constexpr int KP = 32 * KT;
    __shared__ __attribute__((aligned(16))) half4 wl[16][KP];                 // [input channel / 4][output channel]: cb <= 8 blocks = 16 quads
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    for (int e = tid; e < 2 * cb * KP; e += kBlock) {
        const int q4 = e / KP, k = e - q4 * KP;
        half4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (k < k_out && 4 * q4 + j < c) ? (_Float16)cw[(size_t)k * c + 4 * q4 + j] : (_Float16)0.0f;
        wl[q4][k] = v;
    }
    __syncthreads();
    const size_t total = (size_t)n * oh * ow;
    const half8 zero = half8{0, 0, 0, 0, 0, 0, 0, 0};
    const int ohw = oh * ow;
    const int kbt = (k_out + 15) / 16 * 2;                                    // blocks of the output tensor
    const int l31 = lane & 31, lh = lane >> 5;
    for (size_t e0 = (size_t)blockIdx.x * blockDim.x; e0 < total; e0 += (size_t)gridDim.x * blockDim.x) {       // (workgroup-uniform: every lane takes part in the MFMAs)
        const size_t e = e0 + tid;
        const bool live = e < total;
        const size_t ee = live ? e : 0;
        const int ox = (int)(ee % ow);
        const size_t f = ee / ow;
        const int oy = (int)(f % oh), im = (int)(f / oh);
        int off[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int s2 = 0; s2 < 3; ++s2) {
                const int py = oy * sh + r, px = ox * sw + s2;
                const bool inwin = py < hp && px < wp;
                const int cy = (inwin ? py : oy * sh) - pt, cx = (inwin ? px : ox * sw) - pl;
                off[3 * r + s2] = (cy >= 0 && cy < h && cx >= 0 && cx < w) ? cy * w + cx : -1;
            }
        const half8* const xi = reinterpret_cast<const half8*>(x) + (size_t)im * cb * (h * w);
        auto pooled = [&](int b, float (&dst)[8]) {
            if (b < 0 || b >= cb) {
#pragma unroll
                for (int q = 0; q < 8; ++q) dst[q] = 0.0f;
                return;
            }
            const half8* const xp = xi + (size_t)b * (h * w);
            half8 v[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) v[t] = off[t] >= 0 ? xp[off[t]] : zero;
            const half8 m = pk_max3_nan(pk_max3_nan(v[0], v[1], v[2]), pk_max3_nan(v[3], v[4], v[5]), pk_max3_nan(v[6], v[7], v[8]));
#pragma unroll
            for (int q = 0; q < 8; ++q) dst[q] = (8 * b + q < c) ? (float)m[q] : 0.0f;
        };
        floatx32 acc[KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 32; ++r) acc[kt][r] = 0.0f;
        float prev[8], cur[8], nxt[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) prev[q] = 0.0f;
        pooled(0, cur);
        for (int b = 0; b < cb; ++b) {
            pooled(b + 1, nxt);
            float ext[12];                        // channels 8 b - 2 .. 8 b + 9
            ext[0] = prev[6]; ext[1] = prev[7];
#pragma unroll
            for (int q = 0; q < 8; ++q) ext[2 + q] = cur[q];
            ext[10] = nxt[0]; ext[11] = nxt[1];
            half4 o[2];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                float s_ = ext[q] * ext[q];
#pragma unroll
                for (int t = 1; t < 5; ++t) s_ = s_ + ext[q + t] * ext[q + t];
                const _Float16 v = (_Float16)lrn_div(ext[q + 2], bias + alpha * s_, beta, BETA_MODE);      // (the fp16 value maxpool3x3_lrn_c8_kernel stores)
                o[q >> 2][q & 3] = live ? v : (_Float16)0.0f;
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int kt = 0; kt < KT; ++kt)
                    acc[kt] = __builtin_amdgcn_mfma_f32_32x32x4f16(wl[2 * b + s2][32 * kt + l31], o[s2], acc[kt], 0, 0, 0);
#pragma unroll
            for (int q = 0; q < 8; ++q) { prev[q] = cur[q]; cur[q] = nxt[q]; }
        }
        // ---- epilogue: register 16 b2 + 4 g + j of acc[kt] at lane (l31, lh) = output channel 32 kt + 8 g + 4 lh + j of the pixel of lane 32 b2 + l31
        const long opix = live ? (long)im * kbt * ohw + (long)oy * ow + ox : -1;
        long opix_b[2];
        opix_b[0] = ((long)__shfl((int)(opix >> 32), l31, kWave) << 32) | (unsigned)__shfl((int)opix, l31, kWave);
        opix_b[1] = ((long)__shfl((int)(opix >> 32), 32 + l31, kWave) << 32) | (unsigned)__shfl((int)opix, 32 + l31, kWave);
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int gp = 0; gp < 2; ++gp) {
                float bs[2][4];
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int kk = 32 * kt + 8 * (2 * gp + h2) + 4 * lh + j;
                        bs[h2][j] = (cbias != nullptr && kk < k_out) ? cbias[kk] : 0.0f;
                    }
                const int blk = 4 * kt + 2 * gp + lh;            // the block this lane holds after the swap
#pragma unroll
                for (int b2 = 0; b2 < 2; ++b2) {
                    unsigned w0[2], w1[2];
#pragma unroll
                    for (int h2 = 0; h2 < 2; ++h2) {
                        half4 hv;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            float v = acc[kt][16 * b2 + 4 * (2 * gp + h2) + j] + bs[h2][j];
                            if (act != 0) v = __builtin_elementwise_maximum(v, 0.0f);
                            hv[j] = (_Float16)v;
                        }
                        const uint2 u = __builtin_bit_cast(uint2, hv);
                        if (h2 == 0) { w0[0] = u.x; w0[1] = u.y; } else { w1[0] = u.x; w1[1] = u.y; }
                    }
                    const auto s0 = __builtin_amdgcn_permlane32_swap(w0[0], w1[0], false, false);
                    const auto s1 = __builtin_amdgcn_permlane32_swap(w0[1], w1[1], false, false);
                    uint4v piece;
                    piece[0] = s0[0]; piece[1] = s1[0]; piece[2] = s0[1]; piece[3] = s1[1];
                    if (opix_b[b2] >= 0 && blk < kbt)
                        *reinterpret_cast<uint4v*>(y + ((size_t)opix_b[b2] + (size_t)blk * ohw) * 8) = piece;
                }
            }
    }
}

}  // namespace

extern "C" {

int pvhip_maxpool3x3_c8(const void* x, void* y, int n, int c, int h, int w, int oh, int ow, int sh, int sw,
                        int pad_top, int pad_left, int pad_bottom, int pad_right) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(n >= 0 && c > 0 && h > 0 && w > 0 && oh > 0 && ow > 0 && sh > 0 && sw > 0 && pad_top >= 0 && pad_left >= 0 && pad_bottom >= 0 && pad_right >= 0);
    const int hp = h + pad_top + pad_bottom, wp = w + pad_left + pad_right;
    PVHIP_CHECK_ARG((oh - 1) * sh < hp && (ow - 1) * sw < wp);
    if (n == 0) return PVHIP_OK;
    PVHIP_CHECK_ARG(x != nullptr && y != nullptr);
    const int cb = c8_blocks(c);
    const size_t total = (size_t)n * cb * oh * ow;
    hipLaunchKernelGGL(maxpool3x3_c8_kernel, dim3(grid_for(total)), dim3(kBlock), 0, state().stream, static_cast<const _Float16*>(x),
                       static_cast<_Float16*>(y), n, cb, h, w, oh, ow, sh, sw, pad_top, pad_left, hp, wp);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

/* ... and with the 1x1 / stride 1 / unpadded convolution behind the LRN in the same launch (ABI v15; the FP16-IR twin of pvhip_maxpool_lrn_conv1x1_f32):
 * x: c8 (n, c, h, w), c <= 64; w_oihw: the (k_out, c, 1, 1) fp32 weights (holding fp16 values), k_out <= 64; y: c8 (n, k_out, oh, ow); act none / ReLU. */
int pvhip_maxpool3x3_lrn_conv1x1_c8_supported(int c, int k_out, int size) { return (c > 0 && c <= 64 && k_out > 0 && k_out <= 64 && size == 5) ? 1 : 0; }

int pvhip_maxpool3x3_lrn_conv1x1_c8(const void* x, const float* w_oihw, void* y, int n, int c, int h, int w, int oh, int ow, int sh, int sw,
                                    int pad_top, int pad_left, int pad_bottom, int pad_right, int size, float alpha, float beta, float bias,
                                    int k_out, const float* conv_bias, int act) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(n >= 0 && c > 0 && h > 0 && w > 0 && oh > 0 && ow > 0 && sh > 0 && sw > 0 && pad_top >= 0 && pad_left >= 0 && pad_bottom >= 0 && pad_right >= 0);
    PVHIP_CHECK_ARG(act == 0 || act == 1);
    if (!pvhip_maxpool3x3_lrn_conv1x1_c8_supported(c, k_out, size))
        return fail(PVHIP_EUNSUPPORTED, "pvhip_maxpool3x3_lrn_conv1x1_c8: a window of five channels, at most 64 channels either side");
    const int hp = h + pad_top + pad_bottom, wp = w + pad_left + pad_right;
    PVHIP_CHECK_ARG((oh - 1) * sh < hp && (ow - 1) * sw < wp);
    if ((unsigned long long)n * 64 * oh * ow >= (1ull << 31)) return fail(PVHIP_EUNSUPPORTED, "pvhip_maxpool3x3_lrn_conv1x1_c8: tensor too large");
    if (n == 0) return PVHIP_OK;
    PVHIP_CHECK_ARG(x != nullptr && y != nullptr && w_oihw != nullptr);
    const int cb = c8_blocks(c);
    const int bm = lrn_beta_mode(beta, bias);
    const size_t total = (size_t)n * oh * ow;
    const int kt = (k_out + 31) / 32;
#define PVM_PLC(BM_, KT_) hipLaunchKernelGGL((maxpool3x3_lrn_conv1x1_c8_kernel<BM_, KT_>), dim3(grid_for(total)), dim3(kBlock), 0, state().stream,                   \
                                             static_cast<const _Float16*>(x), static_cast<_Float16*>(y), w_oihw, conv_bias, n, cb, c, h, w, oh, ow, sh, sw, pad_top, \
                                             pad_left, hp, wp, alpha, beta, bias, k_out, act)
    if (bm == 4) { if (kt == 1) PVM_PLC(4, 1); else PVM_PLC(4, 2); }
    else if (bm == 1) { if (kt == 1) PVM_PLC(1, 1); else PVM_PLC(1, 2); }
    else { if (kt == 1) PVM_PLC(0, 1); else PVM_PLC(0, 2); }
#undef PVM_PLC
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

int pvhip_maxpool3x3_lrn_c8(const void* x, void* y, int n, int c, int h, int w, int oh, int ow, int sh, int sw,
                            int pad_top, int pad_left, int pad_bottom, int pad_right, int size, float alpha, float beta, float bias) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(n >= 0 && c > 0 && h > 0 && w > 0 && oh > 0 && ow > 0 && sh > 0 && sw > 0 && pad_top >= 0 && pad_left >= 0 && pad_bottom >= 0 && pad_right >= 0);
    if (size != 5) return fail(PVHIP_EUNSUPPORTED, "pvhip_maxpool3x3_lrn_c8: a window of five channels");
    const int hp = h + pad_top + pad_bottom, wp = w + pad_left + pad_right;
    PVHIP_CHECK_ARG((oh - 1) * sh < hp && (ow - 1) * sw < wp);
    if (n == 0) return PVHIP_OK;
    PVHIP_CHECK_ARG(x != nullptr && y != nullptr);
    const int cb = c8_blocks(c);
    const int bm = lrn_beta_mode(beta, bias);
    const size_t total = (size_t)n * oh * ow;
#define PVM_PL(BM_) hipLaunchKernelGGL((maxpool3x3_lrn_c8_kernel<BM_>), dim3(grid_for(total)), dim3(kBlock), 0, state().stream, static_cast<const _Float16*>(x), \
                                       static_cast<_Float16*>(y), n, cb, c, h, w, oh, ow, sh, sw, pad_top, pad_left, hp, wp, alpha, beta, bias)
    switch (bm) {
        case 4: PVM_PL(4); break;
        case 1: PVM_PL(1); break;
        case 2: PVM_PL(2); break;
        case 3: PVM_PL(3); break;
        default: PVM_PL(0); break;
    }
#undef PVM_PL
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

int pvhip_avgpool_c8(const void* x, float* y, int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh, int sw) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(n >= 0 && c > 0 && h > 0 && w > 0 && oh > 0 && ow > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0);
    if (n == 0) return PVHIP_OK;
    PVHIP_CHECK_ARG(x != nullptr && y != nullptr);
    const int cb = c8_blocks(c);
    hipLaunchKernelGGL(avgpool_c8_kernel, dim3(grid_for((size_t)n * cb * oh * ow)), dim3(kBlock), 0, state().stream, static_cast<const _Float16*>(x), y, n, cb, c,
                       h, w, oh, ow, kh, kw, sh, sw);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

int pvhip_lrn_maxpool3x3_c8_supported(int h, int w, int oh, int ow, int sh, int sw, int pad_top, int pad_left, int size) {
    if (size != 5 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || sh <= 0 || sw <= 0 || ow > kBlock) return 0;
    int R = kBlock / ow;                                     // one pooled output per lane
    if (R > oh) R = oh;
    while (R > 1 && ((R - 1) * sh + 3) * w > 4 * kBlock) --R;        // and at most four band pixels per lane
    return (((R - 1) * sh + 3) * w <= 4 * kBlock) ? R : 0;
}

int pvhip_lrn_maxpool3x3_c8(const void* x, void* y, int n, int c, int h, int w, int size, float alpha, float beta, float bias,
                            int oh, int ow, int sh, int sw, int pad_top, int pad_left, int pad_bottom, int pad_right) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(n >= 0 && c > 0 && pad_top >= 0 && pad_left >= 0 && pad_bottom >= 0 && pad_right >= 0);
    const int R = pvhip_lrn_maxpool3x3_c8_supported(h, w, oh, ow, sh, sw, pad_top, pad_left, size);
    if (R == 0) return fail(PVHIP_EUNSUPPORTED, "pvhip_lrn_maxpool3x3_c8: a window of five channels, pooled rows of at most %d outputs, bands of at most %d pixels", kBlock, 4 * kBlock);
    const int hp = h + pad_top + pad_bottom, wp = w + pad_left + pad_right;
    PVHIP_CHECK_ARG((oh - 1) * sh < hp && (ow - 1) * sw < wp);
    if (n == 0) return PVHIP_OK;
    PVHIP_CHECK_ARG(x != nullptr && y != nullptr);
    const int cb = c8_blocks(c);
    const int n_bands = (oh + R - 1) / R;
    const int rows_in = (R - 1) * sh + 3;
    const int ppt = (rows_in * w + kBlock - 1) / kBlock;
    const size_t lds = (size_t)rows_in * w * 16;
    const int bm = lrn_beta_mode(beta, bias) == 4 ? 4 : (lrn_beta_mode(beta, bias) == 1 ? 1 : 0);
    const dim3 grid((unsigned)(n * n_bands));
#define PVM_LP(BM_, PPT_) hipLaunchKernelGGL((lrn_maxpool3x3_c8_kernel<BM_, PPT_>), grid, dim3(kBlock), lds, state().stream, static_cast<const _Float16*>(x), \
                                             static_cast<_Float16*>(y), n, cb, c, h, w, oh, ow, sh, sw, pad_top, pad_left, hp, wp, R, n_bands, alpha, beta, bias)
#define PVM_LP_P(BM_) { if (ppt <= 1) PVM_LP(BM_, 1); else if (ppt <= 2) PVM_LP(BM_, 2); else PVM_LP(BM_, 4); }
    if (bm == 4) PVM_LP_P(4) else if (bm == 1) PVM_LP_P(1) else PVM_LP_P(0)
#undef PVM_LP_P
#undef PVM_LP
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
