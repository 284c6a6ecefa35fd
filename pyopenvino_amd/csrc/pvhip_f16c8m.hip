// FP16 IRs, second step of the fp16 tensors (the reference holds EVERY tensor of an FP16 IR in float16, common_def.py:13-17):
// convolutions that read fp16 blocked by eight channels ("c8", pvhip_f16_c8.h) and WRITE it -- the inception modules of GoogLeNet from
// the module input to the channel Concat without an fp32 tensor in between:
//   * several 1x1 convolutions of the same input as one launch (the 1x1 / 3x3_reduce / 5x5_reduce arms), each output-channel tile storing
//     into the tensor of its member: an fp16 c8 tensor of its own, a channel range of the module's c8 Concat buffer, or (fallback) fp32 NCHW;
//   * the 3x3 / 5x5 convolutions behind the reduce arms, writing their range of the Concat buffer;
//   * MaxPool 3x3 / stride 1 / pad 1 + pool_proj: the pooled operand is the maximum of the nine shifted LDS reads (v_pk_maximum3_f16: a NaN
//     wins, as for np.max; the zeros the copy wrote for cells outside the image are the zero padding MaxPool.py:53 pads with).
// Same roles as conv_f16_c8_kernel (a producer wave copies whole rows by LDS-DMA, four consumer waves own a 32-channel tile each), with
//   * LDS rows of 8 / 16 / 32 / 64 pixels (the smallest power of two that holds W + 2 pad): one copy instruction moves 8 / 4 / 2 / 1 rows,
//     a 14-wide stage is 2-3 instructions per channel block instead of 9;
//   * 1x1 windows: a stage is FOUR 16-channel steps (eight channel blocks), so that a barrier is worth 16 MFMAs;
//   * the MFMA with the WEIGHT fragment first: an accumulator is [channel][pixel], a lane holds four consecutive channels of its pixel
//     per register group -- 8 bytes of a c8 piece, which the other lane half completes to 16.
// The fragment panel, the row-tile plan (without conv_f16_c8_kernel's cap on LDS rows), the counted wait and pk_max3_nan are those of
// pvhip_f16_c8.h; the pooling, LRN and average kernels on the same tensors are pvhip_f16c8pool.hip.
#include "pvhip_f16_c8.h"

using namespace pvhip;

namespace {

constexpr int kMMaxThreads = 512;   // four consumer waves + one to four producer waves (C8mArgs.nprod)
constexpr int kMMaxBuf  = 6;
constexpr int kMSteps   = 4;        // 16-channel steps per stage of a 1x1 window

struct C8mSeg {
    void* y;
    int   m_begin, k;        // first panel row of the member, its real output channels
    int   layout;            // 0: fp32 NCHW; 1: fp16 c8
    int   ctotal, coff;      // channels of the tensor y points into and this member's first channel in it (c8: multiples of 8)
    int   nblk;              // c8: channel blocks this member writes (a tensor of its own: ceil16(k) / 8, zeros included; a range: k / 8)
};

struct C8mArgs {
    const _Float16* xb;      // [N][CB][H*W][8]
    const _Float16* wf;      // [n_mtiles][CB / 2][taps][tm][64 lanes][8 halves]  (the fragment panel of pvhip_f16_c8.h)
    const float*    bias;    // [Kp] or null
    int N, CB, H, W, Kp;
    int tm, n_mtiles, tiles_per_image, n_tiles;
    int R, rows, rows_pad, stride_sh;      // output rows per tile; LDS rows a stage needs / holds (a multiple of 64 >> stride_sh) per channel block; log2 of the LDS row length in pixels
    int n_ins, nbuf, stages;               // copy instructions per stage; stage buffers; stages per tile
    int reg_copy;                          // producers copy through registers (global load + ds_write) instead of LDS-DMA
    int tpw2;                              // consumers own two channel tiles and half the pixel blocks each (groups of three or four tiles)
    int abl;                               // diagnostic build (PVHIP_CONV_ABLATE bits; wrong results on purpose): 1 every consumer loads channel tile 0's weight fragments (one
                                           // set of lines per workgroup: how much is the L2 -> CU traffic of the weights?), 2 no weight loads at all, 4 no stores,
                                           // 16 no copies  (nothing inside the tap loop: a uniform branch there costs a vmcnt(0) per tap, lesson 51 -- an ablation of the
                                           // LDS reads that way made the whole launch 25 % slower and measured itself)
    int nprod;                             // producer waves: the copy instructions of a stage are dealt out to them (a wave issues one per ~200 cycles)
    unsigned x_bytes, wf_bytes;
    int   act;
    float lo, hi;
    int   nseg;
    C8mSeg seg[PVHIP_MAX_CONV_DESTS];
};

// The consumer side of conv_f16_c8m_kernel: TW channel tiles (tile0 ..) x NBW pixel blocks (blk0 ..) of the workgroup's tile.
template <int KS, int NBW, bool POOL, int TW>
__device__ __forceinline__ void c8m_consume(const C8mArgs& a, const char* const c8m_lds, const int lane, const int tile0, const int blk0, const int mt,
                                            const int img, const int oy0, const int npx) {
    constexpr int TAPSW = KS * KS;
    constexpr int TAPS  = KS == 1 ? kMSteps : TAPSW;
    constexpr int BLK   = KS == 1 ? 2 * kMSteps : 2;
    constexpr int RING  = KS == 1 ? kMSteps : KS;
    const int l31 = lane & 31, lh = lane >> 5;
    const int HW     = a.H * a.W;
    const int ncs16  = a.CB >> 1;
    const int stride = 1 << a.stride_sh;
    const unsigned blk_bytes = (unsigned)(a.rows_pad * stride) * 16u;
    const unsigned buf_bytes = blk_bytes * BLK;
    const int S = a.stages;
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(a.wf), 0, a.wf_bytes, 0x00020000);

    unsigned pixoff[NBW];
#pragma unroll
    for (int nb = 0; nb < NBW; ++nb) {
        const int p  = 32 * (blk0 + nb) + l31;
        const int pc = p < a.R * a.W ? p : 0;
        const int pr = pc / a.W, px = pc - pr * a.W;
        pixoff[nb] = (unsigned)lh * blk_bytes + (unsigned)((pr * stride + px) * 16);
    }
    floatx16 acc[TW][NBW];
#pragma unroll
    for (int i = 0; i < TW; ++i)
#pragma unroll
        for (int nb = 0; nb < NBW; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][nb][r] = 0.0f;

#ifdef PVHIP_DIAG
    const int abl = a.abl;
#else
    constexpr int abl = 0;
#endif
    unsigned wlane[TW];
#pragma unroll
    for (int i = 0; i < TW; ++i) wlane[i] = (abl & 2) ? kOob : (unsigned)lane * 16u + ((abl & 1) ? 0u : (unsigned)(tile0 + i) * 1024u);
    // fragment of MFMA step t of stage cs: window taps (KS > 1): 16-channel step cs, tap t; 1x1: 16-channel step cs * 4 + t (past the
    // last one: an out-of-range offset, zeros -- the copy wrote zeros for those channel blocks too)
#define PVM_LOAD_A(dst_, cs_, t_)                                                                                \
    {                                                                                                            \
        const int c16_ = KS == 1 ? (cs_) * kMSteps + (t_) : (cs_);                                               \
        const int tap_ = KS == 1 ? 0 : (t_);                                                                     \
        const unsigned so_ = (unsigned)((((mt * ncs16 + min(c16_, ncs16 - 1)) * TAPSW + tap_) * a.tm) * 1024);   \
        _Pragma("unroll") for (int i = 0; i < TW; ++i)                                                           \
            dst_[i] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(wr, c16_ < ncs16 ? wlane[i] : kOob, so_, 0)); \
    }
    half8 af[RING][TW];
#pragma unroll
    for (int s = 0; s < RING; ++s) PVM_LOAD_A(af[s], 0, s);
    unsigned sb = 0;
    for (int cs = 0; cs < S; ++cs) {
        asm volatile("s_barrier" ::: "memory");
        const char* const buf = c8m_lds + sb * buf_bytes;
        sb = sb + 1 == (unsigned)a.nbuf ? 0u : sb + 1;
        const int cs_x = cs + 1 < S ? cs + 1 : cs;                       // the stage the ring's tail prefetches (the last stage: its own again, unused)
        half8 b8[2][NBW];
        // pixel operand of MFMA step t: window taps: channel blocks (0, 1), shifted by the tap; 1x1: channel blocks (2 t, 2 t + 1);
        // pooled: the maximum over the 3x3 window of those
#define PVM_READ_B(dst_, t_)                                                                                     \
    _Pragma("unroll") for (int nb = 0; nb < NBW; ++nb) {                                                         \
        if (POOL) {                                                                                              \
            const char* const p0_ = buf + pixoff[nb] + (unsigned)(2 * (t_)) * blk_bytes;                         \
            half8 m_[3];                                                                                         \
            _Pragma("unroll") for (int g = 0; g < 3; ++g)                                                        \
                m_[g] = pk_max3_nan(*reinterpret_cast<const half8*>(p0_ + (unsigned)((g * stride + 0) * 16)),   \
                                    *reinterpret_cast<const half8*>(p0_ + (unsigned)((g * stride + 1) * 16)),   \
                                    *reinterpret_cast<const half8*>(p0_ + (unsigned)((g * stride + 2) * 16)));  \
            dst_[nb] = pk_max3_nan(m_[0], m_[1], m_[2]);                                                         \
        } else if (KS == 1) {                                                                                    \
            dst_[nb] = *reinterpret_cast<const half8*>(buf + pixoff[nb] + (unsigned)(2 * (t_)) * blk_bytes);     \
        } else {                                                                                                 \
            dst_[nb] = *reinterpret_cast<const half8*>(buf + pixoff[nb] + (unsigned)((((t_) / KS) * stride + ((t_) % KS)) * 16)); \
        }                                                                                                        \
    }
        if (!POOL) PVM_READ_B(b8[0], 0);
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            // window taps / 1x1: the operands of step t + 1 are read in front of the MFMAs of step t; pooled: step by step (nine reads and
            // four maxima per operand: two steps of them in flight are registers the accumulators do not leave)
            if (POOL) { PVM_READ_B(b8[t & 1], t); }
            else if (t + 1 < TAPS) { PVM_READ_B(b8[(t + 1) & 1], t + 1); }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < TW; ++i)
#pragma unroll
                for (int nb = 0; nb < NBW; ++nb) acc[i][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[t % RING][i], b8[t & 1][nb], acc[i][nb], 0, 0, 0);
            if (t + RING < TAPS) PVM_LOAD_A(af[t % RING], cs, t + RING)
            else                 PVM_LOAD_A(af[t % RING], cs_x, t + RING - TAPS)
            __builtin_amdgcn_sched_barrier(0);
        }
#undef PVM_READ_B
    }
#undef PVM_LOAD_A

    // ---- epilogue: register 4 g + j of accumulator (i, nb) is panel row row0t + 8 g + 4 lh + j of tile pixel 32 (blk0 + nb) + l31
    const ActBounds ab = act_bounds(a.act, a.lo, a.hi);
    typedef const __attribute__((address_space(4))) float* const_float_p;
    const const_float_p bias_c = (const_float_p)(unsigned long)a.bias;
    // the member table is read through the kernarg pointer (indexed as an ordinary argument array it would be copied to scratch)
    typedef const __attribute__((address_space(4))) C8mArgs* kernarg_p;
    kernarg_p ka = (kernarg_p)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    const int P0 = oy0 * a.W + 32 * blk0 + l31;
    const int p0 = 32 * blk0 + l31;                                      // the lane's pixel of block 0 inside the tile
#pragma unroll
    for (int i = 0; i < TW; ++i) {
        const int row0t = (mt * a.tm + tile0 + i) * 32;                  // first panel row of this channel tile
        int sg = 0;
        for (int q = 1; q < a.nseg; ++q) sg = row0t >= ka->seg[q].m_begin ? q : sg;
        const int m_rel = row0t - ka->seg[sg].m_begin;                   // multiple of 32
        const int kreal = ka->seg[sg].k;
        if (ka->seg[sg].layout == 1) {
            _Float16* const yh = static_cast<_Float16*>(ka->seg[sg].y);
            const int cbt = ka->seg[sg].ctotal >> 3, cb0 = (ka->seg[sg].coff + m_rel) >> 3, nblk = ka->seg[sg].nblk - (m_rel >> 3);
            // Two register groups at a time: group g0 = 2 gp holds channels 8 g0 + 4 lh .. + 3 of the lane's pixel, g1 = g0 + 1 the next block's.
            // v_permlane32_swap exchanges the upper lane half of one register with the lower half of another: afterwards a lane of the lower
            // half holds ALL EIGHT channels of block g0 and its partner in the upper half all eight of block g1 -- one 16-byte store per
            // lane instead of two 8-byte ones (a wave's stores leave at ~170 cycles apiece whatever their width: lesson 53).
#pragma unroll
            for (int gp = 0; gp < 2; ++gp) {
                float bs0[2][4], bs1[2][4];
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        bs0[h2][j] = bs1[h2][j] = -0.0f;
                        if (a.bias != nullptr) {
                            bs0[h2][j] = bias_c[min(row0t + 8 * (2 * gp + h2) + j, a.Kp - 1)];
                            bs1[h2][j] = bias_c[min(row0t + 8 * (2 * gp + h2) + 4 + j, a.Kp - 1)];
                        }
                    }
                const int  g_mine = 2 * gp + lh;
                const bool g_ok   = g_mine < nblk;
                _Float16* const yb = yh + (((size_t)img * cbt + cb0 + g_mine) * HW + P0) * 8;
#pragma unroll
                for (int nb = 0; nb < NBW; ++nb) {
                    unsigned w0[2], w1[2];                                // the lane's four channels of block g0 (w0) and g1 (w1) as two dwords each
#pragma unroll
                    for (int h2 = 0; h2 < 2; ++h2) {
                        half4 hv;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            float v = acc[i][nb][4 * (2 * gp + h2) + j] + (lh ? bs1[h2][j] : bs0[h2][j]);
                            if (a.act != 0) v = (v < ab.lo) ? ab.lo : v;
                            if (a.act == 2) v = (v > ab.hi) ? ab.hi : v;
                            hv[j] = (_Float16)v;
                        }
                        const uint2 u = __builtin_bit_cast(uint2, hv);
                        if (h2 == 0) { w0[0] = u.x; w0[1] = u.y; } else { w1[0] = u.x; w1[1] = u.y; }
                    }
                    uint4v piece;
                    {
                        const auto s0 = __builtin_amdgcn_permlane32_swap(w0[0], w1[0], false, false);   // s0[0]: lower half own g0, upper half partner's g1; s0[1]: lower half partner's g0, upper half own g1
                        const auto s1 = __builtin_amdgcn_permlane32_swap(w0[1], w1[1], false, false);
                        piece[0] = s0[0]; piece[1] = s1[0]; piece[2] = s0[1]; piece[3] = s1[1];         // channels 0-3 (two dwords), then 4-7
                    }
                    if (g_ok && p0 + 32 * nb < npx && !(abl & 4)) *reinterpret_cast<uint4v*>(yb + (size_t)(32 * nb) * 8) = piece;
                }
            }
        } else {
            float* const yf = static_cast<float*>(ka->seg[sg].y) + ((size_t)img * ka->seg[sg].ctotal + ka->seg[sg].coff + m_rel) * HW + P0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dr = (r & 3) + 8 * (r >> 2);
                float bs0 = -0.0f, bs1 = -0.0f;
                if (a.bias != nullptr) {
                    bs0 = bias_c[min(row0t + dr, a.Kp - 1)];
                    bs1 = bias_c[min(row0t + dr + 4, a.Kp - 1)];
                }
                const int kk = m_rel + dr + 4 * lh;
                if (kk >= kreal) continue;
#pragma unroll
                for (int nb = 0; nb < NBW; ++nb) {
                    float v = acc[i][nb][r] + (lh ? bs1 : bs0);
                    if (a.act != 0) v = (v < ab.lo) ? ab.lo : v;
                    if (a.act == 2) v = (v > ab.hi) ? ab.hi : v;
                    if (p0 + 32 * nb < npx) conv_store1(yf + (size_t)(dr + 4 * lh) * HW + 32 * nb, v);
                }
            }
        }
    }
}

// KS: window (1, 3, 5); NB: 32-pixel blocks of a tile (2 / 4); POOL (KS == 1): MaxPool 3x3 / stride 1 / pad 1 in front of the 1x1 window
template <int KS, int NB, bool POOL>
__global__ __launch_bounds__(kMMaxThreads, (KS == 5 && NB == 4) ? 3 : 4) void conv_f16_c8m_kernel(C8mArgs a) {
    static_assert(!POOL || KS == 1, "the pooled form is a 1x1 convolution");
    constexpr int PADG  = POOL ? 1 : (KS - 1) / 2;                       // halo of the copied rows
    constexpr int BLK   = KS == 1 ? 2 * kMSteps : 2;                     // channel blocks per stage
    extern __shared__ __attribute__((aligned(1024))) char c8m_lds[];     // [nbuf][BLK][rows_pad][stride][16 bytes]

    const int tid  = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wid  = __builtin_amdgcn_readfirstlane(tid / kWave);
    const int HW     = a.H * a.W;
    const int stride = 1 << a.stride_sh;
    const unsigned blk_bytes = (unsigned)(a.rows_pad * stride) * 16u;
    const unsigned buf_bytes = blk_bytes * BLK;
    const int S = a.stages;

    // tile = (channel group, image, row tile), the channel groups of a pixel tile back to back; XCD-aware as in conv_f16_c8_kernel
    const int tile = xcd_tile(blockIdx.x, gridDim.x);
    const int mt  = tile % a.n_mtiles, pt = tile / a.n_mtiles;
    const int img = pt / a.tiles_per_image;
    const int oy0 = (pt - img * a.tiles_per_image) * a.R;
    const int npx = min(a.R, a.H - oy0) * a.W;

    if (wid >= 4) {
        // ------------------------------------------------------------------ producers: copy instruction k of a stage (channel block k / q_n,
        // rows (k % q_n) * rpi ..) belongs to producer k % nprod
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(a.xb), 0, a.x_bytes, 0x00020000);
        const int  pw    = wid - 4;
        const int  rpi   = 64 >> a.stride_sh;                            // rows per copy instruction
        const int  lrow  = lane >> a.stride_sh;
        const int  x     = (lane & (stride - 1)) - PADG;
        const bool colok = x >= 0 && x < a.W;
        const int  iy0   = oy0 - PADG;
        const int  q_n   = a.rows_pad / rpi;
        const int  mine  = (a.n_ins - pw + a.nprod - 1) / a.nprod;       // this wave's copy instructions per stage
        int s_i = 0;
        auto issue_next = [&]() {
            char* const dst = c8m_lds + (unsigned)(s_i % a.nbuf) * buf_bytes;
            for (int k = pw; k < a.n_ins; k += a.nprod) {
#ifdef PVHIP_DIAG
                if (a.abl & 16) continue;
#endif
                const int  b    = k / q_n, q = k - b * q_n;
                const int  gb   = s_i * BLK + b;
                const bool bok  = gb < a.CB;
                const unsigned plane = (unsigned)((img * a.CB + (bok ? gb : 0)) * HW);
                const int  rr = q * rpi + lrow;
                const int  iy = iy0 + rr;
                const bool ok = bok && colok && rr < a.rows && iy >= 0 && iy < a.H;
                const unsigned vo = ok ? (plane + (unsigned)(iy * a.W + x)) * 16u : kOob;
                lds_dma_b128(xr, reinterpret_cast<float*>(dst + (unsigned)b * blk_bytes + (unsigned)q * 1024u), vo, 0u);
            }
            ++s_i;
        };
        if (a.reg_copy != 0) {
            // The other copy path (PVHIP_CONV_F16_C8_REG=1, up to eight copy instructions per wave and stage): global -> registers ->
            // ds_write_b128.  Loads of stage s + 1 fly while the consumers work on stage s, the writes go to the other buffer before
            // B(s + 1).  Ordinary loads leave a wave faster than LDS-DMA instructions do; they hold registers and lgkm slots instead.
            constexpr int MAXI = 8;
            uint4v regs[MAXI];
            auto load_stage = [&](int st) {
#pragma unroll
                for (int i = 0; i < MAXI; ++i) {
                    const int  k    = pw + i * a.nprod;
                    const int  kc   = k < a.n_ins ? k : 0;
                    const int  b    = kc / q_n, q = kc - b * q_n;
                    const int  gb   = st * BLK + b;
                    const bool bok  = gb < a.CB && k < a.n_ins;
                    const unsigned plane = (unsigned)((img * a.CB + (bok ? gb : 0)) * HW);
                    const int  rr = q * rpi + lrow;
                    const int  iy = iy0 + rr;
                    const bool ok = bok && colok && rr < a.rows && iy >= 0 && iy < a.H;
                    const unsigned vo = ok ? (plane + (unsigned)(iy * a.W + x)) * 16u : kOob;
                    regs[i] = __builtin_bit_cast(uint4v, __builtin_amdgcn_raw_buffer_load_b128(xr, vo, 0u, 0));
                }
            };
            auto write_stage = [&](int st) {
                char* const dst = c8m_lds + (unsigned)(st % a.nbuf) * buf_bytes + (unsigned)lane * 16u;
#pragma unroll
                for (int i = 0; i < MAXI; ++i) {
                    const int k = pw + i * a.nprod;
                    if (k < a.n_ins) {
                        const int b = k / q_n, q = k - b * q_n;
                        *reinterpret_cast<uint4v*>(dst + (unsigned)b * blk_bytes + (unsigned)q * 1024u) = regs[i];
                    }
                }
            };
            load_stage(0);
            write_stage(0);
            for (int s = 0; s < S; ++s) {
                if (s + 1 < S) load_stage(s + 1);
                __builtin_amdgcn_s_waitcnt(0xc07f);                  // lgkmcnt(0): this wave's LDS writes of stage s are done
                asm volatile("s_barrier" ::: "memory");              // B(s)
                if (s + 1 < S) write_stage(s + 1);
            }
            return;
        }
        while (s_i < S && s_i < a.nbuf) issue_next();
        for (int s = 0; s < S; ++s) {
            wait_vmcnt((s_i - s - 1) * mine);
            asm volatile("s_barrier" ::: "memory");
            if (s >= 1 && s_i < S) issue_next();
        }
        return;
    }

    // ---------------------------------------------------------------------- consumers
    // One channel tile and NB pixel blocks per wave -- or (C8mArgs.tpw2: PVHIP_CONV_F16_C8_TPW=2, 1x1 windows) TWO channel tiles and NB / 2
    // pixel blocks: a pixel operand read from LDS then feeds two MFMAs, for a second weight fragment per step.  MEASURED, NOT KEPT: same
    // box, alternating, whole FP16 pass: the nine sibling launches 0.67 -> 0.71 ms (3b 0.109 -> 0.120), with the 3x3 / 5x5 layers in that
    // form too 0.887 -> 0.923 / 0.190 -> 0.200 -- half the LDS reads per MFMA buy nothing: the consumers' LDS reads are not what these
    // launches wait for (lesson 54).
    if (KS == 1 && !POOL && a.tpw2 != 0) {
        constexpr int NBH = NB / 2;
        const int tile0 = 2 * (wid & 1), blk0 = (wid >> 1) * NBH;
        int nt = 0;
        if (tile0 < a.tm && (mt * a.tm + tile0) * 32 < a.Kp) nt = (tile0 + 1 < a.tm && (mt * a.tm + tile0 + 1) * 32 < a.Kp) ? 2 : 1;
        if (nt == 2)      c8m_consume<KS, NBH, POOL, 2>(a, c8m_lds, lane, tile0, blk0, mt, img, oy0, npx);
        else if (nt == 1) c8m_consume<KS, NBH, POOL, 1>(a, c8m_lds, lane, tile0, blk0, mt, img, oy0, npx);
        else for (int s = 0; s < S; ++s) asm volatile("s_barrier" ::: "memory");
        return;
    }
    if (wid < a.tm && (mt * a.tm + wid) * 32 < a.Kp) c8m_consume<KS, NB, POOL, 1>(a, c8m_lds, lane, wid, 0, mt, img, oy0, npx);
    else for (int s = 0; s < S; ++s) asm volatile("s_barrier" ::: "memory");
}

template <int KS, bool POOL>
void launch_c8m(const C8mArgs& a, int grid, int nb, size_t lds) {
    const int threads = 64 * (4 + a.nprod);
    if (nb == 2) hipLaunchKernelGGL((conv_f16_c8m_kernel<KS, 2, POOL>), dim3(grid), dim3(threads), lds, state().stream, a);
    else         hipLaunchKernelGGL((conv_f16_c8m_kernel<KS, 4, POOL>), dim3(grid), dim3(threads), lds, state().stream, a);
}

}  // namespace

extern "C" {

int pvhip_conv2d_f16_c8_multi_supported(int c, int h, int w, int kh, int kw, int pool, int n_dest) {
    if (c <= 0 || kh != kw || (kh != 1 && kh != 3 && kh != 5) || n_dest < 1 || n_dest > PVHIP_MAX_CONV_DESTS) return 0;
    if (pool && kh != 1) return 0;
    if (n_dest > 1 && kh != 1) return 0;
    C8RowTiles t;
    return c8_row_tiles(h, w, pool ? 1 : (kh - 1) / 2, 0, t) ? 1 : 0;
}

int pvhip_conv2d_f16_c8_multi(const void* xb, const float* wf, int n, int c, int h, int w, int kh, int kw, int pool,
                              const float* bias, int act, float act_lo, float act_hi, int n_dest, const pvhip_conv_dest* dests) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(n >= 0 && dests != nullptr);
    if (!pvhip_conv2d_f16_c8_multi_supported(c, h, w, kh, kw, pool, n_dest))
        return fail(PVHIP_EUNSUPPORTED, "pvhip_conv2d_f16_c8_multi: stride-1 \"same\" 1x1 (one or several members, optionally behind a 3x3 / 1 / 1 MaxPool) / 3x3 / 5x5 windows over short rows");
    C8mArgs a;
    int k_panel = 0;
    unsigned long long out_max = 0;
    for (int i = 0; i < n_dest; ++i) {
        const pvhip_conv_dest& d = dests[i];
        PVHIP_CHECK_ARG(d.y != nullptr && d.k > 0 && (d.layout == 0 || d.layout == 1));
        PVHIP_CHECK_ARG(d.channels_total == 0 || (d.channel_offset >= 0 && d.channel_offset + d.k <= d.channels_total));
        C8mSeg& sgm = a.seg[i];
        sgm.y = d.y; sgm.m_begin = k_panel; sgm.k = d.k; sgm.layout = d.layout;
        if (d.layout == 1) {
            PVHIP_CHECK_ARG(act == 0 || act == 1);                      // the zeros of the padding channels must survive the activation
            if (d.channels_total > 0) {
                PVHIP_CHECK_ARG(d.k % 8 == 0 && d.channel_offset % 8 == 0 && d.channels_total % 16 == 0);
                sgm.ctotal = d.channels_total; sgm.coff = d.channel_offset; sgm.nblk = d.k / 8;
            } else {
                sgm.ctotal = (d.k + 15) / 16 * 16; sgm.coff = 0; sgm.nblk = sgm.ctotal / 8;
            }
        } else {
            const ConvPlace place = conv_place(n, d.k, h, w, d.channels_total, d.channel_offset);
            sgm.ctotal = place.ctotal; sgm.coff = place.coff; sgm.nblk = 0;
        }
        k_panel += (d.k + 31) / 32 * 32;
        const unsigned long long oe = (unsigned long long)n * sgm.ctotal * h * w;      // (a blocked member: its whole blocks, zeros included)
        if (oe > out_max) out_max = oe;
    }
    const int cb = c8_blocks(c);
    const unsigned long long in_b = (unsigned long long)n * cb * h * w * 16ull;
    if (in_b >= (1ull << 31) || out_max >= (1ull << 31)) return fail(PVHIP_EUNSUPPORTED, "pvhip_conv2d_f16_c8_multi: input exceeds 2^31 bytes or an output 2^31 elements");
    if (n == 0) return PVHIP_OK;
    PVHIP_CHECK_ARG(xb != nullptr && wf != nullptr);
    C8RowTiles t;
    c8_row_tiles(h, w, pool ? 1 : (kh - 1) / 2, 0, t);
    a.xb = static_cast<const _Float16*>(xb); a.wf = reinterpret_cast<const _Float16*>(wf); a.bias = bias;
    a.N = n; a.CB = cb; a.H = h; a.W = w; a.Kp = k_panel;
    a.tm = frag_tm(k_panel); a.n_mtiles = frag_mtiles(k_panel);
    a.tiles_per_image = t.tiles;
    a.R = t.R; a.rows = t.rows; a.rows_pad = t.rows_pad; a.stride_sh = t.stride_sh;
    const int blk = kh == 1 ? 2 * kMSteps : 2;
    const int ncs16 = cb / 2;
    a.stages = kh == 1 ? (ncs16 + kMSteps - 1) / kMSteps : ncs16;
    a.n_ins  = blk * (t.rows_pad / (64 >> t.stride_sh));
    const size_t stage = (size_t)blk * t.rows_pad * (1 << t.stride_sh) * 16;
    int nbuf = (int)(52 * 1024 / stage);
    if (nbuf > kMMaxBuf) nbuf = kMMaxBuf;
    if (nbuf > a.stages) nbuf = a.stages;
    if (nbuf < 1) nbuf = 1;
    if (settings().f16_c8_reg != 0 && nbuf < 2) nbuf = 2;
    {
        const int knob = settings().f16_c8_prod;                                // PVHIP_CONV_F16_C8_PROD=1..4 (tuning runs); default: ~3 copy instructions per wave and stage
        int np = knob > 0 ? knob : (a.n_ins + 2) / 3;                           // (GoogLeNet at batch 256, 1x1 family: one producer 1.51 ms, by sixes 1.08, four 0.98)
        a.nprod = np < 1 ? 1 : (np > 4 ? 4 : np);
    }
    const int per_wave = (a.n_ins + a.nprod - 1) / a.nprod;
    a.reg_copy = (settings().f16_c8_reg != 0 && per_wave <= 8) ? 1 : 0;
    if ((nbuf - 1) * per_wave > 62) nbuf = 62 / per_wave + 1;
    if (stage * nbuf > 64 * 1024) return fail(PVHIP_EUNSUPPORTED, "pvhip_conv2d_f16_c8_multi: a stage of %zu bytes does not fit", stage);
    a.nbuf = nbuf;
    a.x_bytes  = (unsigned)in_b;
    a.wf_bytes = (unsigned)(frag_panel_halves(k_panel, c, kh * kw) * 2);
    a.act = act; a.lo = act_lo; a.hi = act_hi;
    a.nseg = n_dest;
    {
        const int knob = settings().f16_c8_tpw;                                 // PVHIP_CONV_F16_C8_TPW=2: two channel tiles per consumer wave for 1x1 windows (measured slower: off)
        a.tpw2 = (kh == 1 && knob == 2 && a.tm >= 2) ? 1 : 0;
    }
    a.abl = 0;
#ifdef PVHIP_DIAG
    a.abl = settings().conv_ablate;
#endif
    const long tiles = (long)n * t.tiles * a.n_mtiles;
    if (tiles > 0x3fffffffL) return fail(PVHIP_EUNSUPPORTED, "pvhip_conv2d_f16_c8_multi: too many tiles");
    a.n_tiles = (int)tiles;
    const size_t lds = stage * nbuf;
    if (pool)         launch_c8m<1, true>(a, (int)tiles, t.nb, lds);
    else if (kh == 1) launch_c8m<1, false>(a, (int)tiles, t.nb, lds);
    else if (kh == 3) launch_c8m<3, false>(a, (int)tiles, t.nb, lds);
    else              launch_c8m<5, false>(a, (int)tiles, t.nb, lds);
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
