// Convolution as an implicit GEMM on the fp32 matrix cores (v_mfma_f32_32x32x2_f32).
//
//   D[k_out][pixel] = sum_kred  Wt[kred][k_out] * Col[kred][pixel]
//
//   * MFMA A operand = weights (rows = output channels), B operand = im2col tile (cols = output
//     pixels).  The 32x32 accumulator then has the pixel on the lane (col = lane & 31), so the NCHW
//     store of one accumulator register is two 128-byte runs of consecutive pixels.
//   * The im2col matrix is never materialised: each lane owns one output pixel of the tile, keeps its
//     (n, ih0, iw0) in registers and gathers x[n, c, ih0 + r, iw0 + s] for the tile's 16 reduction
//     rows; (c, r, s) of a row is wave-uniform and comes from a small table built with the weights,
//     so it is decoded on the scalar unit.  Zero padding is a predicate, never memory.
//   * Weights are repacked once per tensor into the K-major panel [kred_pad][kout_pad] (zero padded),
//     so the A tile is a run of aligned float4 loads with no bounds checks.
//   * Both tiles lie K-major in LDS ([BK][BM] / [BK][BN]); the MFMA operand read of a wave is then two 128-byte rows per ds_read_b32
//     (lanes 0-31 -> k, lanes 32-63 -> k+1): conflict-free, no padding.  conv_igemm_dma_kernel (below; every window of fewer than 64
//     taps) fills them global -> LDS with `buffer_load ... lds`: the copies of stage t+1 are issued before the MFMAs of stage t and
//     waited for at its end; one barrier per stage.  Larger windows take the register-staged conv_igemm_kernel (pvhip_conv_igemm.h).
//   * Host side: one route (conv_route), one LDS-DMA launcher (launch_dma), one layout of the packed weights (ConvPanel).  The predecessor
//     kernels (conv_igemm_rs_kernel, conv_wave_kernel, conv_igemm_kernel<.., true>) and the tile overrides are in pvhip_diag_conv.hip,
//     which only the diagnostic build compiles; diag_conv_override is the one hook to it.
#include "pvhip_conv_igemm.h"

using namespace pvhip;

namespace {

// ---------------------------------------------------------------------------------------------------
// LDS-DMA variant of the (r,s)-major kernel: both tiles go global -> LDS with `buffer_load ... lds`, no
// staging registers and no ds_write pass.
//
// The K-major LDS images make this natural.  One wave-instruction of the im2col gather fills 64
// consecutive floats of one tile row (lane <-> pixel, per-lane source offset `voff` or the out-of-range
// sentinel -> the hardware writes 0, wave-uniform channel row in soffset, wave-uniform LDS destination in
// M0); the weight tile [16][BM] is a dense copy of BM/16 one-KiB pieces (16 bytes per lane).  A stage is
// 8 gather instructions + at most 2 weight pieces per wave; the loads of stage t+1 are issued before the
// MFMAs of stage t and waited for only at the end of it.
typedef const __attribute__((address_space(4))) int* const_int_p;

// Global -> LDS loads: lds_dma_b32 / lds_dma_b128 / lds_dma_wait_all of pvhip_common.h (asm statements on purpose, see there).
#define dma_b32 lds_dma_b32
#define dma_b128 lds_dma_b128
#define dma_wait_all lds_dma_wait_all

// kPW (pointwise: 1x1, stride 1, no padding, H*W % 4 == 0, (r,s)-major): the im2col tile is then a plain copy of 16
// channel rows x 128 consecutive pixels, moved as 8 one-KiB pieces (16 bytes per lane, two tile rows per piece) instead
// of 32 dword gathers per stage.
// kValid (c-major only): no padding and every window inside the tensor -- no window test at all, the tap's offset rides in the scalar
// offset of the load: ZERO vector instructions per gathered row instead of five (shift, and, compare, select, add), which were 45 of
// conv1's 61 issue slots per 16 MFMAs.  Padded layers reach it through pvhip_pad2d_f32 (the Convolution plugin pads once per launch).
// kF16 (FP16 IRs, (r,s)-major only): the SAME fp32 tiles in LDS, but a stage of 16 channels is ONE v_mfma_f32_32x32x16_f16 per 32-channel
// tile: a lane reads its eight reduction rows of both operands, rounds them to fp16 (to nearest even; the constants of an FP16 IR are fp16
// values already) and the matrix cores accumulate in fp32 -- 32 MFMA cycles per tile and stage instead of 512, after which the launch is
// as fast as its LDS-DMA copies (Convolution.py:57-87 computed in numpy float16 by the reference, common_def.py:13-17).
template <int BM, bool kRS, bool kPW = false, bool kValid = false, bool kF16 = false>   // kRS: (r,s)-major reduction order (C % 16 == 0); else c-major with the window-bit table
__global__ __launch_bounds__(kBlock, 2) void conv_igemm_dma_kernel(ConvArgs a) {
    static_assert(!kPW || kRS, "the pointwise copy uses the (r,s)-major panel");
    static_assert(!kValid || !kRS, "the test-free gather is the c-major one");
    constexpr int BN = 128, TM = BM / 32, KK = kBK / 2;
    constexpr int A_PIECES = kBK * BM * 4 / 1024;          // 1-KiB wave-instructions per weight tile
    constexpr int A_PER_WAVE = (A_PIECES + 3) / 4;
    constexpr int B_LOADS = kBK * BN / kBlock;             // gather instructions per wave per stage
    static_assert(BM % 32 == 0 && A_PIECES >= 1, "weight tile is whole 1-KiB pieces");

    __shared__ __attribute__((aligned(1024))) float As[2][kBK][BM];
    __shared__ __attribute__((aligned(1024))) float Bs[2][kBK][BN];

    const int nwg = gridDim.x;
    const int lid = xcd_tile(blockIdx.x, nwg);
    const int mt    = lid % a.n_mtiles;
    const int ptile = lid / a.n_mtiles;
    const int m0    = mt * BM;

    const int tid  = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wid  = __builtin_amdgcn_readfirstlane(tid / kWave);

    const int OHW = a.OH * a.OW;
    const int HW  = a.H * a.W;
    const unsigned chan_bytes = (unsigned)HW * 4u;
    const int phalf = (wid & 1) * 64;                      // this wave's 64 pixels of the tile
    const int prow0 = (wid >> 1) * B_LOADS;                // and its 8 reduction rows of every stage
    unsigned           xoff = kValid ? kOob : 0u;           // kValid: a pixel past the end reads zeros through its voffset
    unsigned long long inb  = 0;
    {
        const int gp = ptile * BN + phalf + lane;
        if (gp < a.P) {
            const int n   = gp / OHW;
            const int rem = gp - n * OHW;
            const int oy  = rem / a.OW;
            const int ox  = rem - oy * a.OW;
            const int ih0 = oy * a.sh - a.pt;
            const int iw0 = ox * a.sw - a.pl;
            xoff          = (unsigned)(n * a.C * HW + ih0 * a.W + iw0) * 4u;
            for (int r = 0; r < a.kh; ++r)
                for (int s = 0; s < a.kw; ++s)
                    if ((unsigned)(ih0 + r) < (unsigned)a.H && (unsigned)(iw0 + s) < (unsigned)a.W)
                        inb |= 1ull << (r * a.kw + s);
        }
    }
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wp), 0, a.wp_bytes, 0x00020000);
    // The gather tables were written by conv_pack_kernel in an earlier launch and are constant here: read them
    // through the constant address space so that the loads stay scalar (s_load) next to the asm statements.
    const const_int_p rstab  = (const_int_p)(unsigned long)a.ktab;
    const const_int_p tab_rs = rstab + a.kred_pad + kTabSpare;          // c-major: window-bit index of every row
    const int ncs = kRS ? a.C / kBK : 1;
    const int nrs = a.kh * a.kw;

    // weight pieces of this wave: piece q covers floats [q*256, q*256 + 256) of the [16][BM] image
    unsigned avoff[A_PER_WAVE];
#pragma unroll
    for (int q = 0; q < A_PER_WAVE; ++q) {
        const int f = (wid + 4 * q) * 256 + lane * 4;
        avoff[q]    = (unsigned)((f / BM) * a.kout_pad + m0 + (f % BM)) * 4u;
    }
    const unsigned a_stage_bytes = (unsigned)(kBK * a.kout_pad) * 4u;

    // pointwise: lane -> (row parity inside a piece, group of 4 consecutive pixels); a group never straddles two images
    unsigned pwoff = kOob;
    if (kPW) {
        const int gp = ptile * BN + (lane & 31) * 4;
        if (gp < a.P) {
            const int n = gp / HW, hw = gp - n * HW;
            pwoff = (unsigned)(n * a.C * HW + hw) * 4u + (unsigned)(lane >> 5) * chan_bytes;
        }
    }

    int      rs_l = 0, cs_l = 0, kt_l = 0;      // stage being loaded
    unsigned voff = kRS ? ((inb & 1ull) ? xoff + (unsigned)rstab[0] : kOob) : 0u;
    // c-major: the 8 table entries (byte offset c*H*W + r*W + s, window bit r*kw + s; padding rows carry bit 63,
    // never set) of this wave's rows of the stage being loaded, in scalar registers
    int tko[B_LOADS], trs[B_LOADS];
#define PV3_LOAD_ENT(kt_)                                                                                 \
    if (!kRS) {                                                                                           \
        const const_int_p tp = rstab + (kt_) * kBK + prow0;                                               \
        const const_int_p tq = tab_rs + (kt_) * kBK + prow0;                                              \
        _Pragma("unroll") for (int j = 0; j < B_LOADS; ++j) { tko[j] = tp[j]; trs[j] = tq[j]; }           \
    }
    PV3_LOAD_ENT(0);

#define PV3_ISSUE(buf_)                                                                                   \
    {                                                                                                     \
        if (kPW) {                                                                                        \
            _Pragma("unroll") for (int q = 0; q < 2; ++q)                                                 \
                dma_b128(xr, &Bs[buf_][2 * (wid + 4 * q)][0], pwoff,                                      \
                         (unsigned)(cs_l * kBK + 2 * (wid + 4 * q)) * chan_bytes);                        \
        } else if (kRS) {                                                                                 \
            const unsigned sbase = (unsigned)(cs_l * kBK + prow0) * chan_bytes;                           \
            _Pragma("unroll") for (int j = 0; j < B_LOADS; ++j)                                           \
                dma_b32(xr, &Bs[buf_][prow0 + j][phalf], voff, sbase + (unsigned)j * chan_bytes);         \
        } else {                                                                                          \
            if (kValid && kt_l + 1 < nk) {        /* every row of the stage is a tap, every tap is inside the tensor */ \
                _Pragma("unroll") for (int j = 0; j < B_LOADS; ++j)                                       \
                    dma_b32(xr, &Bs[buf_][prow0 + j][phalf], xoff, (unsigned)tko[j]);                     \
            } else {                              /* (kValid: the last stage and the spare one -- their padding rows read zeros) */ \
                _Pragma("unroll") for (int j = 0; j < B_LOADS; ++j) {                                     \
                    const bool tap = kValid ? trs[j] != 63 : (bool)((unsigned)(inb >> trs[j]) & 1u);      \
                    const unsigned off = tap ? xoff + (unsigned)tko[j] : kOob;                            \
                    dma_b32(xr, &Bs[buf_][prow0 + j][phalf], off, 0u);                                    \
                }                                                                                         \
            }                                                                                             \
        }                                                                                                 \
        _Pragma("unroll") for (int q = 0; q < A_PER_WAVE; ++q)                                            \
            if (A_PIECES % 4 == 0 || wid + 4 * q < A_PIECES)                                              \
                dma_b128(wr, &As[buf_][0][0] + (wid + 4 * q) * 256, avoff[q], (unsigned)kt_l * a_stage_bytes); \
    }
#define PV3_ADVANCE()                                                                                     \
    ++kt_l;                                                                                               \
    PV3_LOAD_ENT(kt_l);                                                                                   \
    if (kRS && ++cs_l == ncs) {                                                                           \
        cs_l = 0;                                                                                         \
        ++rs_l;                                                                                           \
        const unsigned ro = (unsigned)rstab[rs_l];  /* spare zero entries past the last tap */            \
        voff = (rs_l < nrs && ((inb >> rs_l) & 1ull)) ? xoff + ro : kOob;                                 \
    }

    floatx16 acc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    const int l31 = lane & 31, lh = lane >> 5;
    const int b_col = wid * 32 + l31;

    const int nk = kRS ? nrs * ncs : a.kred_pad / kBK;
    PV3_ISSUE(0);
    PV3_ADVANCE();
    dma_wait_all();
    __syncthreads();

    // c-major: the LAST stage is taken out of the loop.  Its rows past C*kh*kw are zero rows of the panel: only the k-steps that hold
    // a real row are multiplied (conv1 of GoogLeNet: 147 rows = 9 stages + 3 rows, 2 of the last stage's 8 k-steps -- 148 of 160
    // MFMA steps), and nothing is copied for a stage behind it.
    const int nk_loop = (kRS || kF16) ? nk : nk - 1;          // (the f16 form: a stage is ONE matrix instruction, nothing to skip)
    for (int kt = 0; kt < nk_loop; ++kt) {
        const int buf = kt & 1;
        if (kF16) {
            typedef _Float16 half8 __attribute__((ext_vector_type(8)));
            PV3_ISSUE(buf ^ 1);     // stage kt+1 (past the end: the spare zero stages)
            __builtin_amdgcn_sched_barrier(0);
            half8 b8;               // MFMA operand layout: lane (column l31, half lh) holds reduction rows 8 lh .. 8 lh + 7
#pragma unroll
            for (int q = 0; q < 8; ++q) b8[q] = (_Float16)Bs[buf][8 * lh + q][b_col];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                half8 a8;
#pragma unroll
                for (int q = 0; q < 8; ++q) a8[q] = (_Float16)As[buf][8 * lh + q][l31 + i * 32];
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a8, b8, acc[i], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            PV3_ADVANCE();
            dma_wait_all();
            __syncthreads();
            continue;
        }
        float af[2][TM], bf[2];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[0][i] = As[buf][lh][l31 + i * 32];
        bf[0] = Bs[buf][lh][b_col];
        PV3_ISSUE(buf ^ 1);     // stage kt+1 (past the end: the spare zero stages)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const int cur = kk & 1, nxt = cur ^ 1;
            if (kk + 1 < KK) {
#pragma unroll
                for (int i = 0; i < TM; ++i) af[nxt][i] = As[buf][2 * (kk + 1) + lh][l31 + i * 32];
                bf[nxt] = Bs[buf][2 * (kk + 1) + lh][b_col];
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][i], bf[cur], acc[i], 0, 0, 0);
            if (kk + 1 < KK) __builtin_amdgcn_sched_group_barrier(0x100, TM + 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, TM, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        PV3_ADVANCE();
        dma_wait_all();
        __syncthreads();
    }
    if (!kRS && !kF16) {
        const int buf   = (nk - 1) & 1;
        const int steps = min(KK, (a.C * nrs - (nk - 1) * kBK + 1) >> 1);     // k-steps of the last stage with a real reduction row
        for (int kk = 0; kk < steps; ++kk) {
            float afl[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) afl[i] = As[buf][2 * kk + lh][l31 + i * 32];
            const float bfl = Bs[buf][2 * kk + lh][b_col];
#pragma unroll
            for (int i = 0; i < TM; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(afl[i], bfl, acc[i], 0, 0, 0);
        }
    }
#undef PV3_ISSUE
#undef PV3_LOAD_ENT
#undef PV3_ADVANCE

    // The destination table is read from the argument block HERE, through a pointer the compiler cannot see through:
    // as ordinary arguments its 30 dwords would be loaded at kernel entry and held in scalar registers across the
    // reduction loop, which has none to spare (the LDS-DMA statements need their operands in SGPRs).
    typedef const __attribute__((address_space(4))) ConvArgs* kernarg_p;
    kernarg_p ka = (kernarg_p)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    const int nseg_l = ka->nseg;
    const __amdgpu_buffer_rsrc_t br = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bias), 0,
                                                                        a.bias != nullptr ? a.K * 4 : 0, 0x00020000);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int row0 = m0 + i * 32 + 4 * lh;
        float     bv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r)
            bv[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                br, (unsigned)(row0 + (r & 3) + 8 * (r >> 2)) * 4u, 0, 0));
        const int gp = ptile * BN + wid * 32 + l31;
        if (gp >= a.P) continue;
        const int n   = gp / OHW;
        const int rem = gp - n * OHW;
        float* __restrict__ yb = a.y;
        int yct = a.y_ctotal, ycoff = a.y_coff, klim = a.K;
        int c8_blocks = 0, c8_first = 0;    // a range stored as blocked fp16: its channel blocks, and the first block of this workgroup's tile
        if (nseg_l > 0) {                   // the destination range this 32-channel tile belongs to (workgroup-uniform)
            int sg = 0;
            for (int q = 1; q < nseg_l; ++q) sg = (m0 + i * 32 >= ka->seg[q].m_begin) ? q : sg;
            yb    = ka->seg[sg].y;
            yct   = ka->seg[sg].ctotal;
            ycoff = ka->seg[sg].coff - ka->seg[sg].m_begin;
            klim  = ka->seg[sg].m_begin + ka->seg[sg].k;
            if (kF16 && ka->seg[sg].layout == 1) {
                c8_blocks = (ka->seg[sg].k + 15) / 16 * 2;
                c8_first  = (m0 - ka->seg[sg].m_begin) / 8;      // ranges begin at whole 32-channel tiles
            }
        }
        float* __restrict__ yp = yb + ((size_t)n * yct + ycoff + row0) * OHW + rem;
        float vv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) vv[r] = acc[i][r];
        bias_act_n<16>(vv, bv, a.bias != nullptr, a.relu, act_bounds(a.relu, a.act_lo, a.act_hi));
        if (kF16 && c8_blocks > 0) {
            // the reader is pvhip_conv2d_f16_c8: fp16 (round to nearest even: the value the reader would round this output to anyway),
            // the eight channels of a pixel in one 16-byte piece.  Registers 4 g .. 4 g + 3 are channels 8 g + 4 lh .. + 3 of the tile:
            // half a piece per lane, the two lane halves of a wave fill it.  Channels past the range's count up to a whole 16-channel
            // stage are written too: zero rows of the panel, zero bias -- zeros, which is what the reader's zero weights expect.
            typedef _Float16 half4v __attribute__((ext_vector_type(4)));
            _Float16* const yh = reinterpret_cast<_Float16*>(yb);
            const int blk0 = c8_first + i * 4;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (blk0 + g >= c8_blocks) continue;
                half4v h;
#pragma unroll
                for (int j = 0; j < 4; ++j) h[j] = (_Float16)vv[4 * g + j];
                *reinterpret_cast<half4v*>(yh + (((size_t)n * c8_blocks + blk0 + g) * OHW + rem) * 8 + 4 * lh) = h;
            }
            continue;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int dr = (r & 3) + 8 * (r >> 2);
            if (row0 + dr < klim) conv_store1(yp + (size_t)dr * OHW, vv[r]);
        }
    }
}

__global__ __launch_bounds__(kBlock) void conv_pack_kernel(const float* __restrict__ w, int* __restrict__ ktab,
                                                            float* __restrict__ wp, int K, int C, int kh, int kw, int H,
                                                            int W, int kred, int kred_pad, int kout_pad, int rsmajor) {
    const size_t total  = (size_t)(kred_pad + kPanelSpare) * kout_pad;   // includes the spare zero stages
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const bool   mask   = kh * kw < 64;
    const int    tab_n  = kred_pad + kTabSpare;                  // spare stages of padding rows
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int kr = (int)(e / kout_pad);   // panel row
        const int ko = (int)(e % kout_pad);
        float     v  = 0.0f;
        if (kr < kred && ko < K) {
            // source reduction index in OIHW order is (c*kh + r)*kw + s
            int src = kr;
            if (rsmajor) {                    // panel row = (r*kw + s)*C + c
                const int rs = kr / C, c = kr - rs * C;
                src          = c * (kh * kw) + rs;
            }
            v = w[(size_t)ko * kred + src];
        }
        wp[e] = v;
    }
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)(2 * tab_n); e += stride) {
        const int i = (int)e;
        int       v = 0;
        if (rsmajor) {
            // table[rs] = byte offset of tap (r, s) inside one channel plane; zeros after the last tap
            if (i < kh * kw) v = ((i / kw) * W + (i % kw)) * 4;
        } else if (i < tab_n) {
            if (i < kred) {
                const int s = i % kw, t = i / kw, r = t % kh, c = t / kh;
                v = (c * H * W + r * W + s) * 4;
            }
        } else {
            const int kr = i - tab_n;
            v            = mask ? 63 : (0x7fff << 8);
            if (kr < kred) {
                const int s = kr % kw, r = (kr / kw) % kh;
                v           = mask ? (r * kw + s) : ((r << 8) | s);
            }
        }
        ktab[i] = v;
    }
}

// ---- host side

// Which kernel a single fp32 launch takes (PVHIP_CONV_KIND_*).  The eligibility chain is spelled here and nowhere else: conv2d_impl
// switches on the answer, pvhip_conv2d_kernel_kind reports it (behind its test for the stem kernels, which are entries of their own).
int conv_route(int n, int c, int h, int w, int kh, int kw, int oh, int ow, int sh, int sw, int pad_top, int pad_left) {
    if (pw_eligible(c, kh, kw, sh, sw, pad_top, pad_left, h, w, oh, ow)) return PVHIP_CONV_KIND_POINTWISE;
    if (wino25_eligible(c, kh, kw, sh, sw, pad_top, pad_left, h, w, oh, ow, n)) return PVHIP_CONV_KIND_WINO_F2_5X5;
    if (wino4_eligible(c, kh, kw, sh, sw, pad_top, pad_left, h, w, oh, ow, n)) return PVHIP_CONV_KIND_WINO_F4_3X3;
    if (wino_eligible(c, kh, kw, sh, sw, pad_top, pad_left, h, w, oh, ow)) return PVHIP_CONV_KIND_WINO_F2_3X3;
    return PVHIP_CONV_KIND_IGEMM;      // windows of 64 taps and more included
}

// Operands, geometry and epilogue of one launch.  The caller adds the destination table (nseg, seg) and the tile counts.
void conv_args(ConvArgs& a, const ConvPanel& p, const float* x, const float* wpack, const float* bias, float* y, int y_ctotal, int y_coff,
               int n, int c, int h, int w, int k, int kh, int kw, int oh, int ow, int sh, int sw, int pad_top, int pad_left, int act,
               float act_lo, float act_hi) {
    a.x = x; a.y = y; a.bias = bias;
    a.ktab = reinterpret_cast<const int*>(wpack);
    a.wp   = p.wp(wpack);
    a.N = n; a.C = c; a.H = h; a.W = w; a.K = k; a.OH = oh; a.OW = ow;
    a.sh = sh; a.sw = sw; a.pt = pad_top; a.pl = pad_left; a.kh = kh; a.kw = kw;
    a.x_bytes  = (unsigned)((unsigned long long)n * c * h * w * 4ull);
    a.wp_bytes = (unsigned)(p.panel * sizeof(float));
    a.kred_pad = p.kred_pad; a.kout_pad = p.kout_pad;
    a.P = n * oh * ow;
    a.relu = act; a.act_lo = act_lo; a.act_hi = act_hi;
    a.y_ctotal = y_ctotal; a.y_coff = y_coff;
}

// What a launch of the implicit-GEMM kernels takes, decided HERE and nowhere else: the launchers below switch on the plan,
// pvhip_conv2d_form reports it.  kernel: PVHIP_IGEMM_* (include/pvhip.h).
struct IgemmPlan {
    int bm, kernel, n_mtiles, n_ptiles;
};

// The forms of conv_igemm_dma_kernel.  Pointwise (1x1, stride 1, unpadded, whole pixel quads; PVHIP_CONV_NOPW: tuning): the tile is a plain copy
inline bool dma_pointwise(int c, int h, int w, int kh, int kw, int oh, int ow, int sh, int sw, int pt, int pl) {
    return rs_major(c, kh, kw) && kh == 1 && kw == 1 && sh == 1 && sw == 1 && pt == 0 && pl == 0 && oh == h &&
           ow == w && (h * w) % 4 == 0 && !settings().conv_nopw;
}
// c-major without a window test: no padding and no window leaves the tensor (PVHIP_CONV_NOVALID: A/B)
inline bool dma_valid(int h, int w, int kh, int kw, int oh, int ow, int sh, int sw, int pt, int pl) {
    return pt == 0 && pl == 0 && (oh - 1) * sh + kh <= h && (ow - 1) * sw + kw <= w && !settings().conv_novalid;
}

// A launch on bm x 128 tiles: conv_igemm_dma_kernel in the form that follows from the geometry (every window of fewer than 64 taps), else
// the register-staged conv_igemm_kernel with a compare per gathered element instead of the window-bit mask.
IgemmPlan plan_tiles(int bm, int p_pixels, int c, int h, int w, int k, int kh, int kw, int oh, int ow, int sh, int sw, int pt, int pl) {
    IgemmPlan p;
    p.bm       = bm;
    p.n_mtiles = (k + bm - 1) / bm;
    p.n_ptiles = (p_pixels + 127) / 128;
    if (!(dma_enabled() && dma_takes(kh, kw))) p.kernel = PVHIP_IGEMM_REGISTER;
    else if (dma_pointwise(c, h, w, kh, kw, oh, ow, sh, sw, pt, pl)) p.kernel = PVHIP_IGEMM_POINTWISE_COPY;
    else if (rs_major(c, kh, kw)) p.kernel = PVHIP_IGEMM_RS_MAJOR;
    else if (dma_valid(h, w, kh, kw, oh, ow, sh, sw, pt, pl)) p.kernel = PVHIP_IGEMM_C_MAJOR_VALID;
    else p.kernel = PVHIP_IGEMM_C_MAJOR_WINDOW;
    return p;
}
inline IgemmPlan plan_tiles(int bm, const ConvArgs& a) {
    return plan_tiles(bm, a.P, a.C, a.H, a.W, a.K, a.kh, a.kw, a.OH, a.OW, a.sh, a.sw, a.pt, a.pl);
}

// PVHIP_CONV_KIND_IGEMM, fp32.  Tiles (calibrated with scripts/tune_conv.py on the GoogLeNet shapes at batch 256): 128 pixels; 64 output
// channels when that wastes less than half a tile and still leaves >= 4 workgroups per CU, else 32.
int igemm_bm(int p_pixels, int k, int kh, int kw) {
    int bm = (k % 64 == 0 || k % 64 > 32) ? 64 : 32;
    if (bm == 64 && (long)((p_pixels + 127) / 128) * ((k + 63) / 64) < 4 * kNumCU) bm = 32;
    if (kh == 1 && kw == 1) bm = 32;      // 1x1 layers: the smaller tile wins on every GoogLeNet shape (more workgroups per CU)
    return bm;
}

// The f16 form (pvhip_conv2d_f16_dma, pvhip_conv2d_multi_f16_dma): the activation tile of a stage is re-read once per channel tile (through
// L2, which is what this form is bound by): wide tiles.  PVHIP_CONV_F16_BM: tuning runs
int f16_bm(int k) { return settings().f16_bm ? settings().f16_bm : (k > 64 ? 128 : (k > 32 ? 64 : 32)); }

// Every launch of conv_igemm_dma_kernel: BM x 128 tiles, p.n_mtiles x p.n_ptiles workgroups, the form the plan names.
// (PVHIP_CONV_LDS_PAD_KB: tuning, extra dynamic LDS caps the workgroups per CU.)
template <int BM, bool kF16>
int launch_dma(const IgemmPlan& p, const ConvArgs& a) {
    const dim3   grid(p.n_mtiles * p.n_ptiles), block(kBlock);
    const size_t dyn = (size_t)settings().conv_lds_pad_kb * 1024;
    switch (p.kernel) {
    case PVHIP_IGEMM_POINTWISE_COPY:
        hipLaunchKernelGGL((conv_igemm_dma_kernel<BM, true, true, false, kF16>), grid, block, dyn, state().stream, a);
        return PVHIP_OK;
    case PVHIP_IGEMM_RS_MAJOR:
        hipLaunchKernelGGL((conv_igemm_dma_kernel<BM, true, false, false, kF16>), grid, block, dyn, state().stream, a);
        return PVHIP_OK;
    default: break;
    }
    if constexpr (BM == 128 && !kF16 && !kDiagBuild)      // no fp32 route picks the widest tile for a c-major layer (PVHIP_CONV_TILE does)
        return fail(PVHIP_EUNSUPPORTED, "conv_igemm_dma_kernel: no 128-channel tile for C=%d (not a multiple of %d)", a.C, kBK);
    else if (p.kernel == PVHIP_IGEMM_C_MAJOR_VALID)
        hipLaunchKernelGGL((conv_igemm_dma_kernel<BM, false, false, true, kF16>), grid, block, dyn, state().stream, a);
    else
        hipLaunchKernelGGL((conv_igemm_dma_kernel<BM, false, false, false, kF16>), grid, block, dyn, state().stream, a);
    return PVHIP_OK;
}

// A launch by its plan: the LDS-DMA kernel, or (fp32, windows of 64 taps and more) the register-staged one.
template <bool kF16>
int launch_plan(const IgemmPlan& p, ConvArgs& a) {
    a.n_mtiles = p.n_mtiles;
    if (p.kernel != PVHIP_IGEMM_REGISTER)
        return p.bm == 128 ? launch_dma<128, kF16>(p, a) : p.bm == 64 ? launch_dma<64, kF16>(p, a) : launch_dma<32, kF16>(p, a);
    const dim3 grid(p.n_mtiles * p.n_ptiles), block(kBlock);
    if (p.bm == 64) hipLaunchKernelGGL((conv_igemm_kernel<64, 128, 1, 4, false>), grid, block, 0, state().stream, a);
    else hipLaunchKernelGGL((conv_igemm_kernel<32, 128, 1, 4, false>), grid, block, 0, state().stream, a);
    return PVHIP_OK;
}

int launch_igemm(ConvArgs& a) {
    int bm = igemm_bm(a.P, a.K, a.kh, a.kw);
#ifdef PVHIP_DIAG
    int bn = 128;
    if (int rc; diag_conv_override(a, &bm, &bn, &rc)) return rc;      // pvhip_diag_conv.hip
#endif
    return launch_plan<false>(plan_tiles(bm, a), a);
}

}  // namespace

extern "C" {

size_t pvhip_conv2d_pack_elems(int k_out, int c, int kh, int kw) {
    if (k_out <= 0 || c <= 0 || kh <= 0 || kw <= 0) return 0;
    return ConvPanel(k_out, c, kh, kw).elems();
}

int pvhip_conv2d_pack_f32(const float* w_oihw, float* wpack, int k_out, int c, int kh, int kw, int h, int w) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(w_oihw != nullptr && wpack != nullptr);
    PVHIP_CHECK_ARG(k_out > 0 && c > 0 && kh > 0 && kw > 0 && h > 0 && w > 0);
    if (kh >= 256 || kw >= 256 || (unsigned long long)c * h * w >= (1ull << 29))
        return fail(PVHIP_EUNSUPPORTED, "pvhip_conv2d_pack_f32: C=%d kh=%d kw=%d H=%d W=%d outside table encoding", c, kh, kw, h, w);
    const ConvPanel p(k_out, c, kh, kw);
    hipLaunchKernelGGL(conv_pack_kernel, dim3(grid_for(p.panel)), dim3(kBlock), 0, state().stream, w_oihw, reinterpret_cast<int*>(wpack),
                       p.wp(wpack), k_out, c, kh, kw, h, w, c * kh * kw, p.kred_pad, p.kout_pad, rs_major(c, kh, kw) ? 1 : 0);
    // the panels that ride along are packed whether a launch will use them or not: that depends on stride, padding, extents and batch
    int rc = PVHIP_OK;
    if (p.pw > 0) rc = pw_pack(w_oihw, p.riders(wpack), k_out, c);
    else if (p.wino25 > 0) rc = wino25_pack(w_oihw, p.riders(wpack), k_out, c);
    else if (p.wino2 > 0) {
        rc = wino_pack(w_oihw, p.riders(wpack), k_out, c);
        if (rc == PVHIP_OK) rc = wino4_pack(w_oihw, p.wino4_panel(wpack), k_out, c);
    }
    if (rc) return rc;
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

static int conv2d_impl(const float* x, const float* wpack, float* y, int n, int c, int h, int w, int k_out, int kh,
                       int kw, int oh, int ow, int sh, int sw, int pad_top, int pad_left, const float* bias, int relu,
                       int out_channel_offset, int out_channels_total, float act_lo, float act_hi, bool f16 = false, bool c8_out = false) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(n >= 0 && c > 0 && h > 0 && w > 0 && k_out > 0 && kh > 0 && kw > 0 && oh >= 0 && ow >= 0);
    PVHIP_CHECK_ARG(sh > 0 && sw > 0 && pad_top >= 0 && pad_left >= 0);
    if (kh >= 256 || kw >= 256)
        return fail(PVHIP_EUNSUPPORTED, "pvhip_conv2d_f32: kh=%d kw=%d outside table encoding", kh, kw);
    PVHIP_CHECK_ARG(out_channels_total == 0 || (out_channel_offset >= 0 && out_channel_offset + k_out <= out_channels_total));
    const int y_ctotal = out_channels_total > 0 ? out_channels_total : k_out;
    const int y_coff   = out_channels_total > 0 ? out_channel_offset : 0;
    const unsigned long long in_e = (unsigned long long)n * c * h * w, out_e = (unsigned long long)n * y_ctotal * oh * ow;
    if (in_e >= (1ull << 29) || out_e >= (1ull << 31))
        return fail(PVHIP_EUNSUPPORTED, "pvhip_conv2d_f32: input exceeds 2^29 elements (buffer offsets below 2^31) or output 2^31");
    if (out_e == 0) return PVHIP_OK;
    PVHIP_CHECK_ARG(x != nullptr && wpack != nullptr && y != nullptr);

    const ConvPanel p(k_out, c, kh, kw);
    ConvArgs a;
    conv_args(a, p, x, wpack, bias, y, y_ctotal, y_coff, n, c, h, w, k_out, kh, kw, oh, ow, sh, sw, pad_top, pad_left, relu, act_lo, act_hi);
    a.nseg = 0;
    if (c8_out) {        // pvhip_conv2d_f16_dma_c8: the output as fp16 blocked by eight channels (one range: the whole panel)
        PVHIP_CHECK_ARG(f16 && out_channels_total == 0 && (relu == 0 || relu == 1));
        a.nseg = 1;
        a.seg[0].y = y; a.seg[0].m_begin = 0; a.seg[0].k = k_out; a.seg[0].ctotal = k_out; a.seg[0].coff = 0; a.seg[0].layout = 1;
    }
    int rc;
    if (f16) {      // pvhip_conv2d_f16_dma: every layer on the LDS-DMA kernel's f16 form (the matrix work is 16x cheaper: no Winograd, wide tiles)
        if (!dma_takes(kh, kw) || !dma_enabled())
            return fail(PVHIP_EUNSUPPORTED, "pvhip_conv2d_f16_dma: C %% 16 == 0 or a window of fewer than 64 taps required (C=%d, %dx%d)", c, kh, kw);
        rc = launch_plan<true>(plan_tiles(f16_bm(k_out), a), a);
    } else {
        switch (conv_route(n, c, h, w, kh, kw, oh, ow, sh, sw, pad_top, pad_left)) {
        case PVHIP_CONV_KIND_POINTWISE: {      // pvhip_pw.hip
            const PwDest d{y, 0, k_out, y_ctotal, y_coff};
            rc = pw_conv(x, p.riders(wpack), n, c, h * w, k_out, bias, relu, act_lo, act_hi, 1, &d);
            break;
        }
        // pvhip_wino.hip: 5x5 / stride 1 / pad 2; 3x3 / stride 1 / same padding as F(4x4, 3x3) (extents and batch large enough) or F(2x2, 3x3)
        case PVHIP_CONV_KIND_WINO_F2_5X5: rc = wino4_conv(2, x, p.riders(wpack), y, n, c, h, w, k_out, bias, relu, act_lo, act_hi, y_coff, y_ctotal); break;
        case PVHIP_CONV_KIND_WINO_F4_3X3: rc = wino4_conv(4, x, p.wino4_panel(wpack), y, n, c, h, w, k_out, bias, relu, act_lo, act_hi, y_coff, y_ctotal); break;
        case PVHIP_CONV_KIND_WINO_F2_3X3: rc = wino_conv(x, p.riders(wpack), y, n, c, h, w, k_out, bias, relu, act_lo, act_hi, y_coff, y_ctotal); break;
        default: rc = launch_igemm(a);
        }
    }
    if (rc) return rc;
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

int pvhip_conv2d_f32(const float* x, const float* wpack, float* y, int n, int c, int h, int w, int k_out, int kh, int kw,
                     int oh, int ow, int sh, int sw, int pad_top, int pad_left, const float* bias, int relu,
                     int out_channel_offset, int out_channels_total, float act_lo, float act_hi) {
    return conv2d_impl(x, wpack, y, n, c, h, w, k_out, kh, kw, oh, ow, sh, sw, pad_top, pad_left, bias, relu, out_channel_offset,
                       out_channels_total, act_lo, act_hi);
}

int pvhip_conv2d_f16_dma_supported(int c, int kh, int kw) { return (c > 0 && kh > 0 && kw > 0 && dma_takes(kh, kw) && dma_enabled()) ? 1 : 0; }

int pvhip_conv2d_f16_dma(const float* x, const float* wpack, float* y, int n, int c, int h, int w, int k_out, int kh, int kw,
                         int oh, int ow, int sh, int sw, int pad_top, int pad_left, const float* bias, int relu,
                         int out_channel_offset, int out_channels_total, float act_lo, float act_hi) {
    return conv2d_impl(x, wpack, y, n, c, h, w, k_out, kh, kw, oh, ow, sh, sw, pad_top, pad_left, bias, relu, out_channel_offset,
                       out_channels_total, act_lo, act_hi, true);
}

int pvhip_conv2d_f16_dma_c8(const float* x, const float* wpack, void* yb, int n, int c, int h, int w, int k_out, int kh, int kw,
                            int oh, int ow, int sh, int sw, int pad_top, int pad_left, const float* bias, int act) {
    return conv2d_impl(x, wpack, static_cast<float*>(yb), n, c, h, w, k_out, kh, kw, oh, ow, sh, sw, pad_top, pad_left, bias, act, 0, 0, 0.0f, 0.0f,
                       true, true);
}

int pvhip_conv2d_kernel_kind(int n, int c, int h, int w, int k_out, int kh, int kw, int oh, int ow, int sh, int sw, int pad_top, int pad_left) {
    // (the row-span kernel is an entry of its own, pvhip_conv2d_stem_f32: the caller pads the image to the row length it asks for)
    if (settings().conv_stem && pvhip_conv2d_stem_f32_supported(c, h, w, k_out, kh, kw, sh, sw, pad_top, pad_left, oh, ow) > 0 &&
        (unsigned long long)n * k_out * oh * ow * 4ull < (1ull << 31) && (unsigned long long)n * c * (h + 6) * 256ull * 4ull < (1ull << 31))
        return (settings().conv_stem_wino && pvhip_conv2d_stem_wino_supported(c, h, w, k_out, kh, kw, sh, sw, pad_top, pad_left, oh, ow) > 0)
                   ? PVHIP_CONV_KIND_STEM_WINO : PVHIP_CONV_KIND_STEM;
    return conv_route(n, c, h, w, kh, kw, oh, ow, sh, sw, pad_top, pad_left);
}

int pvhip_conv2d_form(int entry, int n, int c, int h, int w, int k_out, int kh, int kw, int oh, int ow, int sh, int sw, int pad_top,
                      int pad_left, int* form) {
    PVHIP_CHECK_ARG(form != nullptr);
    for (int i = 0; i < PVHIP_FORM_INTS; ++i) form[i] = 0;
    form[PVHIP_CONV_FORM_KIND] = PVHIP_FORM_NONE;
    PVHIP_CHECK_ARG(entry == PVHIP_CONV_ENTRY_F32 || entry == PVHIP_CONV_ENTRY_F16_DMA);
    PVHIP_CHECK_ARG(n >= 0 && c > 0 && h > 0 && w > 0 && k_out > 0 && kh > 0 && kw > 0 && oh >= 0 && ow >= 0);
    PVHIP_CHECK_ARG(sh > 0 && sw > 0 && pad_top >= 0 && pad_left >= 0);
    if (kh >= 256 || kw >= 256)
        return fail(PVHIP_EUNSUPPORTED, "pvhip_conv2d_form: kh=%d kw=%d outside table encoding", kh, kw);
    const unsigned long long in_e = (unsigned long long)n * c * h * w, out_e = (unsigned long long)n * k_out * oh * ow;
    if (in_e >= (1ull << 29) || out_e >= (1ull << 31))
        return fail(PVHIP_EUNSUPPORTED, "pvhip_conv2d_form: input exceeds 2^29 elements (buffer offsets below 2^31) or output 2^31");
    if (out_e == 0) return PVHIP_OK;                                 // nothing is launched
    const int pixels = n * oh * ow;
    int kind = PVHIP_CONV_KIND_IGEMM;
    if (entry == PVHIP_CONV_ENTRY_F16_DMA) {
        if (!dma_takes(kh, kw) || !dma_enabled())
            return fail(PVHIP_EUNSUPPORTED, "pvhip_conv2d_form: the f16 LDS-DMA entry takes windows of fewer than 64 taps (%dx%d)", kh, kw);
    } else {
        kind = conv_route(n, c, h, w, kh, kw, oh, ow, sh, sw, pad_top, pad_left);
    }
    switch (kind) {
    case PVHIP_CONV_KIND_POINTWISE: {
        const PwPlan p = plan_pw(n, c, h * w, k_out);
        form[PVHIP_CONV_FORM_GRID]       = p.grid;
        form[PVHIP_CONV_FORM_PW_TN]      = p.tn;
        form[PVHIP_CONV_FORM_PW_VEC]     = p.vec ? 1 : 0;
        form[PVHIP_CONV_FORM_PW_NCHUNK]  = p.nchunk;
        form[PVHIP_CONV_FORM_PW_STAGGER] = p.stagger != 0 ? 1 : 0;
        break;
    }
    case PVHIP_CONV_KIND_WINO_F2_3X3: {
        const WinoPlan p = plan_wino(n, h, w, k_out);
        if (p.grid > 0x7fffffffL) return fail(PVHIP_EUNSUPPORTED, "pvhip_conv2d_form: grid too large");
        form[PVHIP_CONV_FORM_GRID]         = (int)p.grid;
        form[PVHIP_CONV_FORM_WINO_KB]      = p.kb;
        form[PVHIP_CONV_FORM_WINO_PATCHES] = p.nt;
        form[PVHIP_CONV_FORM_WINO_WAVES]   = p.waves;
        break;
    }
    case PVHIP_CONV_KIND_WINO_F4_3X3:
    case PVHIP_CONV_KIND_WINO_F2_5X5: {
        const Wino4Plan p = plan_wino4(kind == PVHIP_CONV_KIND_WINO_F4_3X3 ? 4 : 2, n, c, h, w, k_out);
        if (p.tiles_max > 0x3fffffffL) return fail(PVHIP_EUNSUPPORTED, "pvhip_conv2d_form: too many tiles");
        form[PVHIP_CONV_FORM_GRID]         = p.grid;
        form[PVHIP_CONV_FORM_WINO4_M]      = p.m;
        form[PVHIP_CONV_FORM_WINO4_RAGGED] = p.ragged ? 1 : 0;
        form[PVHIP_CONV_FORM_WINO4_SHARED] = p.shared ? 1 : 0;
        form[PVHIP_CONV_FORM_WINO4_ORDER]  = p.s_order;
        form[PVHIP_CONV_FORM_WINO4_TILES]  = p.n_tiles;
        form[PVHIP_CONV_FORM_WINO4_WALK]   = p.walk ? 1 : 0;
        break;
    }
    default: {
        const int bm = entry == PVHIP_CONV_ENTRY_F16_DMA ? f16_bm(k_out) : igemm_bm(pixels, k_out, kh, kw);
        const IgemmPlan p = plan_tiles(bm, pixels, c, h, w, k_out, kh, kw, oh, ow, sh, sw, pad_top, pad_left);
        form[PVHIP_CONV_FORM_GRID]           = p.n_mtiles * p.n_ptiles;
        form[PVHIP_CONV_FORM_IGEMM_BM]       = p.bm;
        form[PVHIP_CONV_FORM_IGEMM_KERNEL]   = p.kernel;
        form[PVHIP_CONV_FORM_IGEMM_N_MTILES] = p.n_mtiles;
    }
    }
    form[PVHIP_CONV_FORM_KIND] = kind;
    return PVHIP_OK;
}

int pvhip_conv2d_multi_supported(int c, int kh, int kw, int sh, int sw, int pad_top, int pad_left, int n_dest) {
    return (n_dest >= 1 && n_dest <= kMaxConvDests && kh == 1 && kw == 1 && sh == 1 && sw == 1 && pad_top == 0 && pad_left == 0 &&
            rs_major(c, kh, kw)) ? 1 : 0;
}

static int conv2d_multi_impl(const float* x, const float* wpack, int n, int c, int h, int w, int kh, int kw, int oh, int ow, int sh,
                             int sw, int pad_top, int pad_left, const float* bias, int act, float act_lo, float act_hi, int n_dest,
                             const pvhip_conv_dest* dests, bool f16) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(n >= 0 && c > 0 && h > 0 && w > 0 && oh >= 0 && ow >= 0 && dests != nullptr);
    if (!pvhip_conv2d_multi_supported(c, kh, kw, sh, sw, pad_top, pad_left, n_dest) || oh != h || ow != w)
        return fail(PVHIP_EUNSUPPORTED, "pvhip_conv2d_multi_f32: only 1x1 / stride 1 / unpadded convolutions with C %% 16 == 0 and at most %d destinations",
                    kMaxConvDests);
    ConvArgs a;
    int k_panel = 0;
    unsigned long long out_max = 0;
    for (int i = 0; i < n_dest; ++i) {
        const pvhip_conv_dest& d = dests[i];
        PVHIP_CHECK_ARG(d.y != nullptr && d.k > 0);
        PVHIP_CHECK_ARG(d.channels_total == 0 || (d.channel_offset >= 0 && d.channel_offset + d.k <= d.channels_total));
        a.seg[i].y       = d.y;
        a.seg[i].m_begin = k_panel;
        a.seg[i].k       = d.k;
        a.seg[i].ctotal  = d.channels_total > 0 ? d.channels_total : d.k;
        a.seg[i].coff    = d.channels_total > 0 ? d.channel_offset : 0;
        a.seg[i].layout  = d.layout;
        if (d.layout != 0) {            // fp16, channels blocked by eight: the f16 form only, a tensor of its own, zeros survive the activation
            PVHIP_CHECK_ARG(d.layout == 1 && f16 && d.channels_total == 0 && (act == 0 || act == 1));
        }
        k_panel += round_up_int(d.k, 32);
        const unsigned long long oe = (unsigned long long)n * a.seg[i].ctotal * oh * ow;
        if (oe > out_max) out_max = oe;
    }
    const unsigned long long in_e = (unsigned long long)n * c * h * w;
    if (in_e >= (1ull << 29) || out_max >= (1ull << 31))
        return fail(PVHIP_EUNSUPPORTED, "pvhip_conv2d_multi_f32: input exceeds 2^29 elements or an output 2^31");
    if (in_e == 0 || oh == 0 || ow == 0) return PVHIP_OK;
    PVHIP_CHECK_ARG(x != nullptr && wpack != nullptr);
    const ConvPanel p(k_panel, c, kh, kw);      // the panel holds the destinations' channels one after the other, each range padded to whole 32-channel tiles
    int rc;
    if (!f16 && conv_route(n, c, h, w, kh, kw, oh, ow, sh, sw, pad_top, pad_left) == PVHIP_CONV_KIND_POINTWISE) {
        PwDest pd[kMaxConvDests];
        for (int i = 0; i < n_dest; ++i) pd[i] = PwDest{a.seg[i].y, a.seg[i].m_begin, a.seg[i].k, a.seg[i].ctotal, a.seg[i].coff};
        rc = pw_conv(x, p.riders(wpack), n, c, h * w, k_panel, bias, act, act_lo, act_hi, n_dest, pd);
    } else {        // the LDS-DMA kernel: fp32 with PVHIP_CONV_POINTWISE=0, and the f16 form for the sibling 1x1 convolutions of an FP16 IR
        conv_args(a, p, x, wpack, bias, dests[0].y, a.seg[0].ctotal, a.seg[0].coff, n, c, h, w, k_panel, kh, kw, oh, ow, sh, sw, pad_top, pad_left,
                  act, act_lo, act_hi);
        a.nseg = n_dest;
        // a 64-channel tile may straddle two ranges: the epilogue looks the range up per 32 channels.  f16: wide tiles, the input tile is re-read per channel tile
        if (f16) rc = launch_plan<true>(plan_tiles(f16_bm(k_panel), a), a);
        else     rc = launch_plan<false>(plan_tiles(settings().multi_bm, a), a);          // PVHIP_CONV_MULTI_BM: tuning runs only
    }
    if (rc) return rc;
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

int pvhip_conv2d_multi_f32(const float* x, const float* wpack, int n, int c, int h, int w, int kh, int kw, int oh, int ow, int sh,
                           int sw, int pad_top, int pad_left, const float* bias, int act, float act_lo, float act_hi, int n_dest,
                           const pvhip_conv_dest* dests) {
    return conv2d_multi_impl(x, wpack, n, c, h, w, kh, kw, oh, ow, sh, sw, pad_top, pad_left, bias, act, act_lo, act_hi, n_dest, dests, false);
}

int pvhip_conv2d_multi_f16_dma(const float* x, const float* wpack, int n, int c, int h, int w, int kh, int kw, int oh, int ow, int sh,
                               int sw, int pad_top, int pad_left, const float* bias, int act, float act_lo, float act_hi, int n_dest,
                               const pvhip_conv_dest* dests) {
    return conv2d_multi_impl(x, wpack, n, c, h, w, kh, kw, oh, ow, sh, sw, pad_top, pad_left, bias, act, act_lo, act_hi, n_dest, dests, true);
}

}  // extern "C"
