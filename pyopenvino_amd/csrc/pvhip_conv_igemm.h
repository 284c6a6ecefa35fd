// Internal header of the implicit-GEMM convolution: what pvhip_conv.hip shares with pvhip_diag_conv.hip (predecessor kernels, diagnostic build
// only): the kernel arguments, the layout of the packed weights, and conv_igemm_kernel, the register-staged fallback for windows of 64 taps and more.
#pragma once
#include <climits>

#include "pvhip_common.h"
#include "pvhip_wino.h"

namespace pvhip {

constexpr int kBK       = 16;   // reduction rows per stage
constexpr int kTabSpare   = 2 * kBK;   // padding rows after the gather table (prefetch / unrolled look-ahead)
constexpr int kPanelSpare = 2 * kBK;   // zero rows after the weight panel
constexpr int kKoutAlign = 128;  // packed panel width is a multiple of this
constexpr int kMaxConvDests = PVHIP_MAX_CONV_DESTS;

struct ConvArgs {
    const float* x;
    const int*   ktab;  // [2][kred_pad + 2*kBK] : byte offsets c*H*W + r*W + s, then bit indices r*kw + s
    const float* wp;    // [kred_pad][kout_pad]
    float*       y;
    const float* bias;  // optional [K]
    int N, C, H, W, K, OH, OW;
    int sh, sw, pt, pl, kh, kw;
    unsigned x_bytes, wp_bytes;
    int kred_pad, kout_pad;
    int P;              // N*OH*OW
    int n_mtiles, n_ptiles;
    int   relu;             // epilogue activation: 0 none, 1 ReLU (ReLU.py:11), 2 clamp to [act_lo, act_hi] (Clamp.py:11)
    float act_lo, act_hi;
    int y_ctotal, y_coff;   // channels of the tensor y points into, and this convolution's first channel in it
    // Several convolutions of the same input as one launch (conv_igemm_dma_kernel only): the panel holds their output
    // channels one after the other, each range padded to whole 32-channel tiles; a tile belongs to one range and stores
    // into that range's tensor.  nseg == 0: the single destination above.
    int nseg;
    struct Seg {
        float* y;
        int m_begin, k;     // first panel row of the range, real output channels in it
        int ctotal, coff;   // as y_ctotal / y_coff
        int layout;         // 0: fp32 NCHW; 1 (f16 form only): fp16, channels blocked by eight ([n][ceil16(k) / 8][oh * ow][8]: pvhip_conv_dest)
    } seg[kMaxConvDests];
};

inline int round_up_int(int v, int q) { return (v + q - 1) / q * q; }

// Is the (r,s)-major reduction order (panel row = (r*kw + s)*C + c: a stage is 16 channels of one tap) used for this weight shape?
inline bool rs_major(int c, int kh, int kw) { return c % kBK == 0 && kh * kw < 64; }

// The window-bit mask of a lane has 64 bits: the LDS-DMA kernel takes every window of fewer taps, conv_igemm_kernel<.., false> the others.
inline bool dma_takes(int kh, int kw) { return kh * kw < 64; }

// The packed weight buffer (pvhip_conv2d_pack_f32 writes it, every pvhip_conv2d_* entry reads it), in floats; only this struct knows the layout:
//   two int tables of kred_pad + kTabSpare entries (gather offsets, then window bits: conv_pack_kernel); the K-major panel
//   [kred_pad + kPanelSpare][kout_pad]; behind it, by window (stride and padding are not known yet): 1x1 the pointwise kernel's panel,
//   3x3 the F(2x2,3x3) panel and then the F(4x4,3x3) panel, 5x5 the F(2x2,5x5) panel (0 floats: not applicable to this C).
struct ConvPanel {
    int    kred_pad, kout_pad;
    size_t tab, panel;                                  // floats of the two tables / of the K-major panel, spare stages included
    size_t pw = 0, wino2 = 0, wino4 = 0, wino25 = 0;    // floats of the panels that ride behind it
    ConvPanel(int k_out, int c, int kh, int kw)
        : kred_pad(round_up_int(c * kh * kw, kBK)), kout_pad(round_up_int(k_out, kKoutAlign)),
          tab(2 * (size_t)(kred_pad + kTabSpare)), panel((size_t)(kred_pad + kPanelSpare) * kout_pad) {
        if (kh == 1 && kw == 1) pw = pw_pack_elems(k_out, c);
        if (kh == 3 && kw == 3) { wino2 = wino_pack_elems(k_out, c); wino4 = wino4_pack_elems(k_out, c); }
        if (kh == 5 && kw == 5) wino25 = wino4_pack_elems(k_out, c);
    }
    size_t elems() const { return tab + panel + pw + wino2 + wino4 + wino25; }
    template <class F> F* wp(F* wpack) const { return wpack + tab; }
    template <class F> F* riders(F* wpack) const { return wpack + tab + panel; }            // the 1x1, F(2x2,3x3) or F(2x2,5x5) panel
    template <class F> F* wino4_panel(F* wpack) const { return wpack + tab + panel + wino2; }
};

// Only the diagnostic build (-DPVHIP_DIAG, libpvhip_diag.so) can switch the LDS-DMA kernel off (PVHIP_CONV_KERNEL=lds) and override a launch:
#ifdef PVHIP_DIAG
constexpr bool kDiagBuild = true;
inline bool dma_enabled() { return settings().conv_kernel != 1; }
// pvhip_diag_conv.hip, given the tile the product chose for its general kernel.  true: a predecessor kernel took the launch, *rc is the
// entry's result.  false: the product launches, on *bm x 128 (PVHIP_CONV_TILE may have changed *bm, to 128 as well).
bool diag_conv_override(ConvArgs& a, int* bm, int* bn, int* rc);
#else
constexpr bool kDiagBuild = false;
inline bool dma_enabled() { return true; }
#endif

// Kernels of this header are internal to each translation unit that includes it: every .hip file registers a code object of its own.
namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

// One gather element of the im2col tile: returns x[n, c, ih0 + r, iw0 + s] or 0 for a padding cell.
// koff / rs are the wave-uniform table entry of the reduction row (byte offset c*H*W + r*W + s, and
// the bit index r*kw + s -- or (r << 8) | s on the compare path), `inb` is the lane's in-bounds bit
// mask over (r, s), `xoff` the lane's byte offset of x[n, 0, ih0, iw0].  An out-of-bounds cell becomes
// an out-of-range buffer offset (the hardware returns 0): no branch, no select on the data.
template <bool kMask>
__device__ __forceinline__ float gather_one(__amdgpu_buffer_rsrc_t xr, int koff, int rs, unsigned long long inb,
                                            unsigned xoff, int ih0, int iw0, int H, int W) {
    unsigned bit;
    if (kMask) {
        bit = (unsigned)(inb >> rs) & 1u;   // padding rows carry rs = 63, a bit that is never set
    } else {
        const int r = rs >> 8, s = rs & 0xff;   // padding rows carry r = 0x7fff
        bit = (((unsigned)(ih0 + r) < (unsigned)H) & ((unsigned)(iw0 + s) < (unsigned)W)) ? 1u : 0u;
    }
    // The whole offset goes through the VGPR: the 32-bit wrap of xoff + koff is what makes a window that
    // starts in the top/left padding (xoff "negative") land on the right element.  A padding cell gets
    // the offset 2^31, which is >= num_records (the host checks x_bytes <= 2^31) and, unlike an all-ones
    // offset, cannot wrap back into range when the address unit adds the access size.
    const unsigned off = bit ? (xoff + (unsigned)koff) : 0x80000000u;
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, off, 0, 0));
}

// Register-staged double buffering: global loads of step t+1 are issued before the MFMAs of step t and written to the other LDS buffer
// after them; one barrier per step.  kMask: window-bit mask (fewer than 64 taps; diagnostic build), else a compare per gathered element.
template <int BM, int BN, int WAVES_M, int WAVES_N, bool kMask>
__global__ __launch_bounds__(kBlock, 2) void conv_igemm_kernel(ConvArgs a) {
    static_assert(WAVES_M * WAVES_N == kBlock / kWave, "4 waves per workgroup");
    constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
    constexpr int TM = WM / 32, TN = WN / 32;
    static_assert(TM >= 1 && TN >= 1 && WM % 32 == 0 && WN % 32 == 0, "wave tile is a multiple of 32x32");
    static_assert(BN % kWave == 0 && kBlock % BN == 0, "a wave gathers whole reduction rows");
    constexpr int B_LOADS    = kBK * BN / kBlock;   // reduction rows gathered per lane per stage
    constexpr int A_F4_TOTAL = kBK * BM / 4;
    constexpr int A_F4       = (A_F4_TOTAL + kBlock - 1) / kBlock;
    constexpr int KK         = kBK / 2;             // MFMA steps per stage

    __shared__ __attribute__((aligned(16))) float As[2][kBK][BM];
    __shared__ __attribute__((aligned(16))) float Bs[2][kBK][BN];

    // ---- tile assignment: XCD-aware remap so that workgroups sharing an L2 work on neighbouring
    // pixel tiles and all output-channel tiles of one pixel tile run back to back on one XCD.
    const int nwg = gridDim.x;
    const int lid = xcd_tile(blockIdx.x, nwg);
    const int mt    = lid % a.n_mtiles;
    const int ptile = lid / a.n_mtiles;
    const int m0    = mt * BM;

    const int tid  = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wid  = __builtin_amdgcn_readfirstlane(tid / kWave);

    // ---- this lane's output pixel for the gather
    const int OHW = a.OH * a.OW;
    const int HW  = a.H * a.W;
    const int pc  = tid % BN;
    const int prow0 = __builtin_amdgcn_readfirstlane(tid / BN) * B_LOADS;  // first reduction row of this wave
    int                ih0 = 0, iw0 = 0;
    unsigned           xoff = 0;
    unsigned long long inb  = 0;
    {
        const int gp = ptile * BN + pc;
        if (gp < a.P) {
            const int n   = gp / OHW;
            const int rem = gp - n * OHW;
            const int oy  = rem / a.OW;
            const int ox  = rem - oy * a.OW;
            ih0           = oy * a.sh - a.pt;
            iw0           = ox * a.sw - a.pl;
            xoff          = (unsigned)(n * a.C * HW + ih0 * a.W + iw0) * 4u;
            if (kMask) {
                for (int r = 0; r < a.kh; ++r)
                    for (int s = 0; s < a.kw; ++s)
                        if ((unsigned)(ih0 + r) < (unsigned)a.H && (unsigned)(iw0 + s) < (unsigned)a.W)
                            inb |= 1ull << (r * a.kw + s);
            }
        } else {
            ih0 = INT_MIN / 2;  // every bounds test fails; the mask stays 0
        }
    }
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, a.x_bytes, 0x00020000);

    float  breg[B_LOADS];
    float4 areg[A_F4];
    int    tko[B_LOADS], trs[B_LOADS];   // table entries of the NEXT stage to gather (scalar registers)
    const int* __restrict__ tab_rs = a.ktab + a.kred_pad + kTabSpare;

#define PV_LOAD_ENT(kt_)                                                              \
    {                                                                                 \
        const int* __restrict__ tp = a.ktab + (kt_) * kBK + prow0;                    \
        const int* __restrict__ tq = tab_rs + (kt_) * kBK + prow0;                    \
        _Pragma("unroll") for (int j = 0; j < B_LOADS; ++j) { tko[j] = tp[j]; trs[j] = tq[j]; } \
    }
#define PV_GATHER(j_) breg[j_] = gather_one<kMask>(xr, tko[j_], trs[j_], inb, xoff, ih0, iw0, a.H, a.W)
#define PV_LOAD_A(kt_)                                                                \
    _Pragma("unroll") for (int j = 0; j < A_F4; ++j) {                                \
        const int f = tid + j * kBlock;                                               \
        if (A_F4_TOTAL % kBlock == 0 || f < A_F4_TOTAL) {                             \
            const int arow = f / (BM / 4), ac4 = f % (BM / 4);                        \
            areg[j] = *reinterpret_cast<const float4*>(a.wp + (size_t)((kt_) * kBK + arow) * a.kout_pad + m0 + ac4 * 4); \
        }                                                                             \
    }
#define PV_STORE_TILES(buf_)                                                          \
    {                                                                                 \
        _Pragma("unroll") for (int j = 0; j < B_LOADS; ++j) Bs[buf_][prow0 + j][pc] = breg[j]; \
        _Pragma("unroll") for (int j = 0; j < A_F4; ++j) {                            \
            const int f = tid + j * kBlock;                                           \
            if (A_F4_TOTAL % kBlock == 0 || f < A_F4_TOTAL) {                         \
                const int arow = f / (BM / 4), ac4 = f % (BM / 4);                    \
                *reinterpret_cast<float4*>(&As[buf_][arow][ac4 * 4]) = areg[j];       \
            }                                                                         \
        }                                                                             \
    }

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int wm  = wid / WAVES_N, wn = wid % WAVES_N;
    const int l31 = lane & 31, lh = lane >> 5;
    const int a_col = wm * WM + l31;
    const int b_col = wn * WN + l31;

    const int nk = a.kred_pad / kBK;
    // prologue: stage 0 into LDS buffer 0; table entries of stage 1 into scalar registers
    PV_LOAD_ENT(0);
#pragma unroll
    for (int j = 0; j < B_LOADS; ++j) PV_GATHER(j);
    PV_LOAD_A(0);
    PV_STORE_TILES(0);
    PV_LOAD_ENT(1);   // the table has one spare stage of padding rows at its end
    __syncthreads();

    // The loop body has no conditionals: the last iteration gathers and stages one stage past the end
    // (table rows there are padding rows -> the loads read as 0; the weight panel has one spare zero
    // stage), which keeps every wait counter of the body exact.
    //
    // Order inside one stage (pinned with sched_barrier so the scheduler cannot sink the global loads
    // behind the MFMAs, which would expose their whole latency before the LDS write):
    //   1. LDS reads of the first MFMA step of stage kt          (latency hidden behind 2.)
    //   2. all global loads of stage kt+1 (A panel + gather)      (in flight during 3.)
    //   3. MFMA steps of stage kt, operands of step kk+1 read from LDS before the MFMAs of step kk
    //   4. table prefetch for stage kt+2, LDS write of stage kt+1, barrier
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        float af[2][TM], bf[2][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[0][i] = As[buf][lh][a_col + i * 32];
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[0][j] = Bs[buf][lh][b_col + j * 32];
        PV_LOAD_A(kt + 1);
#pragma unroll
        for (int j = 0; j < B_LOADS; ++j) PV_GATHER(j);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const int cur = kk & 1, nxt = cur ^ 1;
            if (kk + 1 < KK) {
#pragma unroll
                for (int i = 0; i < TM; ++i) af[nxt][i] = As[buf][2 * (kk + 1) + lh][a_col + i * 32];
#pragma unroll
                for (int j = 0; j < TN; ++j) bf[nxt][j] = Bs[buf][2 * (kk + 1) + lh][b_col + j * 32];
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][i], bf[cur][j], acc[i][j], 0, 0, 0);
            // emit this step as: LDS reads of step kk+1, then the MFMAs of step kk
            if (kk + 1 < KK) __builtin_amdgcn_sched_group_barrier(0x100, TM + TN, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, TM * TN, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        PV_LOAD_ENT(kt + 2);   // consumed one whole stage later
        PV_STORE_TILES(buf ^ 1);
        __syncthreads();
    }
#undef PV_LOAD_ENT
#undef PV_GATHER
#undef PV_LOAD_A
#undef PV_STORE_TILES

    // ---- epilogue: accumulator register r of lane l is D[row = (r&3) + 8*(r>>2) + 4*(l>>5)][col = l&31]
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int gp = ptile * BN + wn * WN + j * 32 + l31;
        if (gp >= a.P) continue;
        const int    n    = gp / OHW;
        const int    rem  = gp - n * OHW;
        float* __restrict__ yp = a.y + ((size_t)n * a.y_ctotal + a.y_coff) * OHW + rem;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ko = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (ko < a.K) {
                    float v = acc[i][j][r];
                    if (a.bias != nullptr) v = v + a.bias[ko];
                    v = act_apply(v, act_bounds(a.relu, a.act_lo, a.act_hi));
                    conv_store1(yp + (size_t)ko * OHW, v);
                }
            }
        }
    }
}

}  // namespace
}  // namespace pvhip
