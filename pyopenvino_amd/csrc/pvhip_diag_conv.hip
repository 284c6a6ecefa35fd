// Diagnostic build only (libpvhip_diag.so; include/pvhip_diag.h), never part of libpvhip.so: the predecessors of the convolution kernels of
// pvhip_conv.hip, kept for A/B measurements (scripts/tune_conv.py, tests/diag_variants.py), and the tile overrides.
//   PVHIP_CONV_KERNEL=lds    conv_igemm_rs_kernel ((r,s)-major; PVHIP_CONV_PW=1: its 16-byte pointwise gather) and the window-bit form
//                            conv_igemm_kernel<.., true> (pvhip_conv_igemm.h) instead of the LDS-DMA kernel
//   PVHIP_CONV_KERNEL=wave   conv_wave_kernel for c-major layers (PVHIP_CONV_WTILE=TMxTN in units of 32; PVHIP_CONV_ABLATE: wrong on purpose)
//   PVHIP_CONV_TILE=BMxBN    every tile of the register-staged kernels; 32|64|128 x 128 of the LDS-DMA kernel, which pvhip_conv.hip launches
// pvhip_conv.hip calls diag_conv_override once per launch of its general kernel.
#include "pvhip_conv_igemm.h"

using namespace pvhip;

namespace {

// ---------------------------------------------------------------------------------------------------
// (r,s)-major variant of the LDS-tiled kernel, used whenever C is a multiple of the stage depth (16).
//
// On gfx950 the fp32 MFMA executes on the SIMD's vector FMA lanes: VALU instructions do not co-issue with
// it (SQ_VALU_MFMA_COEXEC_CYCLES == 0 on this kernel family), so every VALU instruction in the reduction
// loop is MFMA time lost.  The c-major reduction order needs ~5 VALU per gathered element (window-bit
// test, offset add, select).  Ordering the reduction (r,s)-major instead -- row = (r*kw + s)*C + c, the
// weight panel is packed to match -- makes the window tap constant over the C/16 stages of one (r,s):
// the lane's byte offset `voff` (or the out-of-range sentinel when the tap falls in the padding) is
// computed once per tap, and the 16 channel rows of a stage differ only by a wave-uniform soffset
// c*H*W*4 handled by the scalar unit.  The gather is then buffer_load_dword voff, soffset with ZERO
// VALU instructions per element.  Everything else (LDS staging, stage order, tiles) is as in
// conv_igemm_kernel.  Epilogue: bias is fetched with range-checked buffer loads (no per-element bounds code).
template <int BM, int BN, int WAVES_M, int WAVES_N, bool kPW>   // kPW: pointwise (1x1, stride 1, no padding, H*W % 4 == 0)
__global__ __launch_bounds__(kBlock, 2) void conv_igemm_rs_kernel(ConvArgs a) {
    static_assert(WAVES_M * WAVES_N == kBlock / kWave, "4 waves per workgroup");
    constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
    constexpr int TM = WM / 32, TN = WN / 32;
    static_assert(TM >= 1 && TN >= 1 && WM % 32 == 0 && WN % 32 == 0, "wave tile is a multiple of 32x32");
    static_assert(BN % kWave == 0 && kBlock % BN == 0, "a wave gathers whole reduction rows");
    constexpr int B_LOADS    = kBK * BN / kBlock;         // dword gather: rows per lane per stage
    constexpr int B_LOADS4   = kBK * BN / 4 / kBlock;     // pointwise: 16-byte loads per lane per stage
    constexpr int QUADS      = BN / 4;                    // pixel quads per tile row
    constexpr int ROWS_PASS  = kBlock / QUADS;            // tile rows covered by one pass of the workgroup
    constexpr int A_F4_TOTAL = kBK * BM / 4;
    constexpr int A_F4       = (A_F4_TOTAL + kBlock - 1) / kBlock;
    constexpr int KK         = kBK / 2;
    constexpr unsigned kOob  = 0x80000000u;
    static_assert(QUADS % 32 == 0 || QUADS == 32, "a half wave covers whole tile rows");

    __shared__ __attribute__((aligned(16))) float As[2][kBK][BM];
    __shared__ __attribute__((aligned(16))) float Bs[2][kBK][BN];

    const int nwg = gridDim.x;
    int       lid;
    {
        const int bid = blockIdx.x;
        const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
        lid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    const int mt    = lid % a.n_mtiles;
    const int ptile = lid / a.n_mtiles;
    const int m0    = mt * BM;

    const int tid  = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wid  = __builtin_amdgcn_readfirstlane(tid / kWave);

    const int OHW = a.OH * a.OW;
    const int HW  = a.H * a.W;
    const unsigned chan_bytes = (unsigned)HW * 4u;
    // dword gather: lane <-> one pixel, B_LOADS consecutive rows; pointwise: lane <-> one pixel quad of one row
    const int pc    = kPW ? (tid % QUADS) * 4 : tid % BN;
    const int prow0 = kPW ? 0 : __builtin_amdgcn_readfirstlane(tid / BN) * B_LOADS;
    const int qrow  = tid / QUADS;                       // pointwise: tile row of pass 0 (wave-uniform up to lane>>5)
    unsigned           xoff = 0;
    unsigned long long inb  = 0;     // bit (r*kw + s): tap inside the image for this lane's pixel
    {
        const int gp = ptile * BN + pc;
        if (gp < a.P) {
            const int n   = gp / OHW;
            const int rem = gp - n * OHW;
            if (kPW) {
                xoff = (unsigned)(n * a.C * HW + rem) * 4u;
                inb  = 1ull;
            } else {
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
    }
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, a.x_bytes, 0x00020000);
    const int* __restrict__ rstab = a.ktab;            // [kh*kw + spare]: (r*W + s)*4
    const int      ncs        = a.C / kBK;              // channel stages per tap
    const int      nrs        = a.kh * a.kw;

    float  breg[kPW ? 1 : B_LOADS];
    float4 breg4[kPW ? B_LOADS4 : 1];
    float4 areg[A_F4];

    // state of the stage being LOADED (one ahead of the stage being multiplied)
    int      rs_l = 0, cs_l = 0;
    unsigned voff = (inb & 1ull) ? xoff + (unsigned)rstab[0] : kOob;
    // pointwise: the lane's row inside a pass differs between the two half-waves only when a wave spans two
    // tile rows (QUADS == 32); that lane-constant part is folded into voff, the wave-uniform part is added to
    // the scalar row base.  Lanes whose pixel quad lies past the tensor read quad 0 (their columns are never
    // stored): plain global loads have no range check.
    const int qrow_u = __builtin_amdgcn_readfirstlane(qrow);          // row of lane 0 of this wave
    if (kPW) voff = ((inb & 1ull) ? xoff : 0u) + (unsigned)(qrow - qrow_u) * chan_bytes;

#define PV2_GATHER()                                                                                    \
    if (kPW) {                                                                                          \
        /* plain 16-byte global loads: uniform row base (scalar) + the lane's 32-bit byte offset.  (The     \
           16-byte raw-buffer-load builtins of this toolchain lower to a single dword load.) */            \
        _Pragma("unroll") for (int j = 0; j < B_LOADS4; ++j) {                                          \
            const char* rowp = reinterpret_cast<const char*>(a.x) +                                      \
                               (size_t)(cs_l * kBK + qrow_u + j * ROWS_PASS) * chan_bytes;               \
            breg4[j] = *reinterpret_cast<const float4*>(rowp + voff);                                   \
        }                                                                                               \
    } else {                                                                                            \
        const unsigned sbase = (unsigned)(cs_l * kBK + prow0) * chan_bytes;                             \
        _Pragma("unroll") for (int j = 0; j < B_LOADS; ++j)                                             \
            breg[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, voff, sbase + (unsigned)j * chan_bytes, 0)); \
    }
#define PV2_ADVANCE()                                                                                   \
    if (++cs_l == ncs) {                                                                                \
        cs_l = 0;                                                                                       \
        ++rs_l;                                                                                         \
        if (kPW) {                                                                                      \
            --rs_l;                                     /* single tap: the look-ahead past the end re-reads stage 0 (unused) */ \
        } else {                                                                                        \
            const unsigned ro = (unsigned)rstab[rs_l];  /* spare zero entries past the last tap */      \
            voff = (rs_l < nrs && ((inb >> rs_l) & 1ull)) ? xoff + ro : kOob;                           \
        }                                                                                               \
    }
#define PV2_LOAD_A(kt_)                                                               \
    _Pragma("unroll") for (int j = 0; j < A_F4; ++j) {                                \
        const int f = tid + j * kBlock;                                               \
        if (A_F4_TOTAL % kBlock == 0 || f < A_F4_TOTAL) {                             \
            const int arow = f / (BM / 4), ac4 = f % (BM / 4);                        \
            areg[j] = *reinterpret_cast<const float4*>(a.wp + (size_t)((kt_) * kBK + arow) * a.kout_pad + m0 + ac4 * 4); \
        }                                                                             \
    }
#define PV2_STORE_TILES(buf_)                                                         \
    {                                                                                 \
        if (kPW) {                                                                    \
            _Pragma("unroll") for (int j = 0; j < B_LOADS4; ++j)                      \
                *reinterpret_cast<float4*>(&Bs[buf_][qrow + j * ROWS_PASS][pc]) = breg4[j]; \
        } else {                                                                      \
            _Pragma("unroll") for (int j = 0; j < B_LOADS; ++j) Bs[buf_][prow0 + j][pc] = breg[j]; \
        }                                                                             \
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

    const int nk = nrs * ncs;
    PV2_GATHER();
    PV2_ADVANCE();
    PV2_LOAD_A(0);
    PV2_STORE_TILES(0);
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        float af[2][TM], bf[2][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[0][i] = As[buf][lh][a_col + i * 32];
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[0][j] = Bs[buf][lh][b_col + j * 32];
        PV2_LOAD_A(kt + 1);
        PV2_GATHER();           // stage kt+1 (past the end: every lane reads the out-of-range sentinel -> 0)
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
            if (kk + 1 < KK) __builtin_amdgcn_sched_group_barrier(0x100, TM + TN, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, TM * TN, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        PV2_STORE_TILES(buf ^ 1);
        PV2_ADVANCE();
        __syncthreads();
    }
#undef PV2_GATHER
#undef PV2_ADVANCE
#undef PV2_LOAD_A
#undef PV2_STORE_TILES

    // ---- epilogue: accumulator register r of lane l is D[row = (r&3) + 8*(r>>2) + 4*(l>>5)][col = l&31]
    const __amdgpu_buffer_rsrc_t br = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bias), 0,
                                                                        a.bias != nullptr ? a.K * 4 : 0, 0x00020000);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int row0 = m0 + wm * WM + i * 32 + 4 * lh;      // this lane's rows: row0 + (r&3) + 8*(r>>2)
        float     bv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            // range-checked dword loads: channels >= K (and a null bias: 0 records) read as 0.  (16-byte buffer
            // loads through this descriptor return the first dword in all four lanes of the result on gfx950.)
            bv[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                br, (unsigned)(row0 + (r & 3) + 8 * (r >> 2)) * 4u, 0, 0));
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int gp = ptile * BN + wn * WN + j * 32 + l31;
            if (gp >= a.P) continue;
            const int n   = gp / OHW;
            const int rem = gp - n * OHW;
            float* __restrict__ yp = a.y + ((size_t)n * a.y_ctotal + a.y_coff + row0) * OHW + rem;
            float vv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) vv[r] = acc[i][j][r];
            bias_act_n<16>(vv, bv, a.bias != nullptr, a.relu, act_bounds(a.relu, a.act_lo, a.act_hi));
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dr = (r & 3) + 8 * (r >> 2);
                if (row0 + dr < a.K) conv_store1(yp + (size_t)dr * OHW, vv[r]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Wave-direct variant: no LDS staging of operands and no barriers in the reduction loop.
//
// With one VGPR per fp32 MFMA operand and a wave tile of (32*TM) output channels x (32*TN) pixels, the B
// (im2col) elements a wave needs are needed by no other wave of the workgroup, so staging them through
// LDS only adds writes, reads and a barrier per stage.  Here every lane gathers exactly the operand
// element the MFMA wants from it -- lane l supplies B[k = 2*step + (l>>5)][pixel = l&31] -- straight
// into registers, and likewise A[k][k_out = l&31] from the packed panel (128-byte runs; the panel is a
// few hundred KB and lives in L1/L2).  Two register sets alternate (stage t+1 loads are in flight under
// the MFMAs of stage t); waits are counted vmcnt.  The (byte offset, window bit) table of the reduction
// rows is copied to LDS once per workgroup and read per lane with ds_read_b64 (both lane halves read one
// address each: broadcast, conflict-free).  The 4 waves of a workgroup take consecutive output-channel
// tiles of the same pixel tile, so their B loads hit in L1.
template <int TM, int TN, bool kMask, int ABLATE = 0>   // ABLATE (diagnostic builds only): 1 = no B gather, 2 = no A loads
__global__ __launch_bounds__(kBlock, 2) void conv_wave_kernel(ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) int2 tab[];   // [kred_pad + kTabSpare] {koff bytes, rs}
    const int tid  = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wid  = __builtin_amdgcn_readfirstlane(tid / kWave);
    const int l31 = lane & 31, lh = lane >> 5;
    const int tab_n = a.kred_pad + kTabSpare;
    for (int i = tid; i < tab_n; i += kBlock) tab[i] = make_int2(a.ktab[i], a.ktab[tab_n + i]);
    __syncthreads();

    // ---- this wave's tile
    const long n_tiles = (long)a.n_mtiles * a.n_ptiles;
    long       t;
    {
        const int nwg = gridDim.x, bid = blockIdx.x;
        const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
        const int lid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
        t = (long)lid * (kBlock / kWave) + wid;
    }
    if (t >= n_tiles) return;   // no barrier after this point
    const int mt = (int)(t % a.n_mtiles);
    const int pt = (int)(t / a.n_mtiles);
    const int m0 = mt * (32 * TM);
    const int p0 = pt * (32 * TN);

    const int OHW = a.OH * a.OW, HW = a.H * a.W;
    int                ih0[TN], iw0[TN];
    unsigned           xoff[TN];
    unsigned long long inb[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int gp = p0 + j * 32 + l31;
        ih0[j] = INT_MIN / 2; iw0[j] = 0; xoff[j] = 0; inb[j] = 0;
        if (gp < a.P) {
            const int n   = gp / OHW;
            const int rem = gp - n * OHW;
            const int oy  = rem / a.OW;
            const int ox  = rem - oy * a.OW;
            ih0[j]        = oy * a.sh - a.pt;
            iw0[j]        = ox * a.sw - a.pl;
            xoff[j]       = (unsigned)(n * a.C * HW + ih0[j] * a.W + iw0[j]) * 4u;
            if (kMask) {
                for (int r = 0; r < a.kh; ++r)
                    for (int s = 0; s < a.kw; ++s)
                        if ((unsigned)(ih0[j] + r) < (unsigned)a.H && (unsigned)(iw0[j] + s) < (unsigned)a.W)
                            inb[j] |= 1ull << (r * a.kw + s);
            }
        }
    }
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wp), 0, a.wp_bytes, 0x00020000);
    const unsigned woff = (unsigned)(lh * a.kout_pad + m0 + l31) * 4u;   // lane part of the panel offset
    const unsigned wrow = (unsigned)a.kout_pad * 4u;                     // bytes per panel row

    float areg[2][TM][kBK / 2], breg[2][TN][kBK / 2];

#define PV_WLOAD(set_, kt_)                                                                               \
    {                                                                                                     \
        const int row0 = (kt_) * kBK;                                                                     \
        _Pragma("unroll") for (int s = 0; s < kBK / 2; ++s) {                                             \
            const int2 e = tab[row0 + 2 * s + lh];                                                        \
            _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                \
                breg[set_][j][s] = (ABLATE & 1) ? __builtin_bit_cast(float, (xoff[j] & 0xffffu) | 0x3f800000u) \
                                                : gather_one<kMask>(xr, e.x, e.y, inb[j], xoff[j], ih0[j], iw0[j], a.H, a.W); \
            _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                \
                areg[set_][i][s] = (ABLATE & 2) ? __builtin_bit_cast(float, (woff & 0xffffu) | 0x3f800000u)   \
                                                : __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(        \
                    wr, woff + (unsigned)(i * 128), (unsigned)(row0 + 2 * s) * wrow, 0));                 \
        }                                                                                                 \
    }
#define PV_WMMA(set_)                                                                                     \
    _Pragma("unroll") for (int s = 0; s < kBK / 2; ++s)                                                   \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                    \
            _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[set_][i][s], breg[set_][j][s], acc[i][j], 0, 0, 0);

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // Stages are processed in pairs with two register sets; an odd tail runs one stage past the end
    // (padding rows of the table read as 0, the panel has spare zero stages).
    const int nk = a.kred_pad / kBK;
    PV_WLOAD(0, 0);
    for (int kt = 0; kt < nk; kt += 2) {
        PV_WLOAD(1, kt + 1);
        __builtin_amdgcn_sched_barrier(0);
        PV_WMMA(0);
        __builtin_amdgcn_sched_barrier(0);
        PV_WLOAD(0, kt + 2);
        __builtin_amdgcn_sched_barrier(0);
        PV_WMMA(1);
        __builtin_amdgcn_sched_barrier(0);
    }
#undef PV_WLOAD
#undef PV_WMMA

#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int gp = p0 + j * 32 + l31;
        if (gp >= a.P) continue;
        const int n   = gp / OHW;
        const int rem = gp - n * OHW;
        float* __restrict__ yp = a.y + ((size_t)n * a.y_ctotal + a.y_coff) * OHW + rem;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ko = m0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
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

// The register-staged kernels on one tile: (r,s)-major layers on conv_igemm_rs_kernel, c-major ones on conv_igemm_kernel.
template <int BM, int BN, int WAVES_M, int WAVES_N>
void launch_staged(const ConvArgs& a, int n_ptiles) {
    const dim3 grid(a.n_mtiles * n_ptiles), block(kBlock);
    if (rs_major(a.C, a.kh, a.kw)) {
        const bool pointwise = a.kh == 1 && a.kw == 1 && a.sh == 1 && a.sw == 1 && a.pt == 0 && a.pl == 0 &&
                               a.OH == a.H && a.OW == a.W && (a.H * a.W) % 4 == 0 && settings().conv_pw16;   // 16-byte gather measured slower: opt-in
        const size_t dyn = (size_t)settings().conv_lds_pad_kb * 1024;
        if (pointwise) hipLaunchKernelGGL((conv_igemm_rs_kernel<BM, BN, WAVES_M, WAVES_N, true>), grid, block, dyn, state().stream, a);
        else hipLaunchKernelGGL((conv_igemm_rs_kernel<BM, BN, WAVES_M, WAVES_N, false>), grid, block, dyn, state().stream, a);
    } else if (dma_takes(a.kh, a.kw))
        hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WAVES_M, WAVES_N, true>), grid, block, 0, state().stream, a);
    else      // windows of 64 taps and more: a compare per element instead of the window-bit mask
        hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WAVES_M, WAVES_N, false>), grid, block, 0, state().stream, a);
}

// The wave-direct kernel: one 32 tm x 32 tn tile per wave, the gather table (tab_bytes) in dynamic LDS.
int launch_wave(ConvArgs& a, size_t tab_bytes) {
    const int tm = settings().wtile_m, tn = settings().wtile_n;
    a.n_mtiles = (a.K + 32 * tm - 1) / (32 * tm);
    a.n_ptiles = (a.P + 32 * tn - 1) / (32 * tn);
    const long n_tiles = (long)a.n_mtiles * a.n_ptiles;
    const dim3 grid((int)((n_tiles + 3) / 4)), block(kBlock);
    const bool mask    = a.kh * a.kw < 64;
#define PV_WAVE_LAUNCH(TM_, TN_)                                                                                    \
    do {                                                                                                            \
        if (mask) hipLaunchKernelGGL((conv_wave_kernel<TM_, TN_, true>), grid, block, tab_bytes, state().stream, a);  \
        else hipLaunchKernelGGL((conv_wave_kernel<TM_, TN_, false>), grid, block, tab_bytes, state().stream, a);      \
    } while (0)
#define PV_WAVE_ABLATE(TN_, V_) hipLaunchKernelGGL((conv_wave_kernel<2, TN_, true, V_>), grid, block, tab_bytes, state().stream, a)
    if (const int v = settings().conv_ablate) {   // PVHIP_CONV_ABLATE: results are wrong on purpose
        if (tm == 2 && tn == 1) { if (v == 1) PV_WAVE_ABLATE(1, 1); else if (v == 2) PV_WAVE_ABLATE(1, 2); else PV_WAVE_ABLATE(1, 3); }
        else                    { if (v == 1) PV_WAVE_ABLATE(2, 1); else if (v == 2) PV_WAVE_ABLATE(2, 2); else PV_WAVE_ABLATE(2, 3); }
    }
#undef PV_WAVE_ABLATE
    else if (tm == 1 && tn == 1) PV_WAVE_LAUNCH(1, 1);
    else if (tm == 1 && tn == 2) PV_WAVE_LAUNCH(1, 2);
    else if (tm == 2 && tn == 1) PV_WAVE_LAUNCH(2, 1);
    else if (tm == 2 && tn == 2) PV_WAVE_LAUNCH(2, 2);
    else if (tm == 4 && tn == 1) PV_WAVE_LAUNCH(4, 1);
    else if (tm == 1 && tn == 4) PV_WAVE_LAUNCH(1, 4);
    else return fail(PVHIP_EINVAL, "pvhip_conv2d_f32: unsupported PVHIP_CONV_WTILE %dx%d", tm, tn);
#undef PV_WAVE_LAUNCH
    return PVHIP_OK;
}

}  // namespace

bool pvhip::diag_conv_override(ConvArgs& a, int* bm, int* bn, int* rc) {
    const size_t tab_bytes = (size_t)(a.kred_pad + kTabSpare) * sizeof(int2);
    if (settings().conv_kernel == 2 && tab_bytes <= 60 * 1024 && !rs_major(a.C, a.kh, a.kw)) {
        *rc = launch_wave(a, tab_bytes);
        return true;
    }
    if (settings().tile_bm > 0) { *bm = settings().tile_bm; *bn = settings().tile_bn; }      // PVHIP_CONV_TILE
    const bool dma = *bn == 128 && dma_enabled() && dma_takes(a.kh, a.kw);
    if (dma || (settings().tile_bm == 0 && dma_enabled())) return false;      // the LDS-DMA kernel on this tile, or nothing overridden
    a.n_mtiles = (a.K + *bm - 1) / *bm;
    const int n_ptiles = (a.P + *bn - 1) / *bn;
    if (*bm == 128 && *bn == 256) launch_staged<128, 256, 2, 2>(a, n_ptiles);
    else if (*bm == 128 && dma_enabled()) launch_staged<128, 128, 1, 4>(a, n_ptiles);      // (a window of 64 taps and more)
    else if (*bm == 128) launch_staged<128, 128, 2, 2>(a, n_ptiles);
    else if (*bm == 64 && *bn == 256) launch_staged<64, 256, 1, 4>(a, n_ptiles);
    else if (*bm == 32 && *bn == 256) launch_staged<32, 256, 1, 4>(a, n_ptiles);
    else if (*bm == 64) launch_staged<64, 128, 1, 4>(a, n_ptiles);
    else launch_staged<32, 128, 1, 4>(a, n_ptiles);
    *rc = PVHIP_OK;
    return true;
}
