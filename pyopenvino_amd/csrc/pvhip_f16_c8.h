// What the FP16 kernel family shares (pvhip_f16.hip, pvhip_f16stem.hip, pvhip_f16span.hip, pvhip_f16c8.hip, pvhip_f16c8m.hip,
// pvhip_f16c8pool.hip), each stated once: the vector types, the blocked tensor's and the weight-fragment panel's geometry with the one
// kernel that packs the panel, the producers' counted wait, the row-tile plan of the kernels that copy whole rows, where a
// convolution's output goes, and the NaN-propagating maximum of the pooling kernels.
//
// The c8 TENSOR: fp16, channels blocked by eight -- [N][c8_blocks(C)][H * W][8 halves]: the eight channels of a pixel are ONE 16-byte
// piece, the MFMA operand of a lane (v_mfma_f32_32x32x16_f16: lane (pixel n, half h) supplies reduction rows 8 h .. 8 h + 7).  Channels
// past C, up to whole 16-channel stages, are zeros.
//
// The fragment PANEL: w (K, C, ks, ks) fp32 -> fp16 fragments [mt][cs][tap][i][lane][q], one 16-byte load per lane and MFMA.  Output
// channels come in groups of up to 128 (mt < frag_mtiles(K)), a group in frag_tm(K) tiles of 32 (i; one tile per wave), the input
// channels in stages of 16 (cs < c8_blocks(C) / 2).  Lane `lane` of a fragment holds output channel (mt * tm + i) * 32 + lane % 32 at
// input channels cs * 16 + 8 * (lane / 32) + q; output channels past K and input channels past C (C is padded to whole stages) are
// zero.  Packed by conv_f16_c8_pack_kernel (pvhip_f16c8.hip), read by conv_f16_span_kernel, conv_f16_c8_kernel and c8m_consume;
// tests/ref64.py f16_fragments restates it and test_f16_fragment_panel_bits pins its bits.
#pragma once
#include "pvhip_common.h"

namespace pvhip {

typedef float    floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef unsigned uint4v __attribute__((ext_vector_type(4)));

inline int c8_blocks(int c) { return (c + 15) / 16 * 2; }             // channel blocks of a c8 tensor: whole 16-channel stages
inline int frag_mtiles(int k) { return (k + 127) / 128; }             // channel groups of up to 128: one tile per wave (two: 300 registers, one wave per SIMD)
inline int frag_tm(int k) { const int t32 = (k + 31) / 32, nm = frag_mtiles(k); return (t32 + nm - 1) / nm; }
inline size_t frag_panel_halves(int k, int c, int taps) { return (size_t)frag_mtiles(k) * (c8_blocks(c) / 2) * taps * frag_tm(k) * 512; }

// Launches the pack kernel on the current stream: wf takes frag_panel_halves(k, c, taps) halves.  The caller has checked its arguments
// and checks the launch.
void launch_frag_pack(const float* w_oihw, float* wf, int k, int c, int taps);

// Until at most n of this wave's copies are in flight (n: wave-uniform).  The count of s_waitcnt is an immediate, hence the table.
__device__ __forceinline__ void wait_vmcnt(int n) {
#if defined(__HIP_DEVICE_COMPILE__)
    switch (n < 62 ? n : 62) {
#define PVHIP_VMCNT_CASE(k_) case k_: asm volatile("s_waitcnt vmcnt(" #k_ ")" ::: "memory"); break;
#define PVHIP_VMCNT_CASE10(t_) PVHIP_VMCNT_CASE(t_##0) PVHIP_VMCNT_CASE(t_##1) PVHIP_VMCNT_CASE(t_##2) PVHIP_VMCNT_CASE(t_##3) PVHIP_VMCNT_CASE(t_##4) \
                               PVHIP_VMCNT_CASE(t_##5) PVHIP_VMCNT_CASE(t_##6) PVHIP_VMCNT_CASE(t_##7) PVHIP_VMCNT_CASE(t_##8) PVHIP_VMCNT_CASE(t_##9)
        PVHIP_VMCNT_CASE(1) PVHIP_VMCNT_CASE(2) PVHIP_VMCNT_CASE(3) PVHIP_VMCNT_CASE(4) PVHIP_VMCNT_CASE(5) PVHIP_VMCNT_CASE(6) PVHIP_VMCNT_CASE(7)
        PVHIP_VMCNT_CASE(8) PVHIP_VMCNT_CASE(9) PVHIP_VMCNT_CASE10(1) PVHIP_VMCNT_CASE10(2) PVHIP_VMCNT_CASE10(3) PVHIP_VMCNT_CASE10(4) PVHIP_VMCNT_CASE10(5)
        PVHIP_VMCNT_CASE(60) PVHIP_VMCNT_CASE(61) PVHIP_VMCNT_CASE(62)
#undef PVHIP_VMCNT_CASE10
#undef PVHIP_VMCNT_CASE
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;      // fewer in flight than allowed: correct, only slower
    }
#endif
}

// element-wise maximum of three fp16 x 8 vectors, a NaN in any of them wins (np.max, MaxPool.py:70)
__device__ __forceinline__ half8 pk_max3_nan(half8 a, half8 b, half8 c) {
    uint4v x = __builtin_bit_cast(uint4v, a), y = __builtin_bit_cast(uint4v, b), z = __builtin_bit_cast(uint4v, c), d;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned r;
        asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(x[i]), "v"(y[i]), "v"(z[i]));
        d[i] = r;
    }
#else
    d = x; (void)y; (void)z;
#endif
    return __builtin_bit_cast(half8, d);
}

// The row-tile plan of the kernels whose producer waves copy whole image rows of a c8 tensor into LDS (conv_f16_c8_kernel,
// conv_f16_c8m_kernel): a workgroup owns R whole rows (R * w <= 128 pixels) of one image, `tiles` of them cover it evenly, and a stage
// holds rows = R + 2 pad LDS rows per channel block -- at most max_rows of them (0: no cap).  nb: the 32-pixel blocks of a tile (2: up to
// 64 pixels, 4: up to 128).  Lane l of a copy fetches image column l - pad, so the row and its padding must fit 64 lanes.  For the
// module form the LDS row is 1 << stride_sh pixels, the smallest power of two from 8 on that holds w + 2 pad, one copy instruction
// moves 64 >> stride_sh rows, and a stage holds rows_pad of them: whole copy instructions.
struct C8RowTiles { int R, tiles, rows, nb, stride_sh, rows_pad; };
inline bool c8_row_tiles(int h, int w, int pad, int max_rows, C8RowTiles& t) {
    if (h <= 0 || w <= 0 || w + 2 * pad > 64) return false;
    int r = 128 / w;
    if (max_rows > 0 && r > max_rows - 2 * pad) r = max_rows - 2 * pad;
    if (r > h) r = h;
    if (r < 1) return false;
    t.tiles = (h + r - 1) / r;
    t.R     = (h + t.tiles - 1) / t.tiles;
    t.tiles = (h + t.R - 1) / t.R;
    t.rows  = t.R + 2 * pad;
    t.nb    = t.R * w <= 64 ? 2 : 4;
    t.stride_sh = 3;
    while ((1 << t.stride_sh) < w + 2 * pad) ++t.stride_sh;
    const int rpi = 64 >> t.stride_sh;
    t.rows_pad = (t.rows + rpi - 1) / rpi * rpi;
    return true;
}

// Where a convolution's fp32 NCHW output goes: a tensor of its own (out_channels_total == 0), or channels out_channel_offset .. + k of
// a wider one -- the Concat buffer behind it.  elems: the elements of that tensor, for the entry's 2^31 check (the kernels index it
// with 32-bit offsets).  The entry checks the range itself.
struct ConvPlace { int ctotal, coff; unsigned long long elems; };
inline ConvPlace conv_place(int n, int k, int oh, int ow, int out_channels_total, int out_channel_offset) {
    ConvPlace p;
    p.ctotal = out_channels_total > 0 ? out_channels_total : k;
    p.coff   = out_channels_total > 0 ? out_channel_offset : 0;
    p.elems  = (unsigned long long)n * p.ctotal * oh * ow;
    return p;
}

}  // namespace pvhip
