// Internal interface of the Winograd F(2x2, 3x3) convolution (pvhip_wino.hip), used by pvhip_conv.hip.
#pragma once
#include <cstddef>

namespace pvhip {

// 3x3, stride 1, pad 1 ("same"), C a multiple of 4, and not switched off with PVHIP_CONV_WINOGRAD=0
bool   wino_eligible(int c, int kh, int kw, int sh, int sw, int pad_top, int pad_left, int h, int w, int oh, int ow);
size_t wino_pack_elems(int k, int c);                                 // floats of the transformed weight panel (0: not applicable)
int    wino_pack(const float* w_oihw, float* u, int k, int c);       // enqueue the weight transform
int    wino_conv(const float* x, const float* u, float* y, int n, int c, int h, int w, int k_out, const float* bias, int act,
                 float act_lo, float act_hi, int out_channel_offset, int out_channels_total);

// F(4x4, 3x3): additionally H and W multiples of 4 and enough patches to fill the chip (PVHIP_CONV_WINOGRAD4=0 switches it off,
// =force drops the size rule)
bool   wino4_eligible(int c, int kh, int kw, int sh, int sw, int pad_top, int pad_left, int h, int w, int oh, int ow, int n);
size_t wino4_pack_elems(int k, int c);
int    wino4_pack(const float* w_oihw, float* u, int k, int c);
int    wino4_conv(int m, const float* x, const float* u, float* y, int n, int c, int h, int w, int k_out, const float* bias, int act,
                  float act_lo, float act_hi, int out_channel_offset, int out_channels_total);

// F(2x2, 5x5) on the same kernel (m = 2): 5x5 / stride 1 / pad 2 layers with even extents; its panel has wino4_pack_elems floats
bool   wino25_eligible(int c, int kh, int kw, int sh, int sw, int pad_top, int pad_left, int h, int w, int oh, int ow, int n);
int    wino25_pack(const float* w_oihw, float* u, int k, int c);

// Pointwise (1x1 / stride 1 / unpadded, C a multiple of 16) convolutions (pvhip_pw.hip): weights in MFMA-fragment order, one
// workgroup per pixel tile and group of <= 8 32-channel tiles; PVHIP_CONV_POINTWISE=0 selects the general kernel
struct PwDest {
    float* y;
    int    m_begin, k;      // first panel row of this destination's channels, real channels in it
    int    ctotal, coff;    // channels of the tensor y points into, first channel of this convolution in it
};
bool   pw_eligible(int c, int kh, int kw, int sh, int sw, int pad_top, int pad_left, int h, int w, int oh, int ow);
size_t pw_pack_elems(int k, int c);
int    pw_pack(const float* w_oihw, float* ap, int k, int c);
int    pw_conv(const float* x, const float* ap, int n, int c, int hw, int k_panel, const float* bias, int act, float act_lo, float act_hi,
               int ndest, const PwDest* dests);

// What each launcher above launches, decided in ONE plan function per launcher that reads no pointer: the launcher switches on the plan
// and on nothing else, pvhip_conv2d_form (no device needed) reports it.
struct PwPlan {
    int  T, S, tn, nchunk, stagger, grid;     // 32-channel tiles, 16-channel stages, channel tiles per workgroup, chunks of them, start lag, workgroups
    bool vec;                                 // 16-byte copies (hw % 4 == 0), else dword copies
};
PwPlan plan_pw(int n, int c, int hw, int k_panel);

struct WinoPlan {           // F(2x2, 3x3)
    int  kb, nt, waves, n_kb;                 // output channels / patches per workgroup, waves (4 / 8), channel blocks
    bool small;                               // the 32 x 32 four-wave form
    long grid;                                // workgroups (the launcher refuses more than 2^31 - 1)
};
WinoPlan plan_wino(int n, int h, int w, int k_out);

struct Wino4Plan {          // the six-point kernels: F(4x4, 3x3) (m = 4) and F(2x2, 5x5) (m = 2)
    int  m, n_kb, n_stages, s_order, n_tiles, grid;
    long tiles_max;                           // patch blocks x channel blocks (the launcher refuses more than 2^30 - 1)
    bool ragged, shared, walk;                // extents no multiple of m; conv_wino4s_kernel (shared V), else conv_wino4_kernel; n_tiles > grid
};
Wino4Plan plan_wino4(int m, int n, int c, int h, int w, int k_out);

}  // namespace pvhip
