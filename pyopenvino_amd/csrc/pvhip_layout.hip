// Input-format conversion (HBM-bound): the staged host input of a request -- 8-bit pixels and / or channels-last, as a cv2 image
// is -- becomes the fp32 NCHW tensor the network's Parameter expects, in ONE launch on the device.  Exact by construction: every
// u8 value is an fp32 value, and an fp32 input is moved, never computed on.
//
//   U8 NCHW:   a widening copy (u8_to_f32_kernel): 4 bytes per lane in, one float4 nontemporal store out.
//   U8 / FP32 NHWC: per image a (h*w) x c -> c x (h*w) transpose (nhwc_to_nchw_kernel).  A workgroup owns `tile` consecutive pixels
//   of one image: their tile*c inputs are one contiguous span (16-byte loads), and the outputs of every channel are one contiguous
//   span of `tile` floats (float4 nontemporal stores).  The channels are de-interleaved in LDS in between.  Whether the 16-byte
//   forms apply is decided per launch from the alignment of the spans (any h, w, c works: the rest takes masked / scalar tails).
#include "pvhip_common.h"

using namespace pvhip;

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void stg4_nt(float* p, float a, float b, float c, float d) {
    f4v v;
    v.x = a; v.y = b; v.z = c; v.w = d;
    __builtin_nontemporal_store(v, reinterpret_cast<f4v*>(p));
}

__device__ __forceinline__ u4v ldg16_nt(const unsigned char* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const u4v*>(p));
}

// y[i] = float(x[i]).  n4: number of whole 4-byte words the vector loop takes (0 when a pointer is not aligned).  One word per lane: a
// wave's loads are 256 contiguous bytes and its float4 stores 1 KiB contiguous (16 bytes in and four float4 out per lane left each
// store instruction a quarter of its span: 1.6 TB/s).
__global__ __launch_bounds__(kBlock) void u8_to_f32_kernel(const unsigned char* __restrict__ x, float* __restrict__ y, size_t n4, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const unsigned* __restrict__ x4 = reinterpret_cast<const unsigned*>(x);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const unsigned w = __builtin_nontemporal_load(x4 + i);
        stg4_nt(y + 4 * i, (float)(w & 0xffu), (float)((w >> 8) & 0xffu), (float)((w >> 16) & 0xffu), (float)(w >> 24));
    }
    for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = (float)x[i];
}

// grid (ceil(p / tile), n); dynamic LDS tile * c * sizeof(T) bytes.  p = h * w.
// VL: every tile's input span starts 16-byte aligned (x aligned, p*c*sizeof(T) and tile*c*sizeof(T) multiples of 16).
// VS: every channel's output span starts 16-byte aligned and holds a multiple of four floats (y aligned, p and tile multiples of 4).
template <typename T, bool VL, bool VS>
__global__ __launch_bounds__(kBlock) void nhwc_to_nchw_kernel(const T* __restrict__ x, float* __restrict__ y, int c, unsigned p, unsigned tile) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const unsigned n     = blockIdx.y;
    const unsigned p0    = blockIdx.x * tile;
    const unsigned valid = min(tile, p - p0);
    const size_t   elems = (size_t)valid * (unsigned)c;
    const T* __restrict__ src = x + ((size_t)n * p + p0) * (unsigned)c;
    T* l = reinterpret_cast<T*>(lds);
    if (VL) {
        const size_t bytes = elems * sizeof(T);
        const unsigned char* s8 = reinterpret_cast<const unsigned char*>(src);
        for (size_t i = threadIdx.x; i < bytes / 16; i += kBlock) reinterpret_cast<u4v*>(lds)[i] = ldg16_nt(s8 + i * 16);
        for (size_t i = bytes / 16 * 16 + threadIdx.x; i < bytes; i += kBlock) lds[i] = s8[i];        // masked tail of a partial tile
    } else {
        for (size_t i = threadIdx.x; i < elems; i += kBlock) l[i] = src[i];
    }
    __syncthreads();
    float* __restrict__ dst = y + (size_t)n * (unsigned)c * p + p0;
    for (int ch = 0; ch < c; ++ch, dst += p) {
        if (VS) {                       // valid is a multiple of 4 here (p and tile are)
            for (unsigned j = 4 * threadIdx.x; j < valid; j += 4 * kBlock) {
                const T* q = l + (size_t)j * c + ch;
                stg4_nt(dst + j, (float)q[0], (float)q[c], (float)q[2 * c], (float)q[3 * c]);
            }
        } else {
            for (unsigned j = threadIdx.x; j < valid; j += kBlock) dst[j] = (float)l[(size_t)j * c + ch];
        }
    }
}

constexpr size_t kTileBytes = 16384;     // LDS per workgroup at most (ten workgroups per CU still fit)

// What pvhip_input_to_nchw_f32 launches for a geometry and the two addresses modulo 16 (the entry switches on it, pvhip_input_to_nchw_form
// reports it).  U8_LINEAR: n4 words through the vector loop; NHWC: the tile, the two 16-byte forms and the grid.
struct InputPlan {
    int      kind = PVHIP_FORM_NONE;
    size_t   n4 = 0;
    unsigned tile = 0, gx = 0, gy = 0;
    bool     vl = false, vs = false;
};
InputPlan plan_input(int n, int c, size_t p, bool src_u8, bool src_nhwc, unsigned src_align, unsigned dst_align) {
    InputPlan    q;
    const size_t total = (size_t)n * (size_t)c * p;
    if (!src_nhwc && !src_u8) {
        q.kind = PVHIP_INPUT_COPY;
        return q;
    }
    if (!src_nhwc) {
        const bool vec = (src_align % 4 == 0) && (dst_align % 16 == 0);
        q.kind = PVHIP_INPUT_U8_LINEAR;
        q.n4   = vec ? total / 4 : 0;
        const size_t work = q.n4 > 0 ? q.n4 : total, blocks = (work + kBlock - 1) / kBlock;
        q.gx = (unsigned)(blocks < ((size_t)1 << 30) ? blocks : ((size_t)1 << 30));
        q.gy = 1;
        return q;
    }
    const size_t es = src_u8 ? 1 : sizeof(float);
    q.kind = PVHIP_INPUT_NHWC;
    q.tile = 1024;                       // 1024 pixels: one float4 per lane and channel
    while (q.tile > 1 && q.tile * (size_t)c * es > kTileBytes) q.tile >>= 1;
    q.vl = (src_align % 16 == 0) && (p * c * es) % 16 == 0 && ((size_t)q.tile * c * es) % 16 == 0;
    q.vs = (dst_align % 16 == 0) && p % 4 == 0 && q.tile % 4 == 0;
    q.gx = (unsigned)((p + q.tile - 1) / q.tile);
    q.gy = (unsigned)n;
    return q;
}

template <typename T>
int launch_nhwc(const InputPlan& q, const T* x, float* y, int c, unsigned p, hipStream_t st) {
    const dim3     grid(q.gx, q.gy);
    const unsigned tile = q.tile;
    const size_t   lds  = (size_t)tile * c * sizeof(T);
    if (q.vl && q.vs) hipLaunchKernelGGL((nhwc_to_nchw_kernel<T, true, true>), grid, dim3(kBlock), lds, st, x, y, c, p, tile);
    else if (q.vl)    hipLaunchKernelGGL((nhwc_to_nchw_kernel<T, true, false>), grid, dim3(kBlock), lds, st, x, y, c, p, tile);
    else if (q.vs)    hipLaunchKernelGGL((nhwc_to_nchw_kernel<T, false, true>), grid, dim3(kBlock), lds, st, x, y, c, p, tile);
    else              hipLaunchKernelGGL((nhwc_to_nchw_kernel<T, false, false>), grid, dim3(kBlock), lds, st, x, y, c, p, tile);
    return PVHIP_OK;
}

// The argument checks of the entry that do not look at the pointers.
int check_input_geometry(const char* who, int n, int c, int h, int w, int src_nhwc) {
    PVHIP_CHECK_ARG_AS(who, n > 0 && c > 0 && h > 0 && w > 0 && n <= 65535);
    PVHIP_CHECK_ARG_AS(who, (size_t)h * (size_t)w * (size_t)c < ((size_t)1 << 31));       // one image's elements index in 32 bits
    if (src_nhwc) PVHIP_CHECK_ARG_AS(who, c <= 4096);          // one pixel's channels fit the LDS tile
    return PVHIP_OK;
}

}  // namespace

extern "C" {

int pvhip_input_to_nchw_f32(const void* src, float* dst, int n, int c, int h, int w, int src_u8, int src_nhwc) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(src != nullptr && dst != nullptr);
    const int rc = check_input_geometry("pvhip_input_to_nchw_f32", n, c, h, w, src_nhwc);
    if (rc) return rc;
    const size_t p = (size_t)h * (size_t)w;
    const size_t total = (size_t)n * (size_t)c * p;
    hipStream_t st = state().stream;
    const InputPlan q = plan_input(n, c, p, src_u8 != 0, src_nhwc != 0, (unsigned)((uintptr_t)src % 16), (unsigned)((uintptr_t)dst % 16));
    if (q.kind == PVHIP_INPUT_COPY) {   // nothing to convert
        PVHIP_HIP(hipMemcpyAsync(dst, src, total * sizeof(float), hipMemcpyDeviceToDevice, st));
        return PVHIP_OK;
    }
    if (q.kind == PVHIP_INPUT_U8_LINEAR) {
        hipLaunchKernelGGL(u8_to_f32_kernel, dim3(q.gx), dim3(kBlock), 0, st, (const unsigned char*)src, dst, q.n4, total);
    } else if (src_u8) {
        launch_nhwc(q, (const unsigned char*)src, dst, c, (unsigned)p, st);
    } else {
        launch_nhwc(q, (const float*)src, dst, c, (unsigned)p, st);
    }
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

int pvhip_input_to_nchw_form(int n, int c, int h, int w, int src_u8, int src_nhwc, int src_align, int dst_align, int* form) {
    PVHIP_CHECK_ARG(form != nullptr);
    for (int i = 0; i < PVHIP_FORM_INTS; ++i) form[i] = 0;
    form[PVHIP_INPUT_FORM_KIND] = PVHIP_FORM_NONE;
    PVHIP_CHECK_ARG(src_align >= 0 && src_align < 16 && dst_align >= 0 && dst_align < 16);
    const int rc = check_input_geometry("pvhip_input_to_nchw_form", n, c, h, w, src_nhwc);
    if (rc) return rc;
    const InputPlan q = plan_input(n, c, (size_t)h * (size_t)w, src_u8 != 0, src_nhwc != 0, (unsigned)src_align, (unsigned)dst_align);
    form[PVHIP_INPUT_FORM_KIND]   = q.kind;
    form[PVHIP_INPUT_FORM_VEC]    = q.n4 > 0 ? 1 : 0;
    form[PVHIP_INPUT_FORM_TILE]   = (int)q.tile;
    form[PVHIP_INPUT_FORM_VL]     = q.vl ? 1 : 0;
    form[PVHIP_INPUT_FORM_VS]     = q.vs ? 1 : 0;
    form[PVHIP_INPUT_FORM_GRID_X] = (int)q.gx;
    form[PVHIP_INPUT_FORM_GRID_Y] = (int)q.gy;
    return PVHIP_OK;
}

}  // extern "C"
