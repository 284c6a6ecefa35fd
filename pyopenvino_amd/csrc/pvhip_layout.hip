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

template <typename T>
int launch_nhwc(const T* x, float* y, int n, int c, unsigned p, hipStream_t st) {
    const size_t es = sizeof(T);
    unsigned tile = 1024;                // 1024 pixels: one float4 per lane and channel
    while (tile > 1 && tile * (size_t)c * es > kTileBytes) tile >>= 1;
    const bool vl = ((uintptr_t)x % 16 == 0) && ((size_t)p * c * es) % 16 == 0 && ((size_t)tile * c * es) % 16 == 0;
    const bool vs = ((uintptr_t)y % 16 == 0) && p % 4 == 0 && tile % 4 == 0;
    const dim3 grid((p + tile - 1) / tile, (unsigned)n);
    const size_t lds = (size_t)tile * c * es;
    if (vl && vs)  hipLaunchKernelGGL((nhwc_to_nchw_kernel<T, true, true>), grid, dim3(kBlock), lds, st, x, y, c, p, tile);
    else if (vl)   hipLaunchKernelGGL((nhwc_to_nchw_kernel<T, true, false>), grid, dim3(kBlock), lds, st, x, y, c, p, tile);
    else if (vs)   hipLaunchKernelGGL((nhwc_to_nchw_kernel<T, false, true>), grid, dim3(kBlock), lds, st, x, y, c, p, tile);
    else           hipLaunchKernelGGL((nhwc_to_nchw_kernel<T, false, false>), grid, dim3(kBlock), lds, st, x, y, c, p, tile);
    return PVHIP_OK;
}

}  // namespace

extern "C" {

int pvhip_input_to_nchw_f32(const void* src, float* dst, int n, int c, int h, int w, int src_u8, int src_nhwc) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(src != nullptr && dst != nullptr);
    PVHIP_CHECK_ARG(n > 0 && c > 0 && h > 0 && w > 0 && n <= 65535);
    const size_t p = (size_t)h * (size_t)w;
    PVHIP_CHECK_ARG(p * (size_t)c < ((size_t)1 << 31));       // one image's elements index in 32 bits
    const size_t total = (size_t)n * (size_t)c * p;
    hipStream_t st = state().stream;
    if (src_nhwc) PVHIP_CHECK_ARG(c <= 4096);                  // one pixel's channels fit the LDS tile
    if (!src_nhwc && !src_u8) {         // nothing to convert
        PVHIP_HIP(hipMemcpyAsync(dst, src, total * sizeof(float), hipMemcpyDeviceToDevice, st));
        return PVHIP_OK;
    }
    if (!src_nhwc) {
        const bool vec = ((uintptr_t)src % 4 == 0) && ((uintptr_t)dst % 16 == 0);
        const size_t n4 = vec ? total / 4 : 0;
        const size_t work = n4 > 0 ? n4 : total, blocks = (work + kBlock - 1) / kBlock;
        hipLaunchKernelGGL(u8_to_f32_kernel, dim3((unsigned)(blocks < ((size_t)1 << 30) ? blocks : ((size_t)1 << 30))), dim3(kBlock), 0, st,
                           (const unsigned char*)src, dst, n4, total);
    } else if (src_u8) {
        launch_nhwc((const unsigned char*)src, dst, n, c, (unsigned)p, st);
    } else {
        launch_nhwc((const float*)src, dst, n, c, (unsigned)p, st);
    }
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // extern "C"
