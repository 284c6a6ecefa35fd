/*
 * pvhip.h -- C ABI of libpvhip.so: the MI355X (gfx950) numeric back end that sits under the
 * pyopenvino op-plugin boundary `compute(node, inputs, kernel_type, debug)`.
 *
 * The reference (yas-sim/pyopenvino) is pure Python and has no FFI of its own, so these entry points
 * are what a binding for its per-layer hot path binds: one function per `kernel_<Op>_*` body of the
 * reference plugins, plus device memory / stream / event plumbing and one RCCL gather.  Each
 * declaration cites the reference function it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every function returns 0 on success, a negative PVHIP_E* code otherwise; it never throws and
 *     never synchronises the stream unless its comment says so; pvhip_last_error() returns a
 *     human-readable description of the last failure on this thread.
 *   - all tensor pointers are DEVICE pointers obtained from pvhip_malloc, contiguous, fp32 unless
 *     noted; activations are NCHW, convolution weights OIHW, MatMul operands row-major 2-D.
 *   - every kernel is enqueued on the library's single compute stream of the device selected by
 *     pvhip_init (one host thread / process per GPU).
 *   - sizes are element counts (not bytes) unless the name says bytes.
 */
#ifndef PVHIP_H
#define PVHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVHIP_OK            0
#define PVHIP_EHIP         -1   /* a HIP runtime call failed                                  */
#define PVHIP_EINVAL       -2   /* argument rejected on the host (shape / attribute check)    */
#define PVHIP_ENOTINIT     -3   /* pvhip_init has not been called                             */
#define PVHIP_ECOMM        -4   /* RCCL failure / library not loadable                        */
#define PVHIP_EUNSUPPORTED -5   /* configuration outside what the kernels implement           */

#define PVHIP_ABI_VERSION   19

/* ---------------------------------------------------------------- runtime plumbing ---------- */
/* No reference counterpart: the reference computes in host numpy arrays (inference_engine.py:245-256
 * hands ndarray between plugins).  These give plugins a device-resident tensor to hand over instead. */
int         pvhip_abi_version(void);
const char* pvhip_last_error(void);
int         pvhip_device_count(int* count);
int         pvhip_init(int device);                     /* select device, create the compute stream, read the PVHIP_* variables */
int         pvhip_settings_reload(void);                /* read the PVHIP_* environment variables again (they are parsed once, by
                                                           pvhip_init, never on a launch path): tests and tuning scripts that flip one */
int         pvhip_shutdown(void);                       /* free pool, destroy stream                 */
int         pvhip_device_name(char* buf, size_t buflen);
int         pvhip_malloc(void** ptr, size_t bytes);     /* pooled: freed blocks are reused by size   */
int         pvhip_free(void* ptr);                      /* returns the block to the pool             */
int         pvhip_pool_release(void);                   /* hipFree everything cached in the pool     */
int         pvhip_pool_stats(size_t* bytes_in_use, size_t* bytes_cached);
/* Allocation epochs, for forward passes that run on several streams or asynchronously (several requests in flight):
 * blocks allocated between _begin and _dispatched belong to the epoch; one of them that is freed while the epoch is
 * open waits until _end (called once the pass is known to have finished on the device) instead of being handed out
 * again at once; blocks of ended epochs -- the previous outputs a new pass replaces -- are reusable immediately. */
int         pvhip_pool_epoch_begin(int* epoch);
int         pvhip_pool_epoch_dispatched(void);          /* later allocations belong to no epoch */
int         pvhip_pool_epoch_end(int epoch);
int         pvhip_memcpy_h2d(void* dst, const void* src, size_t bytes);  /* Parameter.py:11-13, Const.py:11-13 upload; async w.r.t. device, host buffer reusable on return */
int         pvhip_memcpy_d2h(void* dst, const void* src, size_t bytes);  /* Result.py:17 read-back; SYNCHRONISES the stream */
void*       pvhip_host_alloc(size_t bytes);   /* ABI v16: page-locked host memory for read-backs (NULL when it cannot be had: use pageable memory) */
int         pvhip_host_free(void* p);               /* ABI v17: PVHIP_EINVAL for an address pvhip_host_alloc did not return; pvhip_shutdown frees every block */
int         pvhip_host_stats(size_t* blocks, size_t* bytes);   /* ABI v17: live pvhip_host_alloc blocks and their bytes (no device needed) */
/* ABI v17: the upload of a request's staged input (inference_engine.py InferRequest.input_buffer): on the CURRENT stream, never
 * synchronising.  `src` must lie wholly inside one live pvhip_host_alloc block -- PVHIP_EINVAL for pageable memory, before anything reaches the
 * device -- and stays untouched until the copy has finished (record an event behind it).  Refused while a capture is open. */
int         pvhip_memcpy_h2d_async(void* dst, const void* src, size_t bytes);
int         pvhip_memcpy_d2d(void* dst, const void* src, size_t bytes);
int         pvhip_memset(void* dst, int byte, size_t bytes);
int         pvhip_sync(void);                           /* host-side wait for every compute stream   */

/* Compute streams.  Every launch and copy goes to the CURRENT stream (stream 0 after pvhip_init).  The
 * scheduler may put independent branches of the graph (inference_engine.py:218-242 orders them serially)
 * on up to 8 streams (index 8 is for copies and the RCCL gather of requests in flight) and order them with untimed events; blocks freed while a stream other than 0 has been
 * used are handed out again only after the next full synchronisation (pvhip_sync, or pvhip_memcpy_d2h
 * issued on stream 0). */
#define PVHIP_MAX_STREAMS 9                             /* 8 compute streams + 1 for copies and the gather        */
int         pvhip_stream_select(int index);             /* make stream `index` current (created on first use) */
int         pvhip_stream_wait_event(void* ev);          /* current stream waits for a recorded event  */
int         pvhip_event_create_untimed(void** ev);      /* ordering-only event (no timestamps)        */

/* events on the compute stream: replace the per-node time.time() bracket of inference_engine.py:279-283 */
int         pvhip_event_create(void** ev);
int         pvhip_event_destroy(void* ev);
int         pvhip_event_record(void* ev);
int         pvhip_event_sync(void* ev);
int         pvhip_event_elapsed_ms(void* start, void* stop, float* ms);

/* hipGraph capture of one whole forward pass (the run_tasks loop, inference_engine.py:259-292): between _begin_capture and
 * _end_capture every launch on the current stream -- and on the streams that join it through events -- is recorded instead of
 * executed; pvhip_graph_launch replays the whole pass with one call.  While a capture is open pvhip_malloc must be served
 * by the pool (run the pass eagerly first) and freed blocks stay pinned until pvhip_graph_destroy: the captured kernels hold
 * their addresses.  No host-synchronising call (pvhip_sync, _memcpy_h2d / _d2h) may be made inside a capture.            */
int         pvhip_graph_begin_capture(void);
int         pvhip_graph_capture_status(int* status);    /* current stream: 0 not capturing, 1 capturing, 2 capture invalidated by an illegal call */
int         pvhip_graph_end_capture(void** graph_exec);
int         pvhip_graph_launch(void* graph_exec);
int         pvhip_graph_destroy(void* graph_exec);

/* ---------------------------------------------------------------- streaming elementwise ----- */
/* ReLU.py:9-12  kernel_ReLU_numpy: y = (x < 0) ? 0 : x   (NaN and -0.0 pass through)            */
int pvhip_relu_f32(const float* x, float* y, size_t n);
/* Clamp.py:9-12 kernel_Clamp_numpy: y = min(max(x, lo), hi), NaN propagates                     */
int pvhip_clamp_f32(const float* x, float* y, size_t n, float lo, float hi);
/* Sigmoid.py:10-13 kernel_Sigmoid_numpy: y = 1 / (1 + exp(-x))                                  */
int pvhip_sigmoid_f32(const float* x, float* y, size_t n);

/* Add.py:9-14 kernel_Add_numpy / Multiply.py:9-17 kernel_Multiply_numpy.
 * out = a (op) b with numpy broadcasting already resolved by the caller into element strides:
 * `shape` is the output shape (rank <= PVHIP_MAX_RANK), a_strides/b_strides are element strides of
 * the operands viewed at the output shape (0 on broadcast axes).  The library picks a float4
 * streaming kernel for the common cases (same shape; per-channel (1,C,1,1); trailing-row (1,F);
 * scalar) and a generic strided kernel otherwise.                                               */
#define PVHIP_MAX_RANK 6
int pvhip_add_f32(const float* a, const float* b, float* out, int rank,
                  const int64_t* shape, const int64_t* a_strides, const int64_t* b_strides);
int pvhip_mul_f32(const float* a, const float* b, float* out, int rank,
                  const int64_t* shape, const int64_t* a_strides, const int64_t* b_strides);
/* ABI v19.  Which instantiation and grid a launch of the entries above takes: host-only like the pooling queries further down (no
 * device needed, before pvhip_init too; PVHIP_STREAM_NT / PVHIP_STREAM_WG are honoured), answered by the SAME plan function the launcher
 * switches on.  form[PVHIP_FORM_INTS]; a slot set of its own per family, unused slots 0; kind PVHIP_FORM_NONE (-1) when nothing is launched.
 * pvhip_unary_form(n): unary_f4_kernel<Op, NT, U> over n elements (ReLU, Clamp and Sigmoid share the launcher).                          */
#define PVHIP_UNARY_F4            0   /* unary_f4_kernel                                                                     */
#define PVHIP_UNARY_FORM_KIND     0
#define PVHIP_UNARY_FORM_NT       1   /* nontemporal accesses (the <true, 4> instantiation), else <false, 1>                 */
#define PVHIP_UNARY_FORM_U        2   /* 4 KiB pieces per workgroup and run                                                  */
#define PVHIP_UNARY_FORM_GRID     3   /* workgroups launched                                                                 */
#define PVHIP_UNARY_FORM_RUNS     4   /* 1: at least one whole run of U x 256 float4                                         */
#define PVHIP_UNARY_FORM_REM4     5   /* 1: float4 left behind the last whole run                                            */
#define PVHIP_UNARY_FORM_TAIL     6   /* 1: n % 4 != 0, the scalar tail stores                                               */
#define PVHIP_UNARY_FORM_WRAPS    7   /* 1: more whole runs than workgroups, a workgroup's run loop goes round again         */
int pvhip_unary_form(size_t n, int* form);
/* pvhip_binary_form: the arguments of pvhip_add_f32 / pvhip_mul_f32 without the pointers; commutative = 1 is what both pass (0: the
 * operands of a swapped launch are put back in order, the kSwap instantiations -- reached by the diagnostic build's subtract only). */
#define PVHIP_BINARY_SAME         0   /* binary_same_kernel<Op, NT>: both operands have the output shape                     */
#define PVHIP_BINARY_CHANNEL      1   /* binary_channel_kernel<Op, kSwap>: out as [outer][C][inner], one operand holds C values */
#define PVHIP_BINARY_CHANNEL4     2   /* binary_channel4_kernel<Op, kSwap, NT, U>: the same with inner % 4 == 0 and n % 4 == 0 */
#define PVHIP_BINARY_STRIDED      3   /* binary_strided_kernel: any strides                                                  */
#define PVHIP_BINARY_FORM_KIND    0
#define PVHIP_BINARY_FORM_BCAST   1   /* 0: neither operand is broadcast, 1: the second (b), 2: the first (a): b is streamed */
#define PVHIP_BINARY_FORM_SWAP    2   /* 1: the kSwap instantiation (BCAST == 2 and not commutative)                         */
#define PVHIP_BINARY_FORM_NT      3   /* nontemporal accesses (SAME, CHANNEL4; CHANNEL4 then takes U = 4)                    */
#define PVHIP_BINARY_FORM_C       4   /* CHANNEL, CHANNEL4: values of the broadcast operand                                  */
#define PVHIP_BINARY_FORM_INNER   5   /* CHANNEL, CHANNEL4: elements behind the channel axes                                 */
#define PVHIP_BINARY_FORM_GRID    6   /* workgroups launched                                                                 */
int pvhip_binary_form(int rank, const int64_t* shape, const int64_t* a_strides, const int64_t* b_strides, int commutative, int* form);

/* ---------------------------------------------------------------- pooling / normalisation --- */
/* MaxPool.py:41-72 kernel_MaxPool_numpy: max over the kh x kw window of the ZERO-padded input
 * (pad cells take part with value 0), window clipped at the padded extent.  (oh, ow) are computed
 * by the caller with the rule of MaxPool.py:10-38.                                               */
int pvhip_maxpool2d_f32(const float* x, float* y, int n, int c, int h, int w, int oh, int ow,
                        int kh, int kw, int sh, int sw, int pad_top, int pad_left,
                        int pad_bottom, int pad_right);
/* AvgPool.py:41-59 kernel_AvgPool_numpy: mean of x[y*sh : min(h-1, y*sh+kh), x*sw : min(w-1, x*sw+kw)]
 * -- no padding, window clipped at h-1 / w-1 (reference behaviour, kept).  An empty window yields NaN. */
int pvhip_avgpool2d_f32(const float* x, float* y, int n, int c, int h, int w, int oh, int ow,
                        int kh, int kw, int sh, int sw);
/* SoftMax.py:10-14 kernel_SoftMax_numpy applied per row: y[r,:] = exp(x[r,:]) / sum(exp(x[r,:])),
 * no max subtraction (identical to the reference at batch 1; rows are independent images).      */
int pvhip_softmax_rows_f32(const float* x, float* y, int rows, int cols);
/* LRN.py:10-22 kernel_LRN_numpy: y = x / (bias + alpha * sum_{c' in [c-size/2, c+size/2]} x^2)^beta,
 * window clipped to [0, C); alpha is NOT divided by size.  hw = H*W.                             */
int pvhip_lrn_f32(const float* x, float* y, int n, int c, int hw, int size,
                  float alpha, float beta, float bias);
/* Which kernel form a launch of the four entries above and of pvhip_dwconv2d_f32 takes (an addition to ABI v17).  Host-only like
 * pvhip_conv2d_kernel_kind: no device needed, the PVHIP_* switches are honoured, and the answer comes from the SAME plan function
 * the compute entry switches on.  Each query takes its entry's geometry arguments and fills form[PVHIP_FORM_INTS]; slots a form
 * does not use are 0, and PVHIP_FORM_KIND is PVHIP_FORM_NONE for an empty tensor (nothing is launched).  Returns PVHIP_OK, or
 * what the entry itself would return for these arguments (PVHIP_EINVAL, PVHIP_EUNSUPPORTED).  NOT thread-safe against launches of
 * the same entries from another thread: the 3x3 column planner keeps an unsynchronised cache of plans that both sides use.    */
#define PVHIP_FORM_INTS           16
#define PVHIP_FORM_KIND           0   /* the kernel, ids below                                                              */
#define PVHIP_FORM_G              1   /* (n, c) planes per workgroup / tile                                                 */
#define PVHIP_FORM_BANDS          2   /* bands of output rows per plane (1: whole planes)                                   */
#define PVHIP_FORM_BAND_ROWS      3   /* output rows per band                                                               */
#define PVHIP_FORM_CLIP           4   /* MaxPool, LDS kernels: windows overhang the padded extent (the CLIP instantiation)  */
#define PVHIP_FORM_VEC            5   /* AvgPool / depthwise LDS kernels: 1 when EVERY workgroup starts on a 16-byte boundary
                                         (16-byte staging loads), 0 when some take the scalar loop; LRN: pixels per lane    */
#define PVHIP_FORM_STAGE          6   /* column kernels: outputs leave through the output stage in LDS                      */
#define PVHIP_FORM_NT             7   /* column kernels: nontemporal accesses (PVHIP_STREAM_NT)                             */
#define PVHIP_FORM_S              8   /* column kernels: row segments per output column                                     */
#define PVHIP_FORM_LRN_SIZE       9   /* LRN: the window                                                                    */
#define PVHIP_FORM_LRN_BETA_MODE  10  /* LRN: 0 powf, 1 two square roots (beta 0.75, bias < 1e-20), 2 sqrt (0.5), 3 the
                                         divisor itself (1.0), 4 exp2(-0.75 log2 d) (beta 0.75, bias >= 1e-20)              */
#define PVHIP_FORM_GRID           11  /* LRN, SoftMax: workgroups launched                                                  */
#define PVHIP_FORM_LOOPS          12  /* LRN, SoftMax: 1 when a workgroup's grid-stride loop runs more than once            */
#define PVHIP_FORM_NONE          (-1)
#define PVHIP_MAXPOOL_GLOBAL      0   /* maxpool2d_kernel: one lane per output, windows read from HBM                       */
#define PVHIP_MAXPOOL_LDS         1   /* maxpool2d_lds_kernel<0,0>: run-time window                                         */
#define PVHIP_MAXPOOL_LDS_2X2     2
#define PVHIP_MAXPOOL_LDS_3X3     3
#define PVHIP_MAXPOOL_COLS_S1     4   /* maxpool3x3_cols_kernel, stride 1                                                   */
#define PVHIP_MAXPOOL_COLS_S2     5
#define PVHIP_AVGPOOL_GLOBAL      0   /* avgpool2d_kernel                                                                   */
#define PVHIP_AVGPOOL_LDS         1   /* avgpool2d_lds_kernel: whole planes of at most 16 KB                                */
#define PVHIP_DWCONV_GLOBAL       0   /* dwconv_kernel                                                                      */
#define PVHIP_DWCONV_LDS          1   /* dwconv2d_lds_kernel<0,0>                                                           */
#define PVHIP_DWCONV_LDS_3X3      2
#define PVHIP_DWCONV_COLS_S1      3   /* dwconv3x3_cols_kernel, stride 1                                                    */
#define PVHIP_DWCONV_COLS_S2      4
#define PVHIP_LRN_GENERIC         0   /* lrn_generic_kernel                                                                 */
#define PVHIP_LRN_WINDOW          1   /* lrn_window_kernel<size, vec, beta mode>                                            */
int pvhip_maxpool2d_form(int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh, int sw,
                         int pad_top, int pad_left, int pad_bottom, int pad_right, int* form);
int pvhip_avgpool2d_form(int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh, int sw, int* form);
int pvhip_dwconv2d_form(int n, int g, int h, int wdt, int kh, int kw, int oh, int ow, int sh, int sw,
                        int pad_top, int pad_left, int* form);
int pvhip_lrn_form(int n, int c, int hw, int size, float beta, float bias, int* form);
#define PVHIP_SOFTMAX_ROWS        0   /* softmax_rows_kernel: a workgroup per row, rows beyond the grid in a loop           */
int pvhip_softmax_rows_form(int rows, int cols, int* form);
/* LRN.py:10-22 followed by MaxPool.py:41-72 (3x3 window, stride 1 or 2) as ONE launch: y = maxpool(lrn(x)) with the
 * arithmetic and the pooling rules of the two entries above (bit-identical to calling them in turn); the LRN tensor is
 * never written.  x is (n, c, h, w), y is (n, c, oh, ow).  Covers size == 5, beta == 0.75, c % 8 == 0 and bands of
 * input rows that fit one workgroup; pvhip_lrn_maxpool_supported() (no device needed) tells whether a shape is covered,
 * the compute entry fails with PVHIP_EUNSUPPORTED otherwise.                                                        */
int pvhip_lrn_maxpool_supported(int n, int c, int h, int w, int size, float beta, float bias, int oh, int ow,
                                int kh, int kw, int sh, int sw, int pad_top, int pad_left, int pad_bottom, int pad_right);
int pvhip_lrn_maxpool_f32(const float* x, float* y, int n, int c, int h, int w, int size, float alpha, float beta,
                          float bias, int oh, int ow, int kh, int kw, int sh, int sw, int pad_top, int pad_left,
                          int pad_bottom, int pad_right);
/* The other order, MaxPool.py:41-72 (3x3 window, stride 1 or 2) followed by LRN.py:10-22, as ONE launch: y = lrn(maxpool(x)),
 * bit-identical to calling pvhip_maxpool2d_f32 then pvhip_lrn_f32; the pooled tensor is never written.  x is (n, c, h, w), y is
 * (n, c, oh, ow).  Same coverage as pvhip_lrn_maxpool_f32 (size == 5, beta == 0.75, c % 8 == 0, bands that fit one workgroup).   */
int pvhip_maxpool_lrn_supported(int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh, int sw, int pad_top,
                                int pad_left, int pad_bottom, int pad_right, int size, float beta, float bias);
int pvhip_maxpool_lrn_f32(const float* x, float* y, int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh, int sw,
                          int pad_top, int pad_left, int pad_bottom, int pad_right, int size, float alpha, float beta, float bias);
/* ... and with the 1x1 / stride 1 / unpadded convolution behind the LRN folded in as well (ABI v15; MaxPool.py:41-72, LRN.py:10-22,
 * Convolution.py:57-87 + the fused bias / activation of pvhip_conv2d_f32; GoogLeNet's pool1/3x3_s2 -> pool1/norm1 -> conv2/3x3_reduce): the
 * normalised value a lane would have stored is its column of a k = 1 outer-product MFMA with that channel's weights -- neither the pooled nor
 * the normalised tensor exists.  Rows of a multiple of four pixels, bands of at most 256 pooled outputs, c <= 64, k_out <= 64; w_oihw: the
 * (k_out, c, 1, 1) weights as they are; y: (n, k_out, oh, ow).  The reduction runs over the input channels in ascending order.                */
int pvhip_maxpool_lrn_conv1x1_supported(int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh, int sw, int pad_top,
                                        int pad_left, int pad_bottom, int pad_right, int size, float beta, float bias, int k_out);
int pvhip_maxpool_lrn_conv1x1_f32(const float* x, const float* w_oihw, float* y, int n, int c, int h, int w, int oh, int ow, int kh, int kw,
                                  int sh, int sw, int pad_top, int pad_left, int pad_bottom, int pad_right, int size, float alpha,
                                  float beta, float bias, int k_out, const float* conv_bias, int act, float act_lo, float act_hi);
/* ... and the same without the pooling (an addition to ABI v19), for a tensor x (n, c, hw) that is pooled already -- the second output of
 * pvhip_conv2d_stem_direct_pool_f32: LRN (LRN.py:10-22: five channels, beta = 0.75) then the 1x1 convolution with its bias / activation
 * (Convolution.py:57-87).  A lane owns one pixel and walks the channels; no planes in LDS, no barrier in the loop.  c a multiple of eight and
 * <= 64, k_out <= 64; y: (n, k_out, hw).  The bits of pvhip_lrn_f32 followed by the pointwise convolution.                                       */
int pvhip_lrn_conv1x1_supported(int n, int c, int hw, int size, float beta, float bias, int k_out);
int pvhip_lrn_conv1x1_f32(const float* x, const float* w_oihw, float* y, int n, int c, int hw, int size, float alpha, float beta, float bias,
                          int k_out, const float* conv_bias, int act, float act_lo, float act_hi);

/* ---------------------------------------------------------------- data movement ------------- */
/* Concat.py:9-13 kernel_Concat_numpy: srcs[i] is viewed as [outer][inner[i]] and copied to
 * dst[outer][sum(inner)] at its running offset.  srcs / inner are HOST arrays of n_src entries.  */
#define PVHIP_MAX_CONCAT 16
int pvhip_concat_f32(int n_src, const float* const* srcs, const int64_t* inner, float* dst, int64_t outer);
/* ABI v19.  The copy unit and grid of that launch (host-only; PVHIP_FORM_NONE for an empty output; PVHIP_EINVAL / PVHIP_EUNSUPPORTED
 * as the entry).  Transpose, pad2d and the c8 conversions have one kernel each and no query.                                       */
#define PVHIP_CONCAT_SCALAR       0   /* concat_kernel<float>: some inner[i] is no multiple of 4                              */
#define PVHIP_CONCAT_VEC4         1   /* concat_kernel<float4>                                                               */
#define PVHIP_CONCAT_FORM_KIND    0
#define PVHIP_CONCAT_FORM_GRID_X  1   /* workgroups per source                                                               */
#define PVHIP_CONCAT_FORM_GRID_Y  2   /* sources (zero-length ones included)                                                 */
int pvhip_concat_form(int n_src, const int64_t* inner, int64_t outer, int* form);
/* The zero-padded image Convolution.py:64-66 builds before it slides its window, as a tensor: y (n, c, h + pad_top + pad_bottom,
 * w + pad_left + pad_right) = x (n, c, h, w) with zeros around; channel_add (c floats, may be NULL) is added to every element of x on
 * the way (Add.py:9-14 of a per-channel constant feeding the convolution: one pass instead of two).  The Convolution plugin pads the
 * input of a layer whose channel count is not a multiple of 16 (GoogLeNet conv1) and convolves the result without padding: the
 * kernel's gather then needs no window test (pvhip_conv2d_f32 picks that form whenever no window leaves the tensor).             */
int pvhip_pad2d_f32(const float* x, float* y, int n, int c, int h, int w, int pad_top, int pad_left, int pad_bottom, int pad_right,
                    const float* channel_add);
/* Transpose.py:9-13 kernel_Transpose_numpy, materialised: y = x.transpose(perm), y contiguous.   */
int pvhip_transpose_f32(const float* x, float* y, int rank, const int64_t* in_shape, const int64_t* perm);

/* ---------------------------------------------------------------- MFMA kernels -------------- */
/* MatMul.py:9-17 kernel_MatMul_numpy: C[M,N] = op(A) . op(B); A is stored [M,K] (or [K,M] when
 * trans_a), B is stored [K,N] (or [N,K] when trans_b); fp32 MFMA (v_mfma_f32_32x32x2_f32).        */
int pvhip_matmul_f32(const float* a, const float* b, float* c, int m, int n, int k,
                     int trans_a, int trans_b);
/* ABI v19.  What pvhip_matmul_f32 (f16 = 0) / pvhip_matmul_f16 (f16 = 1) launch for these extents: host-only, answered by the plan
 * function the launcher switches on.  Outputs of fewer than 512 tiles of 64 x 64 split the reduction over grid.z into chunks of a
 * multiple of 16 (at most ceil(k / 64) of them) and sum the partial tiles in split order -- the same bits on every launch.
 * PVHIP_EUNSUPPORTED for m > 65535 * 64, as the entries.                                                                          */
#define PVHIP_MATMUL_MEMSET        0   /* k == 0: the output is zeroed                                                        */
#define PVHIP_MATMUL_SINGLE        1   /* one launch of matmul_kernel                                                         */
#define PVHIP_MATMUL_SPLIT         2   /* matmul_kernel over grid.z = splits into a workspace + matmul_reduce_kernel          */
#define PVHIP_MATMUL_FORM_KIND     0
#define PVHIP_MATMUL_FORM_GRID_X   1   /* tiles along n                                                                       */
#define PVHIP_MATMUL_FORM_GRID_Y   2   /* tiles along m                                                                       */
#define PVHIP_MATMUL_FORM_SPLITS   3
#define PVHIP_MATMUL_FORM_K_CHUNK  4   /* reduction elements per split (a multiple of 16)                                     */
#define PVHIP_MATMUL_FORM_LAST_K   5   /* ... of the last split: k - (splits - 1) * k_chunk                                   */
#define PVHIP_MATMUL_FORM_A_K_FAST 6   /* 1: consecutive lanes stage A along k (its contiguous axis), 0: along m              */
#define PVHIP_MATMUL_FORM_B_N_FAST 7   /* 1: consecutive lanes stage B along n, 0: along k                                    */
#define PVHIP_MATMUL_FORM_F16      8   /* 1: operands rounded to fp16 while staged (matmul_kernel<true>)                      */
int pvhip_matmul_form(int m, int n, int k, int trans_a, int trans_b, int f16, int* form);


/* Convolution.py:57-87 im2col + kernel_Convolution_im2col ("special"), as an implicit GEMM:
 *   y[n,k,oy,ox] = sum_{c,r,s} xpad[n,c,oy*sh+r,ox*sw+s] * w[k,c,r,s]      (dilation ignored, as :72-87 does)
 * Step 1 (once per weight tensor and input extent h x w): repack OIHW weights to the K-major panel the
 *   kernel streams and build the per-reduction-row gather table (byte offset of (c, r, s) in an h x w
 *   image).  wpack must hold pvhip_conv2d_pack_elems(k_out, c, kh, kw) floats.
 * Step 2: the convolution proper.  (oh, ow) computed by the caller per Convolution.py:21-49.
 *   bias (optional, may be NULL): per-output-channel value added in the epilogue; relu == 1 applies the
 *   ReLU.py:11 rule, relu == 2 the Clamp.py:11 rule with [act_lo, act_hi] (fused Convolution->Add->ReLU/Clamp).
 *   out_channels_total > 0: y points at a tensor [n, out_channels_total, oh, ow] and this convolution
 *   writes channels [out_channel_offset, out_channel_offset + k_out) of it -- the Concat.py:9-13 copy of an
 *   inception output done by the producer; 0 = y is the dense [n, k_out, oh, ow] result.            */
size_t pvhip_conv2d_pack_elems(int k_out, int c, int kh, int kw);
int    pvhip_conv2d_pack_f32(const float* w_oihw, float* wpack, int k_out, int c, int kh, int kw, int h, int w);
int    pvhip_conv2d_f32(const float* x, const float* wpack, float* y,
                        int n, int c, int h, int w, int k_out, int kh, int kw, int oh, int ow,
                        int sh, int sw, int pad_top, int pad_left,
                        const float* bias, int relu,
                        int out_channel_offset, int out_channels_total,
                        float act_lo, float act_hi);
/* Which kernel family pvhip_conv2d_f32 dispatches this geometry to (no device needed; honours the PVHIP_* switches): the
 * benchmark's roofline needs it, because the Winograd families execute a fraction of the algorithmic multiplies on the
 * matrix cores -- F(2x2,3x3) 16/36, F(4x4,3x3) 36/144, F(2x2,5x5) 36/100 -- and the direct families all of them.         */
#define PVHIP_CONV_KIND_IGEMM        0   /* implicit GEMM, LDS-DMA tiles (pvhip_conv.hip)                    */
#define PVHIP_CONV_KIND_POINTWISE    1   /* 1x1 / stride 1: fragment-ordered weights (pvhip_pw.hip)          */
#define PVHIP_CONV_KIND_WINO_F2_3X3  2
#define PVHIP_CONV_KIND_WINO_F4_3X3  3
#define PVHIP_CONV_KIND_WINO_F2_5X5  4
#define PVHIP_CONV_KIND_STEM         5   /* ABI v15: 7x7 / 2 over three channels from row spans (pvhip_stem.hip)  */
#define PVHIP_CONV_KIND_STEM_WINO    6   /* ABI v16: the same layer as Winograd F(3x3,4x4) on the space-to-depth image  */
int    pvhip_conv2d_kernel_kind(int n, int c, int h, int w, int k_out, int kh, int kw, int oh, int ow,
                                int sh, int sw, int pad_top, int pad_left);
/* ABI v18.  Which kernel FORM inside its family a convolution launch takes: host-only like pvhip_conv2d_kernel_kind (no device needed, the
 * PVHIP_* switches are honoured), answered by the SAME plan functions the launchers switch on (plan_pw, plan_tiles, plan_wino, plan_wino4).
 * entry PVHIP_CONV_ENTRY_F32: what pvhip_conv2d_f32 launches for this geometry, and what pvhip_conv2d_multi_f32 launches on its pointwise
 * route; PVHIP_CONV_ENTRY_F16_DMA: what pvhip_conv2d_f16_dma / pvhip_conv2d_multi_f16_dma launch.  For a multi-destination launch k_out is
 * the panel width: the sum of the members' channel counts, each rounded up to 32.  Fills form[PVHIP_FORM_INTS] with the slots below (a set
 * of its own: slots 2.. are read by family; unused slots are 0); PVHIP_CONV_FORM_KIND is PVHIP_FORM_NONE for an empty output (nothing is
 * launched).  Returns PVHIP_OK, or what the entry would return for these arguments: PVHIP_EINVAL, PVHIP_EUNSUPPORTED (kh / kw >= 256, an
 * input of 2^29 or an output of 2^31 elements and more, a window of 64 taps and more on the f16 entry).
 * Not reported: the stem entries (pvhip_conv2d_stem_*, pvhip_conv2d_f16_stem*), the span / c8 / c8-multi readers, the MaxPool + 1x1
 * launches, the fp32 multi launch with PVHIP_CONV_POINTWISE=0 (PVHIP_CONV_MULTI_BM), and the diagnostic build's overrides and ablations. */
#define PVHIP_CONV_ENTRY_F32             0
#define PVHIP_CONV_ENTRY_F16_DMA         1
#define PVHIP_CONV_FORM_KIND             0   /* every family: PVHIP_CONV_KIND_* (the f16 entry: PVHIP_CONV_KIND_IGEMM)                   */
#define PVHIP_CONV_FORM_GRID             1   /* every family: workgroups launched                                                        */
#define PVHIP_CONV_FORM_PW_TN            2   /* pointwise: 32-channel tiles per workgroup (1, 2; 4 under PVHIP_PW_TN)                     */
#define PVHIP_CONV_FORM_PW_VEC           3   /* pointwise: 1 = 16-byte copies (h * w a multiple of 4), 0 = dword copies                  */
#define PVHIP_CONV_FORM_PW_NCHUNK        4   /* pointwise: groups of tn channel tiles                                                    */
#define PVHIP_CONV_FORM_PW_STAGGER       5   /* pointwise: 1 when the workgroups start staggered (PVHIP_PW_STAGGER, large grids only)    */
#define PVHIP_CONV_FORM_IGEMM_BM         2   /* implicit GEMM: output channels per tile (fp32: 32 / 64; f16: 32 / 64 / 128)              */
#define PVHIP_CONV_FORM_IGEMM_KERNEL     3   /* implicit GEMM: PVHIP_IGEMM_* below                                                       */
#define PVHIP_CONV_FORM_IGEMM_N_MTILES   4   /* implicit GEMM: channel tiles (GRID = N_MTILES x ceil(pixels / 128))                      */
#define PVHIP_CONV_FORM_WINO_KB          2   /* F(2x2,3x3): output channels per workgroup (64 / 32)                                      */
#define PVHIP_CONV_FORM_WINO_PATCHES     3   /* F(2x2,3x3): patches per workgroup (32 / 64)                                              */
#define PVHIP_CONV_FORM_WINO_WAVES       4   /* F(2x2,3x3): waves per workgroup (4 / 8)                                                  */
#define PVHIP_CONV_FORM_WINO4_M          2   /* six-point: 4 = F(4x4,3x3), 2 = F(2x2,5x5)                                                */
#define PVHIP_CONV_FORM_WINO4_RAGGED     3   /* six-point: an extent is no multiple of m (the RAGGED instantiation)                      */
#define PVHIP_CONV_FORM_WINO4_SHARED     4   /* six-point: 1 = conv_wino4s_kernel (shared V), 0 = conv_wino4_kernel (persistent)         */
#define PVHIP_CONV_FORM_WINO4_ORDER      5   /* six-point: s_order (1: channel-pair-major tile order of the shared-V form)                */
#define PVHIP_CONV_FORM_WINO4_TILES      6   /* six-point: n_tiles (persistent: patch blocks x channel blocks; shared V: x block pairs)   */
#define PVHIP_CONV_FORM_WINO4_WALK       7   /* six-point: 1 when n_tiles exceeds the grid: a workgroup takes more than one tile         */
#define PVHIP_IGEMM_REGISTER             0   /* conv_igemm_kernel: register-staged, windows of 64 taps and more (fp32 only)              */
#define PVHIP_IGEMM_POINTWISE_COPY       1   /* conv_igemm_dma_kernel<.., kPW>: 1x1 / stride 1 / unpadded, whole pixel quads             */
#define PVHIP_IGEMM_RS_MAJOR             2   /* ... (r,s)-major reduction (C a multiple of 16)                                           */
#define PVHIP_IGEMM_C_MAJOR_VALID        3   /* ... c-major, no window leaves the tensor: no window test                                 */
#define PVHIP_IGEMM_C_MAJOR_WINDOW       4   /* ... c-major with the window test                                                         */
int    pvhip_conv2d_form(int entry, int n, int c, int h, int w, int k_out, int kh, int kw, int oh, int ow,
                         int sh, int sw, int pad_top, int pad_left, int* form);
/* MaxPool.py:41-72 (3x3 window, stride 1, pad 1 all round: output extent = input extent) followed by a 1x1 / stride 1 / unpadded
 * Convolution.py:57-87, as one launch: y = conv1x1(maxpool(x)); the pooled tensor is never written.  Bit-identical to
 * pvhip_maxpool2d_f32 followed by pvhip_conv2d_f32.  x is (n, c, h, w); wpack the pvhip_conv2d_pack_f32 panel of the (k_out, c, 1, 1)
 * weights; bias / act / out_channel_offset / out_channels_total / act_lo / act_hi as for pvhip_conv2d_f32.  Covers c % 16 == 0,
 * even w, k_out <= 128 (pvhip_conv2d_pooled_supported; no device needed); PVHIP_EUNSUPPORTED otherwise.                           */
int    pvhip_conv2d_pooled_supported(int n, int c, int h, int w, int k_out);
int    pvhip_conv2d_pooled_f32(const float* x, const float* wpack, float* y, int n, int c, int h, int w, int k_out,
                               const float* bias, int act, int out_channel_offset, int out_channels_total,
                               float act_lo, float act_hi);
/* The same pair for an FP16 IR read with fp16_as_fp32=False (ABI v13): the window maximum in fp32, then both operands rounded to fp16 as
 * they are read from LDS, fp32 accumulation on v_mfma_f32_32x32x16_f16 -- what pvhip_maxpool2d_f32 followed by pvhip_conv2d_f16_dma does. */
int    pvhip_conv2d_pooled_f16(const float* x, const float* wpack, float* y, int n, int c, int h, int w, int k_out,
                               const float* bias, int act, int out_channel_offset, int out_channels_total,
                               float act_lo, float act_hi);
/* Several Convolution.py:149-176 calls that share their input (the 1x1, 3x3_reduce and 5x5_reduce arms of an inception
 * module) as ONE launch: the input is read once and the small arms ride in the big one's grid.  Only 1x1 / stride 1 /
 * unpadded convolutions with c % 16 == 0 (pvhip_conv2d_multi_supported; no device needed).  wpack is the panel of
 * pvhip_conv2d_pack_f32 for the (k_panel, c, 1, 1) weight tensor that holds the convolutions' OIHW weights one after
 * the other, each padded with zero rows to a multiple of 32 output channels (k_panel = sum of the padded counts); bias
 * (k_panel values, optional) and act / act_lo / act_hi as for pvhip_conv2d_f32, shared by all.  dests[i] says where
 * convolution i stores: y (an (n, k, oh, ow) tensor, or with channels_total > 0 the (n, channels_total, oh, ow) tensor
 * whose channels [channel_offset, channel_offset + k) it fills).  Every output carries the bits of its own
 * pvhip_conv2d_f32 call.                                                                                            */
#define PVHIP_MAX_CONV_DESTS 6
typedef struct pvhip_conv_dest {
    float* y;           /* (layout 1: an fp16 tensor behind a float pointer) */
    int    k;
    int    channel_offset;
    int    channels_total;
    int    layout;          /* ABI v14.  0: fp32 NCHW, as above.  1 (pvhip_conv2d_multi_f16_dma only; channels_total = 0; act none or ReLU):
                             * y is an fp16 tensor with the channels blocked by eight, [n][ceil16(k) / 8][oh * ow][8 halves]
                             * (pvhip_c8_f16_elems floats), the input format of pvhip_conv2d_f16_c8: what the reference's float16
                             * tensor of this node holds (common_def.py:13-17), channels past k up to a whole 16 are zeros.           */
} pvhip_conv_dest;
int    pvhip_conv2d_multi_supported(int c, int kh, int kw, int sh, int sw, int pad_top, int pad_left, int n_dest);
int    pvhip_conv2d_multi_f32(const float* x, const float* wpack, int n, int c, int h, int w, int kh, int kw,
                              int oh, int ow, int sh, int sw, int pad_top, int pad_left,
                              const float* bias, int act, float act_lo, float act_hi,
                              int n_dest, const pvhip_conv_dest* dests);
/* The same launch for an FP16 IR read with fp16_as_fp32=False (ABI v13): the f16 form of the LDS-DMA kernel (pvhip_conv2d_f16_dma) over
 * the members' panel -- the module input is read once, operands rounded to fp16 as they are read from LDS, fp32 accumulation.          */
int    pvhip_conv2d_multi_f16_dma(const float* x, const float* wpack, int n, int c, int h, int w, int kh, int kw,
                                  int oh, int ow, int sh, int sw, int pad_top, int pad_left,
                                  const float* bias, int act, float act_lo, float act_hi,
                                  int n_dest, const pvhip_conv_dest* dests);

/* ---- FP16 IRs.  The reference runs an FP16 IR in numpy float16 (common_def.py:13-17; Convolution.py:57-87 and
 * MatMul.py:9-17 then multiply AND accumulate in float16).  These entries take the same fp32 device tensors as their _f32
 * twins, round both operands to fp16 (round to nearest even; the constants of an FP16 IR are fp16 values already) and
 * accumulate in fp32 on the f16 matrix-core instructions (v_mfma_f32_32x32x16_f16, 16x the fp32 MFMA rate).  The engine
 * selects them only for an FP16 IR read with fp16_as_fp32=False.  pvhip_conv2d_f16_pack_elems counts FLOATS of wpack.    */
size_t pvhip_conv2d_f16_pack_elems(int k_out, int c, int kh, int kw);
int    pvhip_conv2d_f16_pack(const float* w_oihw, float* wpack, int k_out, int c, int kh, int kw, int h, int w);
int    pvhip_conv2d_f16(const float* x, const float* wpack, float* y,
                        int n, int c, int h, int w, int k_out, int kh, int kw, int oh, int ow,
                        int sh, int sw, int pad_top, int pad_left,
                        const float* bias, int act,
                        int out_channel_offset, int out_channels_total,
                        float act_lo, float act_hi);
/* The second f16 kernel (ABI v13): layers whose channel count is a multiple of 16 (every GoogLeNet layer but conv1) on the LDS-DMA
 * kernel of pvhip_conv2d_f32 -- the SAME fp32 tiles reach LDS by the same copies, wpack is the fp32 panel of pvhip_conv2d_pack_f32 --
 * with a stage of 16 channels as ONE v_mfma_f32_32x32x16_f16 per 32-channel tile (operands rounded to fp16 as they are read from LDS,
 * fp32 accumulation): 1/16 of the matrix-core cycles, no register-staged gather.  Same arithmetic as pvhip_conv2d_f16 in another
 * summation order ((r,s)-major).  _supported: C % 16 == 0 and a window of fewer than 64 taps.                                    */
int    pvhip_conv2d_f16_dma_supported(int c, int kh, int kw);
int    pvhip_conv2d_f16_dma(const float* x, const float* wpack, float* y,
                            int n, int c, int h, int w, int k_out, int kh, int kw, int oh, int ow,
                            int sh, int sw, int pad_top, int pad_left,
                            const float* bias, int act,
                            int out_channel_offset, int out_channels_total,
                            float act_lo, float act_hi);
/* The third f16 kernel (ABI v13): stride-1 "same" windows (1x1; 3x3 / pad 1; 5x5 / pad 2) with C % 16 == 0 and rows short enough that
 * a 128-pixel tile and its halo are one 1-KiB span per channel (128 + 2 * pad * (w + 1) + 3 <= 256 floats: every GoogLeNet layer but
 * conv1).  A workgroup copies ONE span per channel and stage into LDS and serves every tap and up to 128 output channels from it (no
 * copy per tap, none per channel tile); the weights are fp16 MFMA fragments packed once by _span_pack (wf: _span_pack_elems FLOATS).
 * Operands rounded to fp16 as they are read, fp32 accumulation; arguments as pvhip_conv2d_f32.                                     */
int    pvhip_conv2d_f16_span_supported(int c, int h, int w, int kh, int kw, int sh, int sw, int pad_top, int pad_left, int oh, int ow);
size_t pvhip_conv2d_f16_span_pack_elems(int k_out, int c, int kh, int kw);
int    pvhip_conv2d_f16_span_pack(const float* w_oihw, float* wf, int k_out, int c, int kh, int kw);
int    pvhip_conv2d_f16_span(const float* x, const float* wf, float* y,
                             int n, int c, int h, int w, int k_out, int kh, int kw, int oh, int ow,
                             int sh, int sw, int pad_top, int pad_left,
                             const float* bias, int act,
                             int out_channel_offset, int out_channels_total,
                             float act_lo, float act_hi);
int    pvhip_matmul_f16(const float* a, const float* b, float* c, int m, int n, int k,
                        int trans_a, int trans_b);
/* The fourth f16 kernel (ABI v14) and the first fp16 TENSORS in HBM: the 3x3_reduce / 5x5_reduce convolutions of an FP16 IR hand
 * their output to the 3x3 / 5x5 convolution behind them as fp16 with the channels blocked by eight ("c8": [n][ceil16(c) / 8][h * w][8],
 * the eight channels of a pixel = one 16-byte MFMA operand; written by pvhip_conv2d_multi_f16_dma through pvhip_conv_dest.layout = 1).
 * pvhip_conv2d_f16_c8 reads it: stride-1 "same" windows (1x1; 3x3 / pad 1; 5x5 / pad 2) over rows of at most 64 - 2 pad pixels, any c
 * (padded to whole 16-channel stages with zero weights), fp32 NCHW output with bias / activation / channel offset as pvhip_conv2d_f32.
 * A producer wave copies whole input rows into LDS (the zero padding is the out-of-range rule of the copy), four consumer waves own a
 * 32-channel tile each.  wf: fragments packed by _c8_pack (_c8_pack_elems FLOATS).  _from_f32 / _to_f32 convert between NCHW fp32 and
 * c8 fp16 (round to nearest even): the boundary of the layout for any other reader, and the tests.                                    */
size_t pvhip_c8_f16_elems(int n, int c, int h, int w);
int    pvhip_c8_f16_from_f32(const float* x, void* xb, int n, int c, int h, int w);
int    pvhip_c8_f16_to_f32(const void* xb, float* x, int n, int c, int h, int w);
int    pvhip_conv2d_f16_c8_supported(int c, int h, int w, int kh, int kw, int sh, int sw, int pad_top, int pad_left, int oh, int ow);
size_t pvhip_conv2d_f16_c8_pack_elems(int k_out, int c, int kh, int kw);
int    pvhip_conv2d_f16_c8_pack(const float* w_oihw, float* wf, int k_out, int c, int kh, int kw);
/* The module form (ABI v14): one or several 1x1 convolutions of the same c8 input as one launch (n_dest members; wf: _c8_pack of the
 * members' weights laid one after the other, each padded with zero rows to a multiple of 32 output channels, bias likewise), a 1x1
 * convolution behind a 3x3 / stride 1 / pad 1 MaxPool (pool = 1: MaxPool.py:41-72 then Convolution.py:57-87, the pooled tensor never
 * exists), or one 3x3 / 5x5 convolution.  dests[i].layout: 0 = fp32 NCHW (y, channel_offset, channels_total as pvhip_conv2d_multi_f32),
 * 1 = fp16 c8: a tensor of its own (channels_total = 0: [n][ceil16(k) / 8][h * w][8], zeros past k) or channels [channel_offset,
 * channel_offset + k) of a c8 tensor of channels_total channels (the module's Concat buffer: k and the offset multiples of 8, the
 * total a multiple of 16).  pvhip_maxpool3x3_c8: MaxPool.py:41-72 for a 3x3 window on a c8 tensor (any stride, zero padding, the
 * window clipped at the padded edge; a NaN wins), c8 output.                                                                     */
int    pvhip_conv2d_f16_c8_multi_supported(int c, int h, int w, int kh, int kw, int pool, int n_dest);
int    pvhip_conv2d_f16_c8_multi(const void* xb, const float* wf, int n, int c, int h, int w, int kh, int kw, int pool,
                                 const float* bias, int act, float act_lo, float act_hi,
                                 int n_dest, const pvhip_conv_dest* dests);
int    pvhip_maxpool3x3_c8(const void* x, void* y, int n, int c, int h, int w, int oh, int ow, int sh, int sw,
                           int pad_top, int pad_left, int pad_bottom, int pad_right);
/* The stem of an FP16 IR on blocked fp16 tensors (ABI v14): pvhip_conv2d_f16_dma_c8 = pvhip_conv2d_f16_dma with the output stored as fp16 c8
 * ([n][ceil16(k_out) / 8][oh * ow][8]; act none or ReLU); pvhip_maxpool3x3_lrn_c8 = MaxPool 3x3 (MaxPool.py:41-72) followed by LRN over
 * five channels (LRN.py:10-22) on a c8 tensor as one launch, c8 output.                                                            */
int    pvhip_conv2d_f16_dma_c8(const float* x, const float* wpack, void* yb,
                               int n, int c, int h, int w, int k_out, int kh, int kw, int oh, int ow,
                               int sh, int sw, int pad_top, int pad_left, const float* bias, int act);
int    pvhip_maxpool3x3_lrn_c8(const void* x, void* y, int n, int c, int h, int w, int oh, int ow, int sh, int sw,
                               int pad_top, int pad_left, int pad_bottom, int pad_right,
                               int size, float alpha, float beta, float bias);
/* ... with the 1x1 / stride 1 / unpadded convolution behind the LRN in the same launch (ABI v15; the FP16-IR twin of pvhip_maxpool_lrn_conv1x1_f32:
 * fp16 operands on v_mfma_f32_32x32x4_2b_f16, fp32 accumulation).  x: c8 (n, c, h, w), c <= 64; w_oihw: the (k_out, c, 1, 1) fp32 weights, rounded to
 * fp16 as they are staged; k_out <= 64; y: c8 (n, k_out, oh, ow); conv_bias may be NULL; act: none or ReLU.                                   */
int    pvhip_maxpool3x3_lrn_conv1x1_c8_supported(int c, int k_out, int size);
int    pvhip_maxpool3x3_lrn_conv1x1_c8(const void* x, const float* w_oihw, void* y, int n, int c, int h, int w, int oh, int ow, int sh, int sw,
                                       int pad_top, int pad_left, int pad_bottom, int pad_right, int size, float alpha, float beta, float bias,
                                       int k_out, const float* conv_bias, int act);
/* The first convolution of an image network as an FP16 layer, from row spans (ABI v14): 7x7 / stride 2 / pad 3 over three channels, at most 64
 * output channels (GoogLeNet's conv1).  _supported: 0, or the floats per row the padded input must have (w + 3 rounded up so that every
 * tap of the last output column exists, whole 16-byte pieces); xp: that padded input (n, 3, hp, wp), e.g. from pvhip_pad2d_f32 with
 * pad_top = pad_left = 3, pad_bottom = 3, pad_right = wp - w - 3 (and the per-channel constant of a folded Add); wf: _stem_pack of the
 * (k_out, 3, 7, 7) weights (_stem_pack_elems FLOATS); yb: fp16 c8 output (n, k_out, oh, ow); act: none or ReLU.                        */
int    pvhip_conv2d_f16_stem_supported(int c, int h, int w, int k_out, int kh, int kw, int sh, int sw, int pad_top, int pad_left, int oh, int ow);
size_t pvhip_conv2d_f16_stem_pack_elems(int k_out);
int    pvhip_conv2d_f16_stem_pack(const float* w_oihw, float* wf, int k_out);
int    pvhip_conv2d_f16_stem(const float* xp, const float* wf, void* yb, int n, int hp, int wp, int k_out, int oh, int ow,
                             const float* bias, int act);
/* ... and straight from the UNPADDED image (ABI v15; as pvhip_conv2d_stem_direct_f32: w % 4 == 0, w <= 248; no padding pass; pre_add: the per-channel
 * constant of an Add in front of the layer, or NULL); wf from _direct_pack (the k slots of a filter row start one column in front of the window). */
int    pvhip_conv2d_f16_stem_direct_supported(int c, int h, int w, int k_out, int kh, int kw, int sh, int sw, int pad_top, int pad_left, int oh, int ow);
int    pvhip_conv2d_f16_stem_direct_pack(const float* w_oihw, float* wf, int k_out);
int    pvhip_conv2d_f16_stem_direct(const float* x, const float* wf, void* yb, int n, int h, int w, int k_out, int oh, int ow,
                                    const float* pre_add, const float* bias, int act);
/* The same first convolution in fp32 (ABI v15; Convolution.py:57-87: 7x7 / stride 2 / pad 3 over three channels, at most 64 output channels, output
 * rows of at most 112 pixels and a multiple of four -- GoogLeNet's conv1): from row spans of the padded image, the whole weight tensor resident in
 * registers, no vector instruction in the reduction loop; the reduction runs over the taps in the reference's own (c, r, s) order.  _supported: 0,
 * or the floats per row the padded input must have (as pvhip_conv2d_f16_stem_supported); xp: that padded input (n, 3, hp, wp) with
 * hp >= 2 (oh - 1) + 7, from pvhip_pad2d_f32; wf: _pack of the (k_out, 3, 7, 7) weights (_pack_elems floats); y: (n, k_out, oh, ow) fp32;
 * bias / act / act_lo / act_hi as pvhip_conv2d_f32.  pvhip_conv2d_kernel_kind answers PVHIP_CONV_KIND_STEM for such a layer
 * (PVHIP_CONV_STEM=0: never).                                                                                                       */
int    pvhip_conv2d_stem_f32_supported(int c, int h, int w, int k_out, int kh, int kw, int sh, int sw, int pad_top, int pad_left, int oh, int ow);
size_t pvhip_conv2d_stem_f32_pack_elems(int k_out);
int    pvhip_conv2d_stem_f32_pack(const float* w_oihw, float* wf, int k_out);
int    pvhip_conv2d_stem_f32(const float* xp, const float* wf, float* y, int n, int hp, int wp, int k_out, int oh, int ow,
                             const float* bias, int act, float act_lo, float act_hi);
/* ... and straight from the UNPADDED image x (n, 3, h, w) where w % 4 == 0 and w <= 248 (_direct_supported: 1 / 0): no padding pass at all -- the
 * zero padding is where the copies land in LDS plus out-of-range lanes and rows; pre_add: one fp32 constant per input channel added to the image
 * (not to its padding) on the way, or NULL: the Add of a per-channel Const in front of the layer (Add.py:9-14; GoogLeNet's data/mean).           */
int    pvhip_conv2d_stem_direct_supported(int c, int h, int w, int k_out, int kh, int kw, int sh, int sw, int pad_top, int pad_left, int oh, int ow);
int    pvhip_conv2d_stem_direct_f32(const float* x, const float* wf, float* y, int n, int h, int w, int k_out, int oh, int ow,
                                    const float* pre_add, const float* bias, int act, float act_lo, float act_hi);
/* ... with a SECOND output (an addition to ABI v19): yp (n, k_out, poh, pow) = the 3x3 / stride 2 / unpadded / ceil-rounded MaxPool of y (MaxPool.py:41-72:
 * the window clipped at the extent, a NaN is the maximum; GoogLeNet's pool1/3x3_s2), taken where conv1's values already are.  y keeps the bits of
 * pvhip_conv2d_stem_direct_f32 (Convolution.py:57-87), yp has the bits of pvhip_maxpool2d_f32 on y, whatever the grid.  _supported (1 / 0): the layer
 * is the direct form's, oh >= 3, poh = (oh - 2) / 2 + 1, pow = ow / 2, and -- the size rule, for n > 0 -- every CU walks at least eight tiles of four
 * output rows (n = 0 asks for the shape alone; the entry takes every n of a supported shape).                                                     */
int    pvhip_conv2d_stem_direct_pool_supported(int n, int c, int h, int w, int k_out, int kh, int kw, int sh, int sw, int pad_top, int pad_left,
                                               int oh, int ow, int poh, int pow);
int    pvhip_conv2d_stem_direct_pool_f32(const float* x, const float* wf, float* y, float* yp, int n, int h, int w, int k_out, int oh, int ow,
                                         int poh, int pow, const float* pre_add, const float* bias, int act, float act_lo, float act_hi);
/* The same first convolution as WINOGRAD F(3x3, 4x4) on the space-to-depth image (ABI v16; Convolution.py:57-87 for a 7x7 / stride 2 / pad 3 layer
 * over three channels): x'(c; py, px; i, j) = xpad(c, 2 i + py, 2 j + px) turns it into a 4x4 / stride 1 convolution over 12 channels, which
 * 6x6-point tiles (the interpolation points of the F(4x4,3x3) / F(2x2,5x5) kernels) compute with 0.34 of the multiplies.  x: the UNPADDED
 * (n, 3, h, w) fp32 image, h even, w % 4 == 0, w <= 224; oh = h / 2, ow = w / 2; k_out <= 64 and a multiple of 16; u: pvhip_conv2d_stem_wino_pack's transformed weights
 * (pvhip_conv2d_stem_wino_pack_elems floats); pre_add / bias / act as pvhip_conv2d_stem_direct_f32.  NOT the bits of pvhip_conv2d_f32 (another
 * order of summation): the tolerance of the other Winograd forms.  OPT-IN: pvhip_conv2d_kernel_kind answers PVHIP_CONV_KIND_STEM_WINO only with
 * PVHIP_CONV_STEM_WINO=1 (measured at batch 256: 0.50 ms against the row-span kernel's 0.56, at 0.26 of the fp32 MFMA peak on executed flops).    */
int    pvhip_conv2d_stem_wino_supported(int c, int h, int w, int k_out, int kh, int kw, int sh, int sw, int pad_top, int pad_left, int oh, int ow);
long   pvhip_conv2d_stem_wino_pack_elems(void);
int    pvhip_conv2d_stem_wino_pack(const float* w_oihw, float* u, int k_out);
int    pvhip_conv2d_stem_wino_f32(const float* x, const float* u, float* y, int n, int h, int w, int k_out, int oh, int ow,
                                  const float* pre_add, const float* bias, int act, float act_lo, float act_hi);
/* AvgPool.py:41-59 on a c8 tensor (the window rule of pvhip_avgpool2d_f32); the output is fp32 NCHW holding fp16 values (the mean in fp32,
 * rounded once: the reference's AvgPool of a float16 tensor returns float16). */
int    pvhip_avgpool_c8(const void* x, float* y, int n, int c, int h, int w, int oh, int ow, int kh, int kw, int sh, int sw);
/* ... and the other order: LRN over five channels followed by MaxPool 3x3 on a c8 tensor as one launch (LRN.py:10-22 then MaxPool.py:41-72;
 * the LRN tensor never exists).  _supported: pooled rows per workgroup (0: outside the kernel).                                        */
int    pvhip_lrn_maxpool3x3_c8_supported(int h, int w, int oh, int ow, int sh, int sw, int pad_top, int pad_left, int size);
int    pvhip_lrn_maxpool3x3_c8(const void* x, void* y, int n, int c, int h, int w, int size, float alpha, float beta, float bias,
                               int oh, int ow, int sh, int sw, int pad_top, int pad_left, int pad_bottom, int pad_right);
int    pvhip_conv2d_f16_c8(const void* xb, const float* wf, float* y,
                           int n, int c, int h, int w, int k_out, int kh, int kw,
                           const float* bias, int act,
                           int out_channel_offset, int out_channels_total,
                           float act_lo, float act_hi);

/* GroupConvolution.py:53-79 kernel_GroupConvolution_numpy, depthwise case only (weights
 * [G,1,1,kh,kw], one input and one output channel per group), applied to every image.  bias / act /
 * act_lo / act_hi: optional fused Add(per-channel Const) and ReLU (1) or Clamp (2), as for pvhip_conv2d_f32. */
int pvhip_dwconv2d_f32(const float* x, const float* w, float* y, int n, int g, int h, int wdt,
                       int kh, int kw, int oh, int ow, int sh, int sw, int pad_top, int pad_left,
                       const float* bias, int act, float act_lo, float act_hi);

/* ---------------------------------------------------------------- SSD head ------------------ */
/* DetectionOutput.py:163-259 kernel_DetectionOutput_naive with its helpers iou (:12-34), nms (:38-63),
 * screen_out_prior_boxes (:69-97), decode_bboxes (:100-150), clip_bounding_boxes (:153-158); share_location and
 * normalized boxes, as the reference asserts.  loc [n][P*4], conf [n][P*C], priors [1][2][P*4] (boxes, variances),
 * out [n*records][7] = [rank, class, score, xmin, ymin, xmax, ymax] in descending score order per image, a
 * [-1,0,..] terminator after the last record, zeros after it.  The reference handles n == 1 only; images are
 * independent here.  code_type_center_size: 1 = caffe.PriorBoxParameter.CENTER_SIZE, 0 = CORNER.
 * NaN: a prior with a NaN among its num_classes scores is never a candidate, whatever its other scores (the reference's argsort
 * picks the NaN as the best score and NaN > threshold is false); a +inf best score is kept and ranks first.  A NaN in loc or in a prior
 * box gives a box whose IoU with any other is NaN or 0, never above the threshold: it suppresses nothing, is not suppressed and is stored
 * as it is.  num_priors: at most 11498 (13 bytes of LDS per prior + 4116 within 150 KB), else PVHIP_EUNSUPPORTED. */
int pvhip_detection_output_f32(const float* loc, const float* conf, const float* priors, float* out, int n,
                               int num_priors, int num_classes, int records_per_image, float confidence_threshold,
                               float nms_threshold, int code_type_center_size, int variance_encoded_in_target,
                               int clip_before_nms, int clip_after_nms);
/* Addition to ABI v17 (the version number is unchanged: nothing existing changed): the records above become the (id, x, y, w, h) table
 * of the ROI preprocessing entries below, on the device, so that a cascade never reads them on the host.  `records`: images *
 * records_per_image rows of 7 floats, image b being rows [b P, (b + 1) P).  An image's list ends at its first row whose column 0 is not
 * >= 0 (the terminator above; NaN too).  A live row is selected when score >= min_confidence, its four corners are finite and
 * (labels == NULL or) its label equals (float)labels[j] for some j < num_labels <= 64.  Its rectangle over a frame of (frame_h, frame_w):
 * x0 = floor(min(max(xmin * frame_w, 0), frame_w)), x1 = ceil(min(max(xmax * frame_w, 0), frame_w)) in fp32, never contracted, y0 / y1
 * alike with frame_h; it is dropped when x1 - x0 < min_w or y1 - y0 < min_h.  Survivors keep the order (image, position): survivor
 * k < n becomes rois[k] = (b, x0, y0, w, h) with record_of[k] = b P + p; rows k >= count = min(selected, n) are (-1, 0, 0, 0, 0) -- which
 * the ROI entries write as quiet NaN -- with record_of[k] = -1; counts[0] = count, counts[1] = selected (every survivor, which may
 * exceed n).  The same rule in numpy: tests/detected_rois_ref.py, matched integer for integer.  One workgroup on the current stream,
 * no allocation.  n, images, records_per_image, min_h, min_w >= 1, images * records_per_image < 2^31 / 7, frame_h, frame_w in [1, 2^24],
 * `labels` NULL (any label; num_labels == 0) or a device pointer; else PVHIP_EINVAL. */
int pvhip_detections_to_rois(const float* records, int* rois, int* record_of, int* counts, int n, int images, int records_per_image,
                             int frame_h, int frame_w, float min_confidence, const int* labels, int num_labels, int min_h, int min_w);
/* Addition to ABI v18 (the version number is unchanged: nothing existing changed): the same table for a detector whose input was fitted
 * (pvhip_input_preprocess_fit_f32 below): the detector saw the frame in the rectangle [dy, dy + ih) x [dx, dx + iw) of its (net_h, net_w)
 * input.  Each corner is mapped back in fp32, never contracted, three roundings: u = (xmin * (float)net_w - (float)dx) / (float)iw, xmax
 * alike, ymin / ymax with net_h, dy, ih; then the rule above with u in the place of the corner: floor / ceil of the clamped product
 * with the frame extent, min_h / min_w.  The finite check is on the record's own corners.  A box in the padding clamps to the frame's
 * edge; one wholly in the padding has extent 0 and is dropped.  net_h, net_w in [1, 2^24], iw, ih >= 1, dx, dy >= 0, dx + iw <= net_w,
 * dy + ih <= net_h, and the limits above; else PVHIP_EINVAL.  In numpy: tests/letterbox_ref.py. */
int pvhip_detections_to_rois_fit(const float* records, int* rois, int* record_of, int* counts, int n, int images, int records_per_image,
                                 int frame_h, int frame_w, float min_confidence, const int* labels, int num_labels, int min_h, int min_w,
                                 int net_h, int net_w, int dx, int dy, int iw, int ih);

/* ---------------------------------------------------------------- a classifier's answer ---- */
/* Addition to ABI v18 (the version number is unchanged: nothing existing changed): the k best entries of every row of a contiguous
 * (rows, cols) fp32 tensor -- what the reference's sample makes on the host with np.argsort(res[output_node_name][0])[::-1] -- so that
 * only (rows, k) pairs are read back.  For a row x[0..cols) the answer is the first k positions of the row sorted by this total order:
 *   1. NaN (any sign, any payload) ranks before every number: a poisoned row shows NaN as its first score;
 *   2. then by value, descending; +0.0 and -0.0 are equal;
 *   3. equal rank (ties, zeros of either sign, several NaNs): the lower index first.
 * In numpy: np.lexsort((np.arange(cols), -np.where(isnan, 0, x), ~isnan))[:k] (tests/topk_ref.py; matched index for index).  On a row
 * without ties or NaN this is np.argsort(x)[::-1][:k].  indices[r][j] is that position as an int32; values[r][j] holds the bits of
 * x[r][indices[r][j]] unchanged (-0.0 stays -0.0, a NaN keeps its payload).  `indices` and `values` are (rows, k).  One launch on the
 * current stream, no allocation, no workspace.  rows, cols >= 1, 1 <= k <= min(cols, 64), rows * cols < 2^31, no NULL pointer; else
 * PVHIP_EINVAL and nothing is launched. */
int pvhip_topk_rows_f32(const float* x, int rows, int cols, int k, int* indices, float* values);

/* ---------------------------------------------------------------- an embedding network's answer ---- */
/* Addition to ABI v18 (the version number is unchanged: nothing existing changed): the k best rows of a gallery of enrolled embeddings
 * for every row of a contiguous (n, d) fp32 Result -- what a user of a recognition network makes on the host with `gallery @ x.T` and an
 * argpartition -- so that only (n, k) triples are read back and no (n, g) score matrix is written anywhere.  The rule
 * (pyopenvino_amd/gallery.py and tests/gallery_ref.py state the same one, matched bit for bit):
 *   1. norm    of a row v[0..d) of float32: s = the binary64 sum of (double)v[i] * (double)v[i] for i ascending, started from 0.0, one
 *      rounding per addition (the squares are exact in binary64); the row is void when an element is not finite or when s == 0;
 *      r = sqrt(s), correctly rounded binary64.
 *   2. gallery rows, on the host when the gallery is made: under PVHIP_GALLERY_COSINE u[g][i] = (float)((double)v[i] / r); under
 *      PVHIP_GALLERY_DOT u = v, and a row is void only for an element that is not finite.  A gallery has no void row.
 *   3. chain   a[r][g] starts at +0.0f; for i = 0 .. d - 1 in order a = fmaf(x[r][i], u[g][i], a): fp32, one rounding per step,
 *      subnormals kept.  x is the Result's own bits, not normalised.  A chain may end at -0.0 (a negative underflow); a zero of either sign
 *      counts as +0.0 from here on, so the zero padding behind d does not change the answer.
 *   4. order   per row the gallery rows are sorted by a in the total order of pvhip_topk_rows_f32 above: NaN first, then descending,
 *      +0 equal to -0, ties to the lower gallery index; the first k are the candidates.  A chain of finite factors may overflow to an infinity and then stays there: it never holds NaN.
 *   5. score   under PVHIP_GALLERY_DOT score = a; under PVHIP_GALLERY_COSINE score = (float)((double)a / r_row), r_row from 1. on the
 *      query row.  A NaN score is the quiet NaN 0x7FC00000.  Slot j is kept when has_min_score == 0 or score >= min_score (a NaN is not);
 *      counts[r] is the length of the leading run of kept slots; the slots behind it are void: index -1, score the quiet NaN 0x7FC00000.
 *   6. a void query row -- an element that is not finite under either metric, or s == 0 under PVHIP_GALLERY_COSINE -- has count 0 and
 *      every slot void (the quiet-NaN rows behind `count` of a DetectedRois or LandmarkWarps pass are such rows).
 * `x` may be only 4-byte aligned (a Result that starts inside a tensor).  `packed` is the gallery in the matrix cores' operand order,
 * 16-byte aligned: g padded to gp, a multiple of 32, and d to dp, a multiple of 8, with zeros; blocks of 32 gallery rows hold groups of 8
 * consecutive i; in a group lane ((i & 1) << 5) | j holds 4 floats, elements i0 + (i & 1) + 2 t, t = 0..3, of gallery row 32 b + j:
 *     packed[((b * (dp / 8) + i / 8) * 64 + (((i & 1) << 5) | (g & 31))) * 4 + ((i & 7) >> 1)] = u[g][i],   b = g / 32
 * -- the lane's B operand of four consecutive 32x32x2 matrix steps in one 16-byte load, 1 KB contiguous per wave.
 * Two launches on the current stream, no allocation.  Scores: one workgroup per (4 chunks of PVHIP_GALLERY_CHUNK gallery rows, block of 32
 * query rows), the blocks of one gallery piece side by side on one XCD; the query block is copied once into LDS (32 * dp * 4 bytes: d <= 1024), rows >= n and void rows zero-filled; each wave
 * walks the 32-row blocks of its chunk with v_mfma_f32_32x32x2_f32, i in order, one accumulator tile per block -- bit for bit the chain
 * of 3. --, turns the tiles into the 64-bit keys of pvhip_topk_rows_f32 (low word: the gallery row) and writes the best k of every
 * (query row, chunk) to `scratch` by the same rounds.  Merge: one wave per query row computes 1., merges the chunks' keys by the same
 * rounds and writes 5. and 6.  `scratch`: 8 * n * ceil(g / PVHIP_GALLERY_CHUNK) * k bytes, 8-byte aligned, the caller's, overwritten.
 * `counts` (n) int32, `indices` (n, k) int32, `scores` (n, k) fp32; `norms` NULL or (n) binary64, 8-byte aligned: r of every row (of a
 * row with an element that is not finite: NaN).  1 <= n, n * d < 2^31, ceil(n / 32) * ceil(g / 1024) < 2^30, 1 <= d <= 1024, 1 <= g <= 2^24, 1 <= k <= min(g, 64), metric one
 * of the two, min_score finite when has_min_score (0 or 1), no NULL or misaligned pointer; else PVHIP_EINVAL and nothing is launched. */
#define PVHIP_GALLERY_COSINE 0
#define PVHIP_GALLERY_DOT    1
#define PVHIP_GALLERY_CHUNK  256
int pvhip_gallery_match_f32(const float* x, int n, int d, const float* packed, int g, int k, int metric, int has_min_score,
                            float min_score, void* scratch, int* counts, int* indices, float* scores, double* norms);

/* ---------------------------------------------------------------- a heatmap network's answer ---- */
/* Addition to ABI v19 (the version number is unchanged: nothing existing changed): the peak of every plane of a contiguous (n, k, h, w)
 * fp32 stack of heatmaps -- what a user of a landmark, pose or corner head makes on the host with an argmax per plane after reading
 * 4 n k h w bytes back -- so that only 16 bytes per plane are read back.  The rule (pyopenvino_amd/keypoints.py states the same one in
 * numpy and tests/keypoints_ref.py in plain loops, matched bit for bit), for the plane v[0..h)[0..w) of batch row r and channel c:
 *   1. peak    p is the first position of the plane's h * w values in the total order of pvhip_topk_rows_f32 above: NaN of any sign or
 *      payload first, then descending with +0.0 == -0.0, ties to the lower flat index.  py = p / w, px = p % w.  positions[r][c] = p;
 *      scores[r][c] holds the bits of v[py][px] unchanged.
 *   2. valid   the keypoint is valid iff its score is not NaN and (has_min == 0 or score >= min_score).  The quiet-NaN rows behind
 *      `count` of a DetectedRois or LandmarkWarps pass are void all through.
 *   3. refine  PVHIP_PEAKS_NONE: ox = oy = 0.  PVHIP_PEAKS_QUARTER: if 1 <= px <= w - 2, with l = v[py][px - 1] and r = v[py][px + 1],
 *      ox = +0.25f if r > l, -0.25f if r < l, else 0 (equal values, zeros of either sign, either neighbour NaN); on the plane's first or
 *      last column ox = 0.  oy likewise in y with h, from v[py - 1][px] and v[py + 1][px].  h == 1 or w == 1 never refines that axis.
 *      fx = (float)px + ox, fy = (float)py + oy, fp32 (exact below 2^22).
 *   4. space   PVHIP_PEAKS_HEATMAP: (fx, fy).  PVHIP_PEAKS_NORMALISED, on the pixel-edge convention pvhip_landmarks_to_warps reads (0 the
 *      left or top edge, 1 the right or bottom edge): x = (float)((double)(fx + 0.5f) / (double)w), y = (float)((double)(fy + 0.5f) /
 *      (double)h): one fp32 addition, one correctly rounded binary64 division, one rounding to fp32.  points[r][c] = (x, y); a void
 *      keypoint's are two quiet NaNs 0x7FC00000.  A valid NORMALISED block read as (n, 2 k) is what pvhip_landmarks_to_warps takes.
 * `positions` (n, k) int32, `scores` (n, k) fp32, `points` (n, k, 2) fp32; no counts are written (the caller counts the valid points).
 * `x` may be only 4-byte aligned, and a plane starts on a 16-byte boundary only when h * w % 4 == 0: each plane is split at its own
 * 16-byte boundaries.  One launch on the current stream, every plane read once (the peak and its neighbours once more), no atomics, no
 * workspace.  Two forms, by h * w: PVHIP_PEAKS_FORM_WAVE, one wave per plane, four planes per workgroup, up to 1024 elements;
 * PVHIP_PEAKS_FORM_BLOCK, one 256-thread workgroup per plane, the waves' winners combined through LDS.  pvhip_heatmap_peaks_form
 * returns the form of (h, w) -- no status, no device needed --, PVHIP_PEAKS_FORM_NONE for a plane the entry refuses.
 * n, k, h, w >= 1, 2 <= h * w <= PVHIP_PEAKS_MAX_PLANE, n * k < 2^31, refine and space each one of the two, has_min 0 or 1, min_score
 * finite, no NULL or misaligned pointer; else PVHIP_EINVAL and nothing is launched. */
#define PVHIP_PEAKS_NONE        0
#define PVHIP_PEAKS_QUARTER     1
#define PVHIP_PEAKS_HEATMAP     0
#define PVHIP_PEAKS_NORMALISED  1
#define PVHIP_PEAKS_FORM_NONE   0
#define PVHIP_PEAKS_FORM_WAVE   1
#define PVHIP_PEAKS_FORM_BLOCK  2
#define PVHIP_PEAKS_MAX_PLANE   (1 << 24)
int pvhip_heatmap_peaks_form(int h, int w);
int pvhip_heatmap_peaks_f32(const float* x, int n, int k, int h, int w, int refine, int space, int has_min, float min_score,
                            int* positions, float* scores, float* points);

/* ---------------------------------------------------------------- the local maxima of heatmaps ---- */
/* Addition to ABI v19 (the version number is unchanged: nothing existing changed): the local maxima of every plane of a contiguous
 * (n, k, h, w) fp32 stack of heatmaps with several objects per plane -- what a user of a CenterNet-style detector or of a multi-person
 * pose head makes on the host with a 3 x 3 maximum filter and a partial sort after reading 4 n k h w bytes back -- so that 4 + 20
 * max_per_row bytes per batch row are read back.  The rule (pyopenvino_amd/maxima.py states the same one in numpy and
 * tests/maxima_ref.py in plain loops, matched bit for bit), for the plane v[0..h)[0..w) of batch row r and channel c:
 *   1. maximum  key(q) is the key of (v[q], flat index q) in the total order of pvhip_topk_rows_f32 above: NaN of any sign or payload
 *      first, then descending with +0.0 == -0.0, ties to the lower index.  Position p is a maximum iff v[p] is not NaN and key(p) is
 *      larger than the key of each of its at most eight neighbours that lie inside the plane.  A plateau therefore yields only those
 *      of its pixels that have no plateau neighbour before them in raster order; a flat plane has one maximum, at index 0.  A NaN is
 *      never a maximum and suppresses all its neighbours: the quiet-NaN rows behind `count` of a DetectedRois or LandmarkWarps pass
 *      have count 0.
 *   2. screen   the maximum passes iff has_min == 0 or v[p] >= min_score.  Equality keeps.
 *   3. per plane  the first max_per_plane passing maxima are kept, in descending key order.
 *   4. per row  the kept maxima of the row's k planes are ordered by descending value, ties to the lower channel, then to the lower
 *      position: the key of (value, c * h * w + p).  The first max_per_row are the answer.
 *   5. refine / space  rules 3 and 4 of pvhip_heatmap_peaks_f32 above, word for word, applied at each answered position, with the same
 *      PVHIP_PEAKS_NONE / PVHIP_PEAKS_QUARTER and PVHIP_PEAKS_HEATMAP / PVHIP_PEAKS_NORMALISED.
 * `counts` (n) int32, `channels` (n, max_per_row) int32, `positions` (n, max_per_row) int32 the flat py * w + px, `scores`
 * (n, max_per_row) fp32 the plane's own bits, `points` (n, max_per_row, 2) fp32 (x, y).  The first counts[r] slots of row r are its
 * maxima, best first; the slots behind them are (-1, -1, quiet NaN, quiet NaN, quiet NaN), quiet NaN being 0x7FC00000.  `scratch` is
 * device memory of n * k * max_per_plane 8-byte words that only the two launches read and write.  `x` may be only 4-byte aligned and a
 * plane starts at any 4-byte phase.  Two launches on the current stream, no initialising one, no global-memory atomics: (1) every plane
 * goes through LDS once in tiles of whole rows (column chunks of 1022, in the wave form 510, where w is larger) with a halo of one row above and below each
 * tile (and one column beside a chunk), its 3 x 3 test runs on 32-bit order words, separably, and the max_per_plane largest passing
 * keys of the plane, found by a bounded buffer of keys in LDS that is sorted and cut whenever the next tile could overflow it, go to
 * `scratch`, padded with zeros; (2) one workgroup per batch row keeps the max_per_row largest of its k * max_per_plane keys, re-keyed
 * with the channel, by the same device function, and one lane per slot writes the answer.  Two forms of launch (1), by h * w:
 * PVHIP_MAXIMA_FORM_WAVE, one wave per plane, up to 1024 elements; PVHIP_MAXIMA_FORM_BLOCK, one 256-thread workgroup per plane.
 * pvhip_heatmap_maxima_form returns the form of (h, w) -- no status, no device needed --, PVHIP_MAXIMA_FORM_NONE for a plane the
 * entry refuses.
 * n, k, h, w >= 1, 2 <= h * w <= PVHIP_MAXIMA_MAX_PLANE, k * h * w <= 2^31 - 1, 1 <= max_per_plane <= PVHIP_MAXIMA_MAX_PER_PLANE,
 * 1 <= max_per_row <= PVHIP_MAXIMA_MAX_PER_ROW, n * k * max_per_plane < 2^31, refine and space each one of the two, has_min 0 or 1,
 * min_score finite, no NULL pointer, `scratch` 8-byte and the others 4-byte aligned; else PVHIP_EINVAL and nothing is launched. */
#define PVHIP_MAXIMA_MAX_PLANE      (1 << 24)
#define PVHIP_MAXIMA_MAX_PER_PLANE  256
#define PVHIP_MAXIMA_MAX_PER_ROW    1024
#define PVHIP_MAXIMA_FORM_NONE      0
#define PVHIP_MAXIMA_FORM_WAVE      1
#define PVHIP_MAXIMA_FORM_BLOCK     2
int pvhip_heatmap_maxima_form(int h, int w);
int pvhip_heatmap_maxima_f32(const float* x, int n, int k, int h, int w, int max_per_plane, int max_per_row, int refine, int space,
                             int has_min, float min_score, unsigned long long* scratch, int* counts, int* channels, int* positions,
                             float* scores, float* points);

/* ---------------------------------------------------------------- a segmentation network's answer ---- */
/* Addition to ABI v19 (the version number is unchanged: nothing existing changed): the class map of a contiguous (n, c, h, w) fp32 stack
 * of per-class score planes -- what a user of a semantic segmentation head makes on the host with an argmax across the planes after
 * reading 4 n c h w bytes back, and the pixel count and bounding rectangle of every class with it -- so that one byte per pixel and 20
 * bytes per (row, class) are read back.  The rule (pyopenvino_amd/segments.py states the same one in numpy and tests/segments_ref.py in
 * plain loops, matched exactly), for pixel (y, x) of batch row r, with v[k] = X[r][k][y][x]:
 *   1. best    k* is the first class of the pixel's c values in the total order of pvhip_topk_rows_f32 above: NaN of any sign or payload
 *      first, then descending with +0.0 == -0.0, ties to the lower class.
 *   2. void    the pixel is void iff v[k*] is NaN or (has_min == 1 and v[k*] < min_score).  Any NaN among a pixel's c scores therefore
 *      voids it: the quiet-NaN rows behind `count` of a DetectedRois or LandmarkWarps pass are void all through.  Equality keeps.
 *   3. label   labels[r][y][x] = k*, or PVHIP_SEGMENT_VOID (255) when void.  With c == 1 and a min_score: a thresholded mask.
 *   4. sums    areas[r][k] is the number of pixels of row r labelled k; extents[r][k] = (x0, y0, x1, y1) is min x, min y, max x + 1 and
 *      max y + 1 over those pixels.  Exact integers: the order in which they are accumulated does not matter.
 * `labels` (n, h, w) uint8, `areas` (n, c) int32, `extents` (n, c, 4) int32.  A class without pixels in a row reads (w, h, 0, 0) in
 * `extents` at this level, the state the initialising launch leaves, and not the (0, 0, 0, 0) of the public answer: the caller turns
 * it (areas[r][k] == 0 says where).  `x` may be only 4-byte aligned and `labels` only byte aligned: the flat run of n h w label bytes
 * is cut at its own 4-byte boundaries into quads of four pixels, each one aligned 32-bit store (the partial quads at the two ends of
 * the run are stored by the byte), and the 16-byte loads of a quad stand at whatever 4-byte phase the planes put them.  Two launches on
 * the current stream: one initialises `areas` and `extents`; one walks the quads with a bounded grid, a lane per quad, the classes four
 * loads at a time, one 32-bit order word per pixel, areas and extents summed per (wave, row, class), gathered per workgroup in LDS and sent by integer vector atomics.
 * Every score is read once; no workspace.  One form, PVHIP_SEGMENT_FORM_QUADS; pvhip_segment_labels_form returns the form of
 * (c, h, w) -- no status, no device needed --, PVHIP_SEGMENT_FORM_NONE for what the entry refuses.
 * n, c, h, w >= 1, c <= PVHIP_SEGMENT_MAX_CLASSES, 2 <= h * w <= PVHIP_SEGMENT_MAX_PLANE, n * h * w < 2^31, has_min 0 or 1, min_score
 * finite, no NULL pointer, x / areas / extents 4-byte aligned; else PVHIP_EINVAL and nothing is launched. */
#define PVHIP_SEGMENT_VOID         255
#define PVHIP_SEGMENT_MAX_CLASSES  255
#define PVHIP_SEGMENT_MAX_PLANE    (1 << 24)
#define PVHIP_SEGMENT_FORM_NONE    0
#define PVHIP_SEGMENT_FORM_QUADS   1
int pvhip_segment_labels_form(int c, int h, int w);
int pvhip_segment_labels_f32(const float* x, int n, int c, int h, int w, int has_min, float min_score,
                             unsigned char* labels, int* areas, int* extents);

/* ---------------------------------------------------------------- a text recogniser's answer ---- */
/* Addition to ABI v19 (the version number is unchanged: nothing existing changed): the greedy CTC decoding of a contiguous fp32 tensor of
 * per-timestep class scores -- what a user of a text recogniser makes on the host with argmax(-1) and a collapse after reading
 * 4 n t c bytes back -- so that 4 + 12 t bytes per batch row are read back.  `layout` says where the axes stand:
 * PVHIP_TEXT_LAYOUT_TNC reads x as (t, n, c), PVHIP_TEXT_LAYOUT_NTC as (n, t, c), PVHIP_TEXT_LAYOUT_NCT as (n, c, t).  The rule
 * (pyopenvino_amd/text.py states the same one in numpy and tests/text_ref.py in plain loops, matched bit for bit), for batch row r
 * with scores v[t][c]:
 *   1. winner  w(t) is the first class of timestep t in top_k's total order: NaN of any sign or payload first, then descending with
 *      +0.0 == -0.0, ties to the lower class.
 *   2. void    row r is void iff the winning score of any of its timesteps is NaN, that is, iff any of its T * C scores is NaN.
 *      A void row has length -1 and nothing but filler: the quiet-NaN rows behind `count` of a DetectedRois or LandmarkWarps pass
 *      are void.  An empty string (length 0) is an answer and not a void row.
 *   3. emit    timestep t emits iff w(t) != blank and (merge_repeated is false, or t == 0, or w(t) != w(t - 1)).  A repeat across
 *      a blank therefore emits twice: a, blank, a is aa.
 *   4. order   the emitting timesteps in ascending t fill slots 0, 1, ...: symbols = w(t), scores = the bits of v[t][w(t)],
 *      steps = t.
 * `lengths` (n) int32, `symbols` (n, t) int32, `scores` (n, t) fp32, `steps` (n, t) int32.  The first lengths[r] slots of row r are
 * its string in time order; the slots behind them -- all of them in a void row -- are (-1, quiet NaN, -1), quiet NaN being 0x7FC00000.
 * `blank` is the resolved class, 0 .. c - 1; `merge` is merge_repeated as 0 or 1.  `scratch` is device memory of n * t 8-byte words
 * that only the two launches read and write: scratch[r * t + i] is the key of pvhip_topk_rows_f32's order of (winning score's bits,
 * w(i)).  `x` may be only 4-byte aligned.  Two launches on the current stream, no global-memory atomics, the same bits every call:
 * (1) the winners, in one of two forms by the layout: PVHIP_TEXT_FORM_ROWS (TNC, NTC: the class axis is contiguous), one wave per
 * (r, i) row, split at its 16-byte boundaries into head, body of 16-byte pieces and tail, one pass and one wave-wide maximum, on a
 * grid of at most PVHIP_TEXT_MAX_BLOCKS workgroups of four waves that stride over the rows; PVHIP_TEXT_FORM_PLANES (NCT: the time
 * axis is contiguous), a lane per four consecutive timesteps that walks the classes in 16-byte loads at whatever 4-byte phase the
 * planes stand and takes a strictly larger order word only, one workgroup per 1024 timesteps, no cap; (2) the collapse, one
 * workgroup per batch row: the row's keys in chunks of 256, void by a workgroup-wide reduction, each emitting timestep's slot from a
 * ballot prefix within its wave plus wave and chunk offsets through LDS, every slot of the row written once, filler included.
 * pvhip_ctc_greedy_form returns the form of (layout, t, c) -- no status, no device needed --, PVHIP_TEXT_FORM_NONE for what the
 * entry refuses.
 * n, t >= 1, t <= PVHIP_TEXT_MAX_STEPS, c >= 2, n * t * c < 2^31, layout one of the three, 0 <= blank < c, merge 0 or 1, no NULL
 * pointer, `scratch` 8-byte and the others 4-byte aligned; else PVHIP_EINVAL and nothing is launched. */
#define PVHIP_TEXT_MAX_STEPS    4096
#define PVHIP_TEXT_MAX_BLOCKS   2048
#define PVHIP_TEXT_LAYOUT_TNC   0
#define PVHIP_TEXT_LAYOUT_NTC   1
#define PVHIP_TEXT_LAYOUT_NCT   2
#define PVHIP_TEXT_FORM_NONE    0
#define PVHIP_TEXT_FORM_ROWS    1
#define PVHIP_TEXT_FORM_PLANES  2
int pvhip_ctc_greedy_form(int layout, int t, int c);
int pvhip_ctc_greedy_f32(const float* x, int n, int t, int c, int layout, int blank, int merge, unsigned long long* scratch,
                         int* lengths, int* symbols, float* scores, int* steps);

/* ---------------------------------------------------------------- a dense detector head's answer ---- */
/* Addition to ABI v19 (the version number is unchanged: nothing existing changed): the table of detections of a contiguous fp32 tensor of
 * per-anchor boxes and class scores -- what a user of a YOLO-style export makes on the host with a confidence filter, a box decoding and
 * a greedy suppression after reading 4 n a e bytes back -- so that 32 bytes per surviving box are read back.  e = 4 + objectness + c
 * channels per anchor, the first four the box; PVHIP_BOXES_LAYOUT_NCA reads x as (n, e, a) (channel planes, anchors contiguous: YOLOv8 /
 * v11), PVHIP_BOXES_LAYOUT_NAC as (n, a, e) (YOLOv5 / v7, YOLOX).  The rule (pyopenvino_amd/boxes.py states the same one in numpy and
 * tests/boxes_ref.py in plain loops, matched bit for bit), for image r and anchor i with channel values v[0 .. e - 1], O = objectness:
 *   1. winner  k* is the first of the c class scores v[4 + O ..] in the total order of pvhip_topk_rows_f32 above: NaN of any sign or
 *      payload first, then descending with +0.0 == -0.0, ties to the lower class.  score = v[4 + O + k*], or, with objectness,
 *      v[4] * v[4 + O + k*] as one fp32 product, rounded once, never contracted.  The anchor is out iff !(score >= min_score) -- so for a
 *      NaN score; equality keeps.  Any NaN among an anchor's class scores therefore drops it: the quiet-NaN rows behind `count` of a
 *      DetectedRois or LandmarkWarps pass have counts = selected = 0.
 *   2. box     all four box numbers must be finite, else the anchor is out.  PVHIP_BOXES_CXCYWH corners in fp32, never contracted:
 *      xa = cx - w * 0.5f, xb = cx + w * 0.5f, ya and yb alike; PVHIP_BOXES_XYXY: the numbers themselves.  They are pixels of the
 *      network's input, in which the frame stands in the rectangle [dy, dy + ih) x [dx, dx + iw): a corner p maps to the frame in
 *      binary64 as t = ((double)p - (double)d) * (double)F / (double)i, three operations, each rounded once, none contracted, (d, i, F) =
 *      (dx, iw, frame_w) for an x corner and (dy, ih, frame_h) for a y corner.  x0 = floor(min(max(t(xa), 0), frame_w)), x1 =
 *      ceil(min(max(t(xb), 0), frame_w)), w = x1 - x0; y0, y1, h alike.  The anchor is out when w < min_w or h < min_h (an inverted box
 *      is), and, with labels != NULL, unless k* == labels[j] for some j < num_labels <= 64 (num_labels 0 with a pointer: every anchor is
 *      out).  With the identity geometry (0, 0, frame_w, frame_h) p * F / F is p itself: a box on integer pixel edges stays on them.
 *   3. cap     selected[r] counts the anchors still in.  The max_candidates best of them go on, in descending score with +0.0 == -0.0,
 *      ties to the lower anchor: the descending order of the keys (score bits, i) of pvhip_topk_rows_f32.
 *   4. suppression  greedy in that order by the rule of pvhip_detections_merge_tiles below, word for word: int64 areas of the frame
 *      rectangles, den the union (PVHIP_OVERLAP_IOU) or the smaller area (PVHIP_OVERLAP_IOS), a candidate dropped iff an earlier kept
 *      one -- of the same k* when per_label -- overlaps it with (double)inter > (double)threshold * (double)den; equality keeps.
 *   5. table   image r keeps its first counts[r] = min(kept, max_per_image) kept candidates; rows are eight 32-bit words (r, x0, y0, w,
 *      h, k*, score bits, r * a + i), in (image, order of 3.) order without gaps; total = sum(counts).
 * `header` = counts[n], selected[n], total; `rows`: n * max_per_image rows of 32 bytes at most, 16-byte aligned; rows >= total are not
 * written.  `x` may be only 4-byte aligned.  `scratch` is device memory, 16-byte aligned, that only the three launches read and write:
 * the (n, a) 8-byte keys, the (n, a) int32 winners, then -- at the next 16-byte boundary -- the n * max_per_image staging rows:
 * PVHIP_BOXES_SCRATCH_BYTES(n, a, max_per_image) bytes.
 * Three launches on the current stream, no global-memory atomics, no workgroup waits for another, the same bits every call.
 * (1) score: x is read once; every anchor's key -- that of (score bits, i) when it passes 1. and 2. in full, else 0 -- and its k* are
 * written.  PVHIP_BOXES_FORM_PLANES (NCA): a lane owns four consecutive anchors and walks the class planes in 16-byte loads at whatever
 * 4-byte phase they stand, one 32-bit order word and class per anchor, a strictly larger word replacing.  NAC: a team of lanes takes an
 * anchor's e contiguous numbers in 16-byte pieces between the row's own 16-byte boundaries, then one team-wide maximum of keys --
 * PVHIP_BOXES_FORM_ROWS_TEAM, 16 lanes and four anchors a wave, for e <= PVHIP_BOXES_TEAM_ROW, PVHIP_BOXES_FORM_ROWS_WAVE, a wave per
 * anchor, above.  pvhip_dense_boxes_form returns the form of (layout, a, e) -- no status, no device needed --, PVHIP_BOXES_FORM_NONE
 * for what the entry refuses.  (2) images: one workgroup of 1024 lanes per image keeps the max_candidates largest keys by the bounded
 * buffer of pvhip_heatmap_maxima_f32 (in dynamic LDS, at most 64 KB), counts selected, makes the sorted survivors' rectangles again by
 * the device function of (1), suppresses greedily in chunks of 64 as pvhip_detections_merge_tiles does and writes the kept rows to the
 * image's staging rows.  (3) write: one wave per image sums the counts in front of it and copies its rows in 16-byte stores; the
 * last image's wave writes total.
 * n, a, c >= 1, n * a * (4 + objectness + c) < 2^31, layout, box and overlap each one of the two, objectness and per_label 0 or 1,
 * min_score finite, 0 <= num_labels <= 64 (labels not NULL when > 0), frame_h, frame_w, iw, ih in 1 .. 2^24, dx, dy in 0 .. 2^24,
 * min_h, min_w >= 1, 1 <= max_candidates <= PVHIP_BOXES_MAX_CANDIDATES, 1 <= max_per_image <= max_candidates, 0 <= threshold <= 1, no
 * NULL or misaligned pointer; else PVHIP_EINVAL and nothing is launched. */
#define PVHIP_BOXES_LAYOUT_NCA       0
#define PVHIP_BOXES_LAYOUT_NAC       1
#define PVHIP_BOXES_CXCYWH           0
#define PVHIP_BOXES_XYXY             1
#define PVHIP_BOXES_FORM_NONE        0
#define PVHIP_BOXES_FORM_PLANES      1
#define PVHIP_BOXES_FORM_ROWS_TEAM   2
#define PVHIP_BOXES_FORM_ROWS_WAVE   3
#define PVHIP_BOXES_TEAM_ROW         128
#define PVHIP_BOXES_MAX_CANDIDATES   4096
#define PVHIP_BOXES_SCRATCH_BYTES(n, a, max_per_image) \
    ((((size_t)12 * (size_t)(n) * (size_t)(a) + 15u) & ~(size_t)15u) + (size_t)32 * (size_t)(n) * (size_t)(max_per_image))
int pvhip_dense_boxes_form(int layout, int a, int e);
int pvhip_dense_boxes_f32(const float* x, int n, int a, int c, int layout, int objectness, int box, float min_score,
                          const int* labels, int num_labels, int frame_h, int frame_w, int dx, int dy, int iw, int ih,
                          int min_h, int min_w, int max_candidates, int overlap, float threshold, int per_label, int max_per_image,
                          void* scratch, int* header, int* rows);

/* ---------------------------------------------------------------- a detector's answer ------ */
/* Addition to ABI v18 (the version number is unchanged: nothing existing changed): the records of pvhip_detection_output_f32 become one
 * flat table of the detections a caller wants -- what the reference's sample makes on the host with `for record in res.reshape(100, 7):
 * if conf > 0.5: x0 = int(xmin * img_w) ...` -- so that only the survivors are read back.  `records`: images * records_per_image rows of
 * [rank, label, score, xmin, ymin, xmax, ymax], image b being rows [b P, (b + 1) P).  `live`, `selected` and the rectangle (x0, y0, w, h)
 * over (frame_h, frame_w) are exactly those of pvhip_detections_to_rois above (one device function serves both): an image's list ends at
 * its first row whose column 0 is not >= 0; a live row is selected when score >= min_confidence, its four corners are finite and (labels
 * == NULL or) its label equals (float)labels[j] for some j < num_labels <= 64; x0 = floor(min(max(xmin * frame_w, 0), frame_w)), x1 =
 * ceil(min(max(xmax * frame_w, 0), frame_w)) in fp32, never contracted, y0 / y1 alike with frame_h; dropped when x1 - x0 < min_w or
 * y1 - y0 < min_h.  selected[b] counts the survivors of image b.  New here:
 *   cap     image b keeps its first counts[b] = min(selected[b], max_per_image) survivors in position order (its best scores: an image's
 *           records stand in descending score order);
 *   table   the kept survivors of all images stand in (image, position) order without a gap between images; total = sum(counts);
 *   row     one survivor is eight 32-bit words (b, x0, y0, w, h, label, score bits, record): label = (int32) of column 1 when that is
 *           finite and in [-2^31, 2^31), else -1; score bits are the record's own; record = b P + p.  Rows >= total are not written.
 * header = counts[images], then selected[images], then total: 2 * images + 1 ints.  `rows` holds images * min(P, max_per_image) rows of
 * 32 bytes and is 16-byte aligned.  The same rule in numpy: tests/detections_ref.py, matched word for word.  Two launches on the current
 * stream (count, then write: one wave per image; no atomics, no wait of one workgroup on another, so the result does not depend on
 * timing), no allocation, no workspace.  images, records_per_image, min_h, min_w, max_per_image >= 1, images * records_per_image <
 * 2^31 / 7, frame_h, frame_w in [1, 2^24], `labels` NULL (any label; num_labels == 0) or a device pointer with num_labels <= 64 (a
 * non-NULL `labels` with num_labels == 0 selects nothing), no NULL records / header / rows; else PVHIP_EINVAL and nothing is launched. */
int pvhip_detections_compact(const float* records, int images, int records_per_image, int frame_h, int frame_w, float min_confidence,
                             const int* labels, int num_labels, int min_h, int min_w, int max_per_image, int* header, int* rows);
/* Addition to ABI v18 (the version number is unchanged: nothing existing changed): the same answer for a detector whose input was fitted:
 * the rectangle rule of pvhip_detections_to_rois_fit (one device function serves all four entries), everything else as above. */
int pvhip_detections_compact_fit(const float* records, int images, int records_per_image, int frame_h, int frame_w, float min_confidence,
                                 const int* labels, int num_labels, int min_h, int min_w, int max_per_image, int* header, int* rows,
                                 int net_h, int net_w, int dx, int dy, int iw, int ih);
/* Addition to ABI v18 (the version number is unchanged: nothing existing changed): a TILED detector's answer.  The n batch rows of the
 * pass are tiles of m frames -- `tiles` is the (n, 5) int32 device table of a RoiInput, row b = (f, x, y, w, h): batch row b saw the
 * rectangle [y, y + h) x [x, x + w) of frame f --, and the records of all tiles become one table of FRAME detections: shifted into frame
 * pixels, ordered by score, and suppressed greedily across the tiles of a frame, so that an object in the overlap of two tiles comes back
 * once.  `records`: n * records_per_tile rows of [rank, label, score, xmin, ymin, xmax, ymax], tile b being rows [b P, (b + 1) P).
 *   1. candidates  tile b contributes nothing if f is outside [0, m), w < 1 or h < 1 (or w or h above 2^24, which fp32 does not hold
 *      exactly).  Otherwise its candidates are exactly the records pvhip_detections_compact selects over (frame_h, frame_w) = (h, w) of
 *      the tile -- live, score >= min_confidence, four finite corners, the label filter, floor / ceil of the clamped fp32 products,
 *      (min_h, min_w); one device function serves both entries -- so a rectangle clamps to its tile: the detector saw nothing else.  The
 *      frame rectangle is (x + x0, y + y0, w, h) (the sums wrap as int32 do; a RoiInput's table never gets there).  A tile keeps its first
 *      max_per_tile candidates in position order.  selected[f] = the kept candidates of all tiles of frame f.
 *   2. order  the candidates of a frame are ordered by descending score as a float, +0.0 = -0.0 (no NaN passes the screen); ties go to the
 *      lower flat record b P + p: the order of pvhip_topk_rows_f32.
 *   3. suppression  greedy in that order: candidate i is dropped iff an earlier candidate j that was kept overlaps it -- and, with
 *      per_label = 1, has the same label word (the row's int32 label below).  With int64 inter = the area of the intersection of the two
 *      frame rectangles (0 when they do not meet), a_i, a_j = their areas, den = a_i + a_j - inter for PVHIP_OVERLAP_IOU and den =
 *      min(a_i, a_j) for PVHIP_OVERLAP_IOS: i overlaps j iff (double)inter > (double)threshold * (double)den -- one IEEE float64 product
 *      and one comparison; extents are at most 2^24, so every area is exact in float64.  Equality does not suppress.
 *   4. cap and table  a frame keeps its first max_per_frame kept candidates: counts[f].  The table holds them in (frame, order of step 2)
 *      order without gaps; a row is (f, x0, y0, w, h, label, score bits, record) as pvhip_detections_compact writes it, record = b P + p:
 *      the tile of a row is record / P.  total = sum(counts).  Rows >= total are not written.
 * header = counts[m], then selected[m], then total: 2 m + 1 ints.  `rows` holds min(n * max_per_tile, m * max_per_frame) rows of 32 bytes
 * and is 16-byte aligned.  `scratch`: 9 * n * max_per_tile + n ints, 16-byte aligned, the caller's, overwritten: the candidate rows, the
 * place of each in its frame's answer, the candidates of each tile.  The same rule in numpy: tests/tiles_ref.py, matched word for word.
 * Three launches on the current stream (one wave per tile; one workgroup per frame: a sort of 64-bit keys in LDS, then the suppression;
 * one wave per tile again), no allocation: no atomics and no wait of one workgroup on another, so nothing depends on timing.  n,
 * records_per_tile, min_h, min_w, max_per_tile, max_per_frame >= 1, 1 <= frames < 2^30, n * records_per_tile < 2^31 / 7, n * max_per_tile
 * <= 4096 (the candidate capacity), threshold in [0, 1] (not NaN), overlap one of the two kinds, per_label 0 or 1, `labels` NULL (any
 * label; num_labels == 0) or a device pointer with num_labels <= 64 (non-NULL with num_labels == 0 selects nothing), no other NULL or
 * misaligned pointer; else PVHIP_EINVAL and nothing is launched. */
#define PVHIP_OVERLAP_IOU 0
#define PVHIP_OVERLAP_IOS 1
int pvhip_detections_merge_tiles(const float* records, const int* tiles, int n, int records_per_tile, int frames, float min_confidence,
                                 const int* labels, int num_labels, int min_h, int min_w, int max_per_tile, int overlap, float threshold,
                                 int per_label, int max_per_frame, int* scratch, int* header, int* rows);
/* Addition to ABI v18 (the version number is unchanged: nothing existing changed): the answer of a detector whose batch rows are REGIONS
 * of m frames -- of any aspect, placed in its (net_h, net_w) input by the fit the preprocessing launch used (pvhip_input_preprocess_fit_f32
 * with the same table) --: a second-stage detector behind a first one (person -> face, vehicle -> plate), or tiles that are not the
 * network's aspect.  `regions` is the (n, 5) int32 device table, row b = (f, x, y, w, h): a RoiInput's table, or the one
 * pvhip_detections_to_rois wrote, whose rows from `count` on are (-1, 0, 0, 0, 0).  `fit`: 0 STRETCH, 1 LETTERBOX, 2 TOP_LEFT.
 *   1. candidates  region b contributes nothing if f is outside [0, m), or w or h is outside [1, 2^24].  Otherwise (dx, dy, iw, ih) is the
 *      fitted rectangle of a source of (hs, ws) = (h, w) in (hd, wd) = (net_h, net_w) by the integer rule stated at
 *      pvhip_input_preprocess_fit_f32 (one function serves the launch that places the pixels and this one), and the region's candidates are
 *      exactly the records pvhip_detections_compact_fit selects over (frame_h, frame_w) = (h, w) with (net_h, net_w, dx, dy, iw, ih): a
 *      record is live in front of the list end; score >= min_confidence; the finite check is on the record's own four corners; the label
 *      filter; each corner is mapped back in fp32, never contracted, three roundings, u = (xmin * (float)net_w - (float)dx) / (float)iw
 *      (ymin / ymax with net_h, dy, ih); the rectangle is floor / ceil of the clamped fp32 products of u with the region's extent, subject
 *      to (min_h, min_w).  A box in the padding therefore clamps to the region's edge and one wholly in the padding is dropped.  With fit 0
 *      no mapping is applied at all (net_h and net_w are not read): the answer is pvhip_detections_merge_tiles' bit for bit.  The frame
 *      rectangle is (x + x0, y + y0, w, h) (the sums wrap as int32 do).  A region keeps its first max_per_region candidates in position
 *      order.  selected[f] = the kept candidates of all regions of frame f.
 *   2. - 4. order, suppression, cap and table: those of pvhip_detections_merge_tiles unchanged -- descending score, ties to the lower flat
 *      record; greedy, int64 areas, (double)inter > (double)threshold * (double)den, equality does not suppress; max_per_frame; rows
 *      (f, x0, y0, w, h, label, score bits, record), the region of a row is record / P.  For a table pvhip_detections_to_rois wrote,
 *      record_of[record / P] there is the first-stage record the box came from.
 * header, `rows` and `scratch` (9 * n * max_per_region + n ints) as for pvhip_detections_merge_tiles.  The same rule in numpy:
 * tests/regions_ref.py, matched word for word.  Three launches on the current stream (the candidates launch computes each region's geometry
 * once per wave; the frames and write launches are pvhip_detections_merge_tiles' own), no allocation, no atomics, no wait of one workgroup
 * on another.  The limits of pvhip_detections_merge_tiles, fit in {0, 1, 2}, and net_h, net_w in [1, 2^24] when fit != 0; else PVHIP_EINVAL
 * and nothing is launched. */
int pvhip_detections_merge_regions(const float* records, const int* regions, int n, int records_per_region, int frames, float min_confidence,
                                   const int* labels, int num_labels, int min_h, int min_w, int max_per_region, int overlap, float threshold,
                                   int per_label, int max_per_frame, int net_h, int net_w, int fit, int* scratch, int* header, int* rows);

/* ---------------------------------------------------------------- multi-GPU gather ---------- */
/* No reference counterpart (the reference is single-process).  Batch shards are independent; the only
 * exchange is an all-gather of the Result tensor over RCCL/xGMI.  unique_id is a 128-byte buffer. */
#define PVHIP_UNIQUE_ID_BYTES 128
int pvhip_comm_unique_id(void* unique_id_out);
int pvhip_comm_init(const void* unique_id, int rank, int world);
int pvhip_comm_allgather_f32(const float* send, float* recv, size_t count_per_rank);   /* every rank the SAME count (ncclAllGather) */
int pvhip_comm_ranks(int* count);                 /* ncclCommCount of the communicator: how many ranks RCCL itself sees */
int pvhip_comm_destroy(void);

/* ---------------------------------------------------------------- input formats (ABI v17) --- */
/* Parameter.py:11-13 casts the caller's array to the IR type; the reference's callers hand it `cv2_image.transpose((2,0,1)).astype(float32)`.
 * A network input declared U8 and / or NHWC (IENetwork.input_info) is uploaded as it is and converted here, in one launch, into the fp32
 * NCHW tensor `dst` of shape (n, c, h, w): src_u8 = 1: `src` holds uint8 values (else fp32); src_nhwc = 1: `src` is (n, h, w, c) (else
 * (n, c, h, w)).  Exact: dst == src.transpose(0, 3, 1, 2).astype(float32) bit for bit.  fp32 NCHW is a device copy.  n <= 65535,
 * c * h * w < 2^31, c <= 4096 for NHWC (pvhip_layout.hip). */
int         pvhip_input_to_nchw_f32(const void* src, float* dst, int n, int c, int h, int w, int src_u8, int src_nhwc);
/* ABI v19.  What that entry launches (host-only): src_align / dst_align are the two addresses modulo 16, which decide the 16-byte forms.
 * PVHIP_EINVAL as the entry (c > 4096 for NHWC).                                                                                   */
#define PVHIP_INPUT_COPY           0   /* fp32 NCHW: a device copy                                                            */
#define PVHIP_INPUT_U8_LINEAR      1   /* u8_to_f32_kernel                                                                    */
#define PVHIP_INPUT_NHWC           2   /* nhwc_to_nchw_kernel<T, VL, VS>                                                      */
#define PVHIP_INPUT_FORM_KIND      0
#define PVHIP_INPUT_FORM_VEC       1   /* U8_LINEAR: 1 when the word loop is taken (src 4-byte, dst 16-byte aligned, >= 4 elements) */
#define PVHIP_INPUT_FORM_TILE      2   /* NHWC: pixels per workgroup (1024 halved until tile * c * sizeof(T) <= 16 KB)        */
#define PVHIP_INPUT_FORM_VL        3   /* NHWC: 16-byte loads                                                                 */
#define PVHIP_INPUT_FORM_VS        4   /* NHWC: 16-byte stores                                                                */
#define PVHIP_INPUT_FORM_GRID_X    5
#define PVHIP_INPUT_FORM_GRID_Y    6
int         pvhip_input_to_nchw_form(int n, int c, int h, int w, int src_u8, int src_nhwc, int src_align, int dst_align, int* form);
/* Addition to ABI v17 (the version number is unchanged: nothing existing changed): an input with declared preprocessing
 * (IENetwork.input_info[name].preprocess_info) -- bilinear resize of a (src_h, src_w) source to the Parameter's (dst_h, dst_w), channel
 * reversal, per-channel mean / scale -- and the format change above, in ONE launch into the fp32 NCHW tensor `dst` (n, c, dst_h, dst_w).
 * `src`: uint8 (src_u8 = 1) or fp32 values, (n, src_h, src_w, c) for src_nhwc = 1, else (n, c, src_h, src_w).  Resize iff the extents
 * differ: half-pixel centres clamped at the border, no antialiasing, coordinates exact in integers (pvhip_preprocess.hip; the same rule
 * in numpy: tests/preprocess_ref.py, matched bit for bit).  reverse_channels = 1: output channel k reads source channel c-1-k.  `mean` /
 * `std_scale`: NULL or c device floats, y = (v - mean[k]) / std_scale[k].  Equal extents, no reversal, both NULL: exactly the conversion
 * above.  n <= 65535, c <= 1024, c * h * w < 2^31 for source and destination, fp32 sources 4-byte aligned; else PVHIP_EINVAL. */
int         pvhip_input_preprocess_f32(const void* src, float* dst, int n, int c, int src_h, int src_w, int dst_h, int dst_w,
                                       int src_u8, int src_nhwc, int reverse_channels, const float* mean, const float* std_scale);
/* Addition to ABI v17 (the version number is unchanged: nothing existing changed): the same launch for a YUV 4:2:0 source
 * (preprocess_info.color_format 'NV12' / 'I420'), a video decoder's frame as it is.  `src`: uint8, n frames of 3 src_h / 2 rows of src_w
 * bytes each: the Y plane, then src_h / 2 rows of src_w / 2 interleaved (U, V) pairs (planar = 0, NV12) or the U plane and the V plane of
 * src_h / 2 x src_w / 2 bytes each (planar = 1, I420); any alignment.  Every pixel is converted with the (U, V) of its 2 x 2 block (no
 * chroma interpolation) by the BT.601 limited-range rule in 20-bit integers (pvhip_preprocess.hip; in numpy: tests/yuv_ref.py) to uint8
 * B, G, R -- channel 0 is B --, and that image goes through the resize, reversal (reverse_channels = 1: R, G, B) and mean / scale of
 * pvhip_input_preprocess_f32 with c = 3 into `dst` (n, 3, dst_h, dst_w), bit for bit what that entry gives for the converted U8 NHWC
 * image.  n <= 65535, src_h and src_w even, 3 * h * w < 2^31 for source and destination; else PVHIP_EINVAL. */
int         pvhip_input_preprocess_yuv_f32(const void* src, float* dst, int n, int src_h, int src_w, int dst_h, int dst_w, int planar,
                                           int reverse_channels, const float* mean, const float* std_scale);
/* Addition to ABI v17 (the version number is unchanged: nothing existing changed): regions of interest.  The two launches above with a
 * source rectangle per output image: `src` holds m frames of extent (src_h, src_w) in the format of the entry above it (m is independent
 * of n), `rois` is a device pointer to n x 5 int32 (id, x, y, w, h) -- the order of OpenVINO's ROI struct --, and image b of `dst` is the
 * rectangle [y, y + h) x [x, x + w) of frame id, cropped and THEN resized to (dst_h, dst_w): the taps clamp at the rectangle's edge, not
 * the frame's; a rectangle of exactly (dst_h, dst_w) is copied, not interpolated; a YUV rectangle may have an odd origin and odd sizes (a
 * pixel takes the chroma of its 2 x 2 block of the frame).  Reversal and mean / scale as above.  In numpy: tests/roi_ref.py, matched bit
 * for bit.  max_roi_h / max_roi_w: the largest h and w in the table, which the caller knows (the tiles are sized for them on the host).
 * The table is read on the device only: an image whose rectangle is not inside a frame (id outside [0, m), x or y < 0, w or h < 1,
 * x + w > src_w, y + h > src_h) or exceeds max_roi_h / max_roi_w is written as quiet NaN, and nothing of `src` is read for it.
 * The limits of the entries above, and rois != NULL, m >= 1, 1 <= max_roi_h <= src_h, 1 <= max_roi_w <= src_w; else PVHIP_EINVAL. */
int         pvhip_input_preprocess_roi_f32(const void* src, float* dst, const int* rois, int n, int m, int c, int src_h, int src_w,
                                           int dst_h, int dst_w, int max_roi_h, int max_roi_w, int src_u8, int src_nhwc,
                                           int reverse_channels, const float* mean, const float* std_scale);
int         pvhip_input_preprocess_yuv_roi_f32(const void* src, float* dst, const int* rois, int n, int m, int src_h, int src_w,
                                               int dst_h, int dst_w, int max_roi_h, int max_roi_w, int planar, int reverse_channels,
                                               const float* mean, const float* std_scale);
/* Addition to ABI v18 (the version number is unchanged: nothing existing changed): the same launch for frames of 4-byte units
 * (preprocess_info.color_format 'YUY2' / 'UYVY' / 'BGRX' / 'RGBX'), a camera's, a capture card's or a screen capture's frame as it is.
 * `src`: uint8, any alignment; kind 0 YUY2, 1 UYVY, 2 BGRX, 3 RGBX.
 *   YUY2 / UYVY (packed YUV 4:2:2): n frames of shape (src_h, src_w, 2), src_w even, src_h any value >= 1.  Each row is src_w / 2 groups
 *     of 4 bytes: Y0 U Y1 V for YUY2, U Y0 V Y1 for UYVY.  Pixel (y, x) has luma Y[x & 1] of group x / 2 of row y, and that group's
 *     (U, V): chroma is not interpolated.  Each pixel goes to B, G, R by exactly the integer rule of pvhip_input_preprocess_yuv_f32
 *     (BT.601 limited range over 2^20, arithmetic shifts, clamp to [0, 255]; tests/yuv_ref.py): the same function, not a second set of
 *     constants.
 *   BGRX / RGBX (four-byte pixels): n frames of shape (src_h, src_w, 4), any src_h, src_w >= 1.  The B, G, R image is bytes 0, 1, 2 of
 *     every pixel for BGRX and bytes 2, 1, 0 for RGBX; byte 3 is never read into the result, whatever it holds.
 * The resulting uint8 B, G, R image -- channel 0 is B -- goes through the resize, reversal (reverse_channels = 1: R, G, B) and mean /
 * scale of pvhip_input_preprocess_f32 with c = 3 into `dst` (n, 3, dst_h, dst_w), bit for bit what that entry gives for the converted
 * U8 NHWC image.  In numpy: tests/packed_ref.py.  The _roi form is pvhip_input_preprocess_roi_f32's for these frames: image b is the
 * rectangle rois[b] = (id, x, y, w, h) of the CONVERTED frame id of m, the taps clamp at the rectangle's edge, a 4:2:2 pixel keeps the
 * chroma of its absolute column pair (so a rectangle may start on an odd x and have an odd w), and an invalid or oversized rectangle is
 * written as quiet NaN with nothing read for it.  One launch on the current stream, no allocation.  kind in 0..3, src_w even for kinds
 * 0 and 1, no NULL src / dst (/ rois), every size >= 1, n <= 65535, 3 * h * w < 2^31 for source and destination, m >= 1,
 * 1 <= max_roi_h <= src_h, 1 <= max_roi_w <= src_w; else PVHIP_EINVAL and nothing is launched. */
int         pvhip_input_preprocess_packed_f32(const void* src, float* dst, int n, int src_h, int src_w, int dst_h, int dst_w,
                                              int kind, int reverse_channels, const float* mean, const float* std_scale);
int         pvhip_input_preprocess_packed_roi_f32(const void* src, float* dst, const int* rois, int n, int m, int src_h, int src_w,
                                                  int dst_h, int dst_w, int max_roi_h, int max_roi_w, int kind, int reverse_channels,
                                                  const float* mean, const float* std_scale);
/* Addition to ABI v18 (the version number is unchanged: nothing existing changed): the launches above with an aspect-preserving fit
 * (preprocess_info.resize_fit 'LETTERBOX' / 'TOP_LEFT') in place of the stretch.  Each takes the arguments of the matching _roi_ entry --
 * rois == NULL: whole images, image b is source image b, and m, max_roi_h, max_roi_w are ignored (taken as n, src_h, src_w) -- plus
 * `fit` (1 LETTERBOX, 2 TOP_LEFT) and `pad_value`, one finite fp32 number in source units.  The geometry, integers only (int64): a
 * source (or rectangle) of (hs, ws) onto (hd, wd) = (dst_h, dst_w) is fitted into
 *   wide, ws hd >= hs wd:  iw = wd, ih = min(max((2 hs wd + ws) / (2 ws), 1), hd)   (the short side rounded half up)
 *   else:                  ih = hd, iw = min(max((2 ws hd + hs) / (2 hs), 1), wd)
 *   LETTERBOX: dx = (wd - iw) / 2, dy = (hd - ih) / 2 (floor);  TOP_LEFT: dx = dy = 0.
 * Output pixel (y, x) inside [dy, dy + ih) x [dx, dx + iw) is exactly what the entry without the fit gives at (y - dy, x - dx) for the
 * same source onto a destination of (ih, iw): the same taps, the same fp32 expression in the same order, the rule that a source or
 * rectangle of exactly (ih, iw) is copied included.  Outside, the interpolated value is pad_value, and it goes through the same
 * (v - mean[k]) / std_scale[k].  A geometry of whole images that fills the destination IS the launch without the fit.  An invalid or
 * oversized rectangle is written as quiet NaN over the whole image, padding included; a tile that lies wholly in the padding reads
 * nothing of `src`.  In numpy: tests/letterbox_ref.py, matched bit for bit.  The limits of the _roi_ entries, fit 1 or 2, pad_value
 * finite; else PVHIP_EINVAL and nothing is launched. */
int         pvhip_input_preprocess_fit_f32(const void* src, float* dst, const int* rois, int n, int m, int c, int src_h, int src_w,
                                           int dst_h, int dst_w, int max_roi_h, int max_roi_w, int src_u8, int src_nhwc,
                                           int reverse_channels, const float* mean, const float* std_scale, int fit, float pad_value);
int         pvhip_input_preprocess_yuv_fit_f32(const void* src, float* dst, const int* rois, int n, int m, int src_h, int src_w,
                                               int dst_h, int dst_w, int max_roi_h, int max_roi_w, int planar, int reverse_channels,
                                               const float* mean, const float* std_scale, int fit, float pad_value);
int         pvhip_input_preprocess_packed_fit_f32(const void* src, float* dst, const int* rois, int n, int m, int src_h, int src_w,
                                                  int dst_h, int dst_w, int max_roi_h, int max_roi_w, int kind, int reverse_channels,
                                                  const float* mean, const float* std_scale, int fit, float pad_value);
/* Addition to ABI v18 (the version number is unchanged: nothing existing changed): affine warps.  Image b of `dst` (n, c, dst_h, dst_w) is
 * frame id of the m frames in `src`, sampled through a 2 x 3 matrix: `table` is a device pointer to n x 7 int64
 * (id, A00, A01, C0, A10, A11, C1), the coefficients in Q16 (the host's rint(v * 65536), ties to even; |A| <= 2^26, |C| <= 2^40, so
 * nothing below overflows int64).  `format` says what the frames are and `how` is the last format argument of the matching entry
 * above: format 0 raw, how = src_u8 | src_nhwc << 1; format 1 YUV 4:2:0, how = planar; format 2 frames of 4-byte units, how = kind.
 * Output pixel (y, x) of image b, integers for coordinates and fp32 in a fixed order for values:
 *   SX = A00 x + A01 y + C0,  SY = A10 x + A11 y + C1                                  (int64)
 *   ix = SX >> 16 (arithmetic: floor),  fx = float(SX & 0xFFFF) * 2^-16 (exact);  iy, fy likewise
 *   P(r, c) = the pixel of frame id at row r, column c when 0 <= r < src_h and 0 <= c < src_w (compared in int64), else pad_value in
 *             every channel; for formats 1 and 2 the converted uint8 B, G, R of the entries above (a 4:2:0 pixel takes the chroma of
 *             its 2 x 2 block of the frame, a 4:2:2 pixel that of its absolute column pair: the same functions, the same constants)
 *   top = fx == 0 ? P(iy, ix) : (1 - fx) P(iy, ix) + fx P(iy, ix + 1);   bot: the same on row iy + 1, used only when fy != 0
 *   v   = fy == 0 ? top : (1 - fy) top + fy bot                                        (fp32, in that order, never contracted to fma)
 * and then the reversal (reverse_channels = 1: output channel k reads channel c-1-k) and (v - mean[k]) / std_scale[k] of the entries
 * above; pad_value is in source units and goes through them like a pixel.  A zero fraction takes no second tap: an integer translation
 * is a copy bit for bit (fp32 -0.0, infinities and NaN included), A00 = -65536 a reversed copy.  Pixel centres sit at the integers: the
 * matrix is the one cv2.warpAffine takes with WARP_INVERSE_MAP.  In numpy: tests/warp_ref.py, matched bit for bit.  The table is read
 * on the device only: an image whose id is outside [0, m) is written as quiet NaN, and nothing of `src` is read for it.  One launch on
 * the current stream, no allocation.  The limits of the _roi_ entries for the format (format 0: c <= 1024, fp32 sources 4-byte aligned;
 * format 1: src_h, src_w even, how 0 or 1; format 2: how in 0..3, src_w even for kinds 0 and 1), and table != NULL, m >= 1, format in
 * 0..2, how in 0..3 for format 0, c == 3 for formats 1 and 2, pad_value finite; else PVHIP_EINVAL and nothing is launched. */
int         pvhip_input_preprocess_warp_f32(const void* src, float* dst, const long long* table, int n, int m, int c, int src_h,
                                            int src_w, int dst_h, int dst_w, int format, int how, int reverse_channels,
                                            const float* mean, const float* std_scale, float pad_value);
/* Addition to ABI v18 (the version number is unchanged: nothing existing changed): the YUV launches above for frames of another matrix
 * or range (preprocess_info.color_standard / color_range).  ONE integer rule converts every YUV pixel, in 32-bit ints with arithmetic
 * shifts, and six ints say which encoding it undoes:
 *   y = max(Y - yoff, 0),  u = U - 128,  v = V - 128,  t = y CY + 2^19
 *   B = clamp((t + CBU u) >> 20),  G = clamp((t - CGV v - CGU u) >> 20),  R = clamp((t + CRV v) >> 20)        clamp to [0, 255]
 *   matrix  full_range                       yoff       CY      CRV      CGV      CGU      CBU
 *     0         0       BT.601 limited        16   1220542  1673527   852492   409993  2116026    (what every entry above applies)
 *     0         1       BT.601 full (JFIF)     0   1048576  1470104   748826   360853  1858077
 *     1         0       BT.709 limited        16   1220945  1879825   558796   223607  2215014
 *     1         1       BT.709 full            0   1048576  1651297   490864   196424  1945738
 *     2         0       BT.2020 limited       16   1220945  1760217   682019   196426  2245811
 *     2         1       BT.2020 full           0   1048576  1546230   599107   172546  1972791
 * Row (0, 0) is cv2's three-decimal coefficients, kept bit for bit; every other row is rint(x 2^20) of CRV = 2 (1 - Kr), CBU = 2 (1 - Kb),
 * CGV = 2 Kr (1 - Kr) / Kg, CGU = 2 Kb (1 - Kb) / Kg with Kg = 1 - Kr - Kb and (Kr, Kb) = (0.299, 0.114), (0.2126, 0.0722),
 * (0.2627, 0.0593), times 255/224 for limited range, where CY = 255/219 too.  Over all 2^24 byte triples every intermediate stays below
 * 5.8e8 and each channel is within 1 of the rounded, clamped float64 matrix value.  The chroma a pixel takes does not change (4:2:0: its
 * 2 x 2 block; 4:2:2: its absolute column pair; no interpolation), nor does anything behind the conversion.  In numpy:
 * tests/colorimetry_ref.py.
 *   _yuv_color_     the arguments of pvhip_input_preprocess_yuv_fit_f32, then matrix and full_range.  fit may be 0 as well: the stretch,
 *                   whatever pad_value holds.  fit = 0 and rois == NULL is pvhip_input_preprocess_yuv_f32, fit = 0 with a table
 *                   pvhip_input_preprocess_yuv_roi_f32; with (matrix, full_range) = (0, 0) each form is its existing entry bit for bit.
 *   _packed_color_  the same over pvhip_input_preprocess_packed_fit_f32; kinds 2 and 3 hold nothing to convert: PVHIP_EINVAL for them
 *                   unless matrix and full_range are both 0.
 *   _warp_color_    the arguments of pvhip_input_preprocess_warp_f32, then matrix and full_range; format 0, and format 2 with how 2 or 3,
 *                   likewise only with both 0.
 * One launch on the current stream, no allocation; the kernels of the entries above, reading the six ints from the launch arguments
 * ((0, 0) takes the very instantiations of those entries, whose constants are literals).  The
 * limits of the entry each generalises, matrix in 0..2, full_range 0 or 1; else PVHIP_EINVAL and nothing is launched. */
int         pvhip_input_preprocess_yuv_color_f32(const void* src, float* dst, const int* rois, int n, int m, int src_h, int src_w,
                                                 int dst_h, int dst_w, int max_roi_h, int max_roi_w, int planar, int reverse_channels,
                                                 const float* mean, const float* std_scale, int fit, float pad_value, int matrix,
                                                 int full_range);
int         pvhip_input_preprocess_packed_color_f32(const void* src, float* dst, const int* rois, int n, int m, int src_h, int src_w,
                                                    int dst_h, int dst_w, int max_roi_h, int max_roi_w, int kind, int reverse_channels,
                                                    const float* mean, const float* std_scale, int fit, float pad_value, int matrix,
                                                    int full_range);
int         pvhip_input_preprocess_warp_color_f32(const void* src, float* dst, const long long* table, int n, int m, int c, int src_h,
                                                  int src_w, int dst_h, int dst_w, int format, int how, int reverse_channels,
                                                  const float* mean, const float* std_scale, float pad_value, int matrix, int full_range);
/* Addition to ABI v18 (the version number is unchanged: nothing existing changed): projective warps.  Image b of `dst` (n, c, dst_h, dst_w)
 * is frame id of the m frames in `src`, sampled through a 3 x 3 homography: `table` is a device pointer to n x 10 int64
 * (id, Q00, Q01, Q02, Q10, Q11, Q12, Q20, Q21, Q22).  The matrix maps an output pixel index (x, y) to the source position
 * sx = (h00 x + h01 y + h02) / (h20 x + h21 y + h22), sy = (h10 x + h11 y + h12) / (the same denominator), pixel centres at the integers:
 * the one cv2.warpPerspective takes with WARP_INVERSE_MAP.  The host scales each matrix by ONE power of two of its own, which the ratio
 * does not see and the table therefore does not store: with B_r = |h_r0| (dst_w - 1) + |h_r1| (dst_h - 1) + |h_r2| for its three rows r
 * and B = max B_r in [2^(e-1), 2^e), Q = rint(double(h) * 2^(51-e)), ties to even (a matrix with a non-finite value or B == 0 is none).
 * Then |Q_r0| (dst_w - 1) + |Q_r1| (dst_h - 1) + |Q_r2| <= 2^52 for every r -- the limit of a table filled directly as well --, so each
 * linear form below is exact as int64 and as binary64.  Output pixel (y, x) of image b:
 *   NX = Q00 x + Q01 y + Q02,  NY = Q10 x + Q11 y + Q12,  D = Q20 x + Q21 y + Q22          (int64)
 *   TX = floor(double(NX) / double(D) * 65536.0),  TY likewise          (binary64: one correctly rounded division each, no reciprocal
 *                                                                        shared between the two, nothing contracted)
 *   the pixel is pad_value in every channel unless D != 0 and |TX| < 2^47 and |TY| < 2^47 (compares that a NaN fails); else
 *   SX = (int64)TX,  SY = (int64)TY
 * and from SX, SY on the rule of pvhip_input_preprocess_warp_f32 word for word: ix = SX >> 16, fx = float(SX & 0xFFFF) * 2^-16, a tap
 * outside the frame is pad_value, a zero fraction reads no second tap, top, bot and v in fp32 in that order without fma, colour frames
 * converted per tap with the chroma of the pixel's block of the frame, then the reversal and (v - mean[k]) / std_scale[k].  A negative D
 * is a legal denominator: -H is the same map as H; where D changes sign inside an image (the horizon of the map) the pixels with D == 0
 * are the pad and those on either side are sampled.  With (Q20, Q21, Q22) = (0, 0, 2^16) and Q16 coefficients in the first two rows it is
 * the warp entry bit for bit.  In numpy: tests/perspective_ref.py, matched bit for bit.  The table is read on the device only: an image
 * whose id is outside [0, m) is written as quiet NaN, and nothing of `src` is read for it; the device cannot check the limit, so it
 * computes the forms in wrapping unsigned arithmetic and a table beyond it gives other pixels, never a load outside the frames.  `format`,
 * `how`, every other argument and every limit are those of pvhip_input_preprocess_warp_f32 -- table != NULL, m >= 1, format in 0..2,
 * c == 3 for formats 1 and 2, pad_value finite and the rest --; else PVHIP_EINVAL and nothing is launched.  _color_: then matrix and full_range
 * as pvhip_input_preprocess_warp_color_f32 takes them, under its limits.  One launch on the current stream, no allocation. */
int         pvhip_input_preprocess_perspective_f32(const void* src, float* dst, const long long* table, int n, int m, int c, int src_h,
                                                   int src_w, int dst_h, int dst_w, int format, int how, int reverse_channels,
                                                   const float* mean, const float* std_scale, float pad_value);
int         pvhip_input_preprocess_perspective_color_f32(const void* src, float* dst, const long long* table, int n, int m, int c,
                                                         int src_h, int src_w, int dst_h, int dst_w, int format, int how,
                                                         int reverse_channels, const float* mean, const float* std_scale,
                                                         float pad_value, int matrix, int full_range);
/* Addition to ABI v18 (the version number is unchanged: nothing existing changed): the table of the warp entry above made on the device
 * from a landmark network's points, so that a cascade aligns its crops without reading them on the host.  Row b of the n x 7 int64
 * `table` becomes the least-squares similarity, without reflection, from the K points of a template onto the K landmarks of row b -- which
 * is directly the inverse map a warp takes: an output pixel at a template point reads the frame at the landmark.
 * All of it is binary64, every operation rounded once, in the order written, nothing contracted.
 *   `tmpl`, 2 K + 3 doubles the host makes once of the template's points (t_ix, t_iy), output pixel indices with centres at the integers:
 *     tbx = (t_0x + t_1x + ...) / K in index order, tby likewise;  cx_i = t_ix - tbx,  cy_i = t_iy - tby;
 *     S = sum over i of (cx_i cx_i + cy_i cy_i), each term formed first and then added in index order, starting from term 0;
 *     every value finite, |t| <= 2^24 and S != 0;  laid out as (tbx, tby, S, cx_0, cy_0, cx_1, cy_1, ...).
 *   `points`, fp32 (rows, 2 K) as x0, y0, x1, y1, ..., normalised to the row's region on pixel-edge coordinates: 0 is the region's left
 *     or top edge, 1 its right or bottom edge.  `regions`: int32 (rows, 5), row b = (id, x, y, w, h) as the _roi_ entries take it; NULL:
 *     row b's region is the whole frame, (m == 1 ? 0 : b, 0, 0, src_w, src_h).
 *   Row b is void when b >= rows, id is outside [0, m), w or h is outside [1, 2^24], or one of its 2 K values is not finite.  Else
 *     px_i = (double(x) + double(u_i) double(w)) - 0.5,  py_i likewise with y and h          (frame pixels, centres at the integers)
 *     mx = (px_0 + px_1 + ...) / K,  my likewise;   dx_i = px_i - mx,  dy_i = py_i - my
 *     A = sum of (cx_i dx_i + cy_i dy_i),  B = sum of (cx_i dy_i - cy_i dx_i), each term formed first and then added, in index order
 *     a = A / S,  b = B / S;   c0 = mx - (a tbx - b tby),  c1 = my - (b tbx + a tby)
 *     the matrix is [[a, -b, c0], [b, a, c1]] and its Q16 coefficients rint(v 65536), ties to even, A01 = rint(-b 65536).
 *   The row is void as well when one of the six is not finite, when one breaks the limits of the warp entry (|A| <= 2^26, |C| <= 2^40), or
 *   when A00 == 0 and A10 == 0 (every point in one place).  A valid row is (id, A00, A01, C0, A10, A11, C1), a void one
 *   (-1, 0, 0, 0, 0, 0, 0) -- which the warp entry writes as quiet NaN, reading nothing for it.  valid[b] = 1 or 0 for b < n, and
 *   valid[n] = the number of valid rows (a second launch of one wave: nothing is added atomically).
 * The fit minimises sum |M t_i - p_i|^2 over the landmarks' space; cv2.estimateAffinePartial2D of landmarks -> template, inverted,
 * minimises in the template's space: the two agree where the fit is exact.  In Python floats: pyopenvino_amd/landmarks.py; in numpy:
 * tests/landmark_warps_ref.py; matched bit for bit.  One thread per row, 64 per workgroup, on the current stream, no allocation.
 * No NULL pointer but `regions`, n, rows, m >= 1, K in [2, 32], src_h, src_w in [1, 2^24], points / regions / valid 4-byte and tmpl /
 * table 8-byte aligned; else PVHIP_EINVAL and nothing is launched. */
int         pvhip_landmarks_to_warps(const float* points, const int* regions, const double* tmpl, long long* table, int* valid, int n,
                                     int rows, int k, int m, int src_h, int src_w);

#ifdef __cplusplus
}
#endif
#endif /* PVHIP_H */
