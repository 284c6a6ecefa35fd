// A detector's answer on the device: DetectionOutput records become one flat table of (image, rectangle, label, score, record) rows -- what
// the reference's sample makes on the host with `for record in res.reshape(100, 7): if conf > 0.5: ...` after reading every record back.
// include/pvhip.h states the rule (pvhip_detections_compact), tests/detections_ref.py is the same in numpy; the screen and the rectangle
// are pvhip_detect_rule.h's, shared with pvhip_detections_to_rois.
//
// A latency kernel (12 800 records at batch 128), parallel over images: one wave per image, kBlock / 64 images per workgroup, no LDS.
//   walk    a wave takes its image in chunks of 64 records, one per lane.  The ballot of "column 0 is not >= 0" finds the list end: lanes
//           behind its first set bit are dead and the wave stops after that chunk.  The ballot of `keep` with mbcnt ranks the chunk's
//           survivors behind those of the chunks before.
//   count   writes selected[b] and counts[b] = min(selected[b], cap).
//   write   a second launch behind the first on the same stream, so every count is there: the wave sums counts[0..b) (lane-strided loads,
//           a wave reduction), walks its image again and stores survivor `rank` < cap at row base + rank in two 16-byte stores.  The last
//           image's wave writes total.
// No wave waits for another one, nothing is added atomically: every output word has one writer and its value depends on the records alone.
#include "pvhip_common.h"
#include "pvhip_detect_rule.h"

using namespace pvhip;

namespace {

struct CompactArgs {
    ScreenWalk walk;       // the records [N * P][7] and the screen
    int*       header;     // counts[N], selected[N], total
    int4*      rows;       // [N * min(P, cap)][2]
    int N, H, W, cap;
    DetectionFit fit;      // FIT kernels: the geometry of the detector's fitted input
};

constexpr int kImagesPerBlock = kBlock / kWave;

template <bool FIT>
__global__ __launch_bounds__(kBlock) void detections_count_kernel(CompactArgs a) {
    const int b = blockIdx.x * kImagesPerBlock + (threadIdx.x >> 6);
    if (b >= a.N) return;                                                       // (the whole wave: nothing below meets a barrier)
    const int selected = walk_image<FIT>(a.walk, b, a.H, a.W, a.walk.P, [](int, int, const DetectionRect&, const float*) {}, a.fit);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        a.header[b]       = min(selected, a.cap);
        a.header[a.N + b] = selected;
    }
}

template <bool FIT>
__global__ __launch_bounds__(kBlock) void detections_write_kernel(CompactArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int b    = blockIdx.x * kImagesPerBlock + (threadIdx.x >> 6);
    if (b >= a.N) return;
    int base = 0;                                                               // rows of the images before b (<= N * P: an int)
    for (int i = lane; i < b; i += kWave) base += a.header[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) base += __shfl_xor(base, m, kWave);
    const int count = a.header[b];
    if (count > 0) {
        int4* out = a.rows + 2 * (size_t)base;
        walk_image<FIT>(a.walk, b, a.H, a.W, count, [&](int rank, int r, const DetectionRect& rect, const float* q) {
            out[2 * rank + 0] = make_int4(b, rect.x0, rect.y0, rect.w);
            out[2 * rank + 1] = make_int4(rect.h, detection_label(q[1]), (int)__float_as_uint(q[2]), r);
        }, a.fit);
    }
    if (b == a.N - 1 && lane == 0) a.header[2 * a.N] = base + count;
}

// The one launcher; fit: NULL, or the geometry of the _fit entry.
int compact_launch(const float* records, int images, int records_per_image, int frame_h, int frame_w, float min_confidence,
                   const int* labels, int num_labels, int min_h, int min_w, int max_per_image, int* header, int* rows,
                   const DetectionFit* fit) {
    PVHIP_REQUIRE_INIT();
    PVHIP_CHECK_ARG(fit == nullptr || detection_fit_ok(*fit));
    PVHIP_CHECK_ARG(records != nullptr && header != nullptr && rows != nullptr);
    PVHIP_CHECK_ARG(((uintptr_t)rows & 15u) == 0 && ((uintptr_t)header & 3u) == 0 && ((uintptr_t)records & 3u) == 0);
    PVHIP_CHECK_ARG(images >= 1 && records_per_image >= 1 && min_h >= 1 && min_w >= 1 && max_per_image >= 1);
    PVHIP_CHECK_ARG((long long)images * records_per_image < ((1LL << 31) / 7));
    PVHIP_CHECK_ARG(frame_h >= 1 && frame_h <= (1 << 24) && frame_w >= 1 && frame_w <= (1 << 24));   // exact as fp32
    PVHIP_CHECK_ARG(num_labels >= 0 && num_labels <= kScreenLabels && (num_labels == 0 || labels != nullptr));   // (NULL: any label)
    CompactArgs a;
    a.walk = ScreenWalk{records, labels, records_per_image, num_labels, min_h, min_w, min_confidence};
    a.header = header; a.rows = reinterpret_cast<int4*>(rows);
    a.N = images; a.H = frame_h; a.W = frame_w; a.cap = max_per_image;
    a.fit = fit != nullptr ? *fit : DetectionFit{};
    const dim3 grid((images + kImagesPerBlock - 1) / kImagesPerBlock);
    if (fit != nullptr) {
        hipLaunchKernelGGL(detections_count_kernel<true>, grid, dim3(kBlock), 0, state().stream, a);
        hipLaunchKernelGGL(detections_write_kernel<true>, grid, dim3(kBlock), 0, state().stream, a);
    } else {
        hipLaunchKernelGGL(detections_count_kernel<false>, grid, dim3(kBlock), 0, state().stream, a);
        hipLaunchKernelGGL(detections_write_kernel<false>, grid, dim3(kBlock), 0, state().stream, a);
    }
    PVHIP_LAUNCH_CHECK();
    return PVHIP_OK;
}

}  // namespace

extern "C" {

int pvhip_detections_compact(const float* records, int images, int records_per_image, int frame_h, int frame_w, float min_confidence,
                             const int* labels, int num_labels, int min_h, int min_w, int max_per_image, int* header, int* rows) {
    return compact_launch(records, images, records_per_image, frame_h, frame_w, min_confidence, labels, num_labels, min_h, min_w,
                          max_per_image, header, rows, nullptr);
}

int pvhip_detections_compact_fit(const float* records, int images, int records_per_image, int frame_h, int frame_w, float min_confidence,
                                 const int* labels, int num_labels, int min_h, int min_w, int max_per_image, int* header, int* rows,
                                 int net_h, int net_w, int dx, int dy, int iw, int ih) {
    const DetectionFit g{net_h, net_w, dx, dy, iw, ih};
    return compact_launch(records, images, records_per_image, frame_h, frame_w, min_confidence, labels, num_labels, min_h, min_w,
                          max_per_image, header, rows, &g);
}

}  // extern "C"
