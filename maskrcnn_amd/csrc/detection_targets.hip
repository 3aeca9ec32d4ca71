// Detection training targets: model.mrn_samples (model.py:396-576) for a batch of images, in two entry points. The rule is stated
// at mrcnn_detection_targets in include/maskrcnn_hip.h.
//
//   mrcnn_detection_targets   steps 1-6: crowd rule, fp32 IoU of every RoI against every kept row, first argmax (target_match.hpp,
//                             shared with csrc/targets.hip), the classes, the positives and negatives with the smallest
//                             (key, roi index), boxes_deltas in fp32 with an fp64 log.
//   mrcnn_mask_targets_*      step 7: crop_and_resize of the matched row's mask with the RoI as the box (the arithmetic of
//                             csrc/crop.hip: crop_math.hpp), rounded to nearest even.
//
// detection_targets. ONE workgroup of 1024 lanes per image, one launch for the batch. The image's rows (box, class id) are staged
// in LDS, 20 KB at the 1024-row limit. A lane takes RoIs tid, tid + 1024, ... (N <= 4096), walks the rows keeping max / first
// argmax / crowd max, and forms ONE 64-bit sort key per RoI:
//     class (0 positive, 1 negative, 2 neither) << 53 | key (31 bits) << 22 | roi index (12 bits) << 10 | matched row (10 bits)
// The RoI index is unique, so the row bits never decide an order: they ride along and spare a second table. One LDS bitonic sort
// (workgroup.hpp) of the next power of two >= N keys (32 KB at 4096; the padding is all ones and sorts last) yields the positives and then the
// negatives, each in (key, roi index) order; the class counts P and Q come from LDS atomics. Slot s < num_pos reads sorted entry
// s, slot num_pos <= s < num_pos + num_neg reads entry P + (s - num_pos), every other slot is written as zeros / -1: the kernel
// writes every byte of its outputs, so there is no memset. neg_limit is evaluated on the device in fp64 (the file is built with
// contraction off: the product and the difference are rounded separately, as Python's int(r * p - p)).
//
// mask_targets. Grid (slot, image); 256 lanes. The crop's row and column samples go to LDS once, a lane then owns output pixels
// p, p + 256, ... (x fastest: coalesced stores, neighbouring taps share cache lines). Slots >= num_pos write zeros. The mask row
// is found through gt_off[b] + gt_index[s] and its offset is computed in 64 bits (33 rows of 8192 x 8192 bytes pass 2^31).
//
// Every index is checked where it is used: row offsets are clamped into [0, num_rows] and to 1024 rows an image, a decoded RoI
// index is compared with N, a row index with the image's row count, num_pos with count. Nothing here synchronises with the host.
#pragma clang fp contract(off)

#include "common.hpp"
#include "crop_math.hpp"
#include "target_match.hpp"
#include "workgroup.hpp"

namespace {

using namespace mrcnn_match;

constexpr int kBlock = 1024;               // detection_targets: one workgroup per image
constexpr int kMaskBlock = 256;
constexpr int kMaxRois = 4096;             // RoIs of one image (LDS sort; 12 bits of the sort key)
constexpr int kMaxCount = 1024;
constexpr int kMaxMaskSide = 64;
constexpr int kMaxImageSide = 16384;
constexpr int kRowBits = 10, kRoiBits = 12, kKeyBits = 31;
static_assert(kMaxRows == 1 << kRowBits && kMaxRois == 1 << kRoiBits, "the sort key's row and RoI fields");
constexpr int kClassShift = kRowBits + kRoiBits + kKeyBits;
constexpr unsigned long long kPadding = ~0ull;

struct TargetParams {
    const float* rois;
    const float* boxes;
    const int32_t* ids;
    const int32_t* gt_off;
    const int32_t* keys;
    int32_t n, m, count, pos_limit;
    double r;                 // 1.0 / positive_ratio
    float pos_iou, crowd_iou;
    float std_dev[4];
    float* rois_out;
    int32_t* class_ids;
    float* deltas;
    int32_t* roi_index;
    int32_t* gt_index;
    int32_t* num_pos;
    int32_t* num_neg;
    int32_t* status;
};

__global__ __launch_bounds__(kBlock) void detection_targets_kernel(TargetParams p) {
    __shared__ float4 s_box[kMaxRows];
    __shared__ int s_id[kMaxRows];
    __shared__ unsigned long long s_key[kMaxRois];
    __shared__ int s_count[2];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const Rows r = image_rows(p.gt_off, b, p.m);
    int crowd = 0;
    for (int i = tid; i < r.n; i += kBlock) {
        const float* g = p.boxes + 4 * (int64_t)(r.start + i);
        const int id = p.ids[r.start + i];
        s_box[i] = make_float4(g[0], g[1], g[2], g[3]);
        s_id[i] = id;
        crowd |= id < 0;
    }
    if (tid < 2) s_count[tid] = 0;
    crowd = __syncthreads_or(crowd);          // also: the rows are staged
    int kept = 0;
    for (int i = tid; i < r.n; i += kBlock) kept |= row_kept(s_id[i], crowd != 0);
    kept = __syncthreads_or(kept);

    int sort_n = 1;
    while (sort_n < p.n) sort_n <<= 1;        // <= kMaxRois
    int n_pos = 0, n_neg = 0;
    if (kept) {
        const float* rois = p.rois + 4 * (int64_t)b * p.n;
        const int32_t* keys = p.keys + (int64_t)b * p.n;
        int my_pos = 0, my_neg = 0;
        for (int i = tid; i < sort_n; i += kBlock) {
            unsigned long long key = kPadding;
            if (i < p.n) {
                const float4 roi = make_float4(rois[4 * i], rois[4 * i + 1], rois[4 * i + 2], rois[4 * i + 3]);
                const float a_area = box_area(roi);
                Match walk;
                for (int g = 0; g < r.n; ++g) {
                    const float4 box = s_box[g];
                    const float iou = box_iou(roi, a_area, box, box_area(box));
                    const int id = s_id[g];
                    if (row_kept(id, crowd != 0)) walk.kept_row(g, iou);
                    else if (id < 0) walk.crowd_row(iou);
                }
                unsigned long long cls = 2ull;
                if (walk.arg >= 0) {
                    if (walk.best >= p.pos_iou) cls = 0ull;
                    else if (walk.best < p.pos_iou && walk.crowd_max < p.crowd_iou) cls = 1ull;
                }
                my_pos += cls == 0ull;
                my_neg += cls == 1ull;
                key = (cls << kClassShift) | ((unsigned long long)((uint32_t)keys[i] & 0x7fffffffu) << (kRowBits + kRoiBits)) |
                      ((unsigned long long)(uint32_t)i << kRowBits) | (unsigned long long)(uint32_t)max(walk.arg, 0);
            }
            s_key[i] = key;
        }
        if (my_pos) atomicAdd(&s_count[0], my_pos);
        if (my_neg) atomicAdd(&s_count[1], my_neg);
        mrcnn::bitonic_sort<kBlock, false>(s_key, sort_n);   // its barriers publish s_count too (one barrier when sort_n == 1)
        n_pos = min(s_count[0], p.n);
        n_neg = min(s_count[1], p.n - n_pos);
    }
    const int num_pos = min(n_pos, p.pos_limit);
    int num_neg = 0;
    if (num_pos > 0) {
        double t = p.r * (double)num_pos;     // int(r * positive_count - positive_count): two roundings, then truncation
        t = t - (double)num_pos;
        const int room = p.count - num_pos;
        const int limit = t >= (double)room ? room : (t > 0.0 ? (int)t : 0);
        num_neg = min(n_neg, limit);
    }
    if (tid == 0) {
        p.num_pos[b] = num_pos;
        p.num_neg[b] = num_neg;
        p.status[b] = kept ? 0 : 1;
    }
    for (int s = tid; s < p.count; s += kBlock) {
        float4 roi = make_float4(0.f, 0.f, 0.f, 0.f), delta = roi;
        int cls_id = 0, ri = -1, gi = -1;
        if (s < num_pos + num_neg) {
            const bool positive = s < num_pos;
            const int e = positive ? s : n_pos + (s - num_pos);          // < n_pos + n_neg <= N <= sort_n
            const unsigned long long key = s_key[e];
            const int i = (int)((key >> kRowBits) & ((1u << kRoiBits) - 1u));
            const int g = (int)(key & ((1u << kRowBits) - 1u));
            if (i < p.n) {
                const float* a = p.rois + 4 * ((int64_t)b * p.n + i);
                roi = make_float4(a[0], a[1], a[2], a[3]);
                ri = i;
                if (positive && g < r.n) {
                    const float4 gt = s_box[g];
                    gi = g;
                    cls_id = s_id[g];
                    // boxes_deltas (data.py:103-121) on fp32 tensors
                    const float h = roi.z - roi.x, w = roi.w - roi.y;
                    const float cy = roi.x + 0.5f * h, cx = roi.y + 0.5f * w;
                    const float gt_h = gt.z - gt.x, gt_w = gt.w - gt.y;
                    const float gt_cy = gt.x + 0.5f * gt_h, gt_cx = gt.y + 0.5f * gt_w;
                    const float dy = (gt_cy - cy) / h, dx = (gt_cx - cx) / w;
                    const float dh = (float)log((double)(gt_h / h)), dw = (float)log((double)(gt_w / w));
                    delta = make_float4(dy / p.std_dev[0], dx / p.std_dev[1], dh / p.std_dev[2], dw / p.std_dev[3]);
                }
            }
        }
        const int64_t o = (int64_t)b * p.count + s;
        float* ro = p.rois_out + 4 * o;
        float* dl = p.deltas + 4 * o;
        ro[0] = roi.x; ro[1] = roi.y; ro[2] = roi.z; ro[3] = roi.w;
        dl[0] = delta.x; dl[1] = delta.y; dl[2] = delta.z; dl[3] = delta.w;
        p.class_ids[o] = cls_id;
        p.roi_index[o] = ri;
        p.gt_index[o] = gi;
    }
}

__device__ __forceinline__ float mask_value(const uint8_t* m, int64_t i) { return (float)m[i]; }
__device__ __forceinline__ float mask_value(const float* m, int64_t i) { return m[i]; }

template <typename T>
__global__ __launch_bounds__(kMaskBlock) void mask_targets_kernel(const T* masks, int m, int H, int W, const int32_t* gt_off,
                                                                  int count, const float* rois_out, const int32_t* gt_index,
                                                                  const int32_t* num_pos, int mh, int mw, float* out) {
    __shared__ mrcnn_crop::Sample s_y[kMaxMaskSide], s_x[kMaxMaskSide];
    const int tid = (int)threadIdx.x, s = (int)blockIdx.x, b = (int)blockIdx.y;
    const int plane = mh * mw;
    const int64_t slot = (int64_t)b * count + s;
    float* o = out + slot * plane;
    const Rows r = image_rows(gt_off, b, m);
    const int np = min(max(num_pos[b], 0), count);
    const int g = s < np ? gt_index[slot] : -1;
    if (g < 0 || g >= r.n) {                               // the same for the whole workgroup
        for (int e = tid; e < plane; e += kMaskBlock) o[e] = 0.f;
        return;
    }
    const float* box = rois_out + 4 * slot;
    const float y1 = box[0], x1 = box[1], y2 = box[2], x2 = box[3];
    for (int t = tid; t < mh + mw; t += kMaskBlock) {
        if (t < mh) s_y[t] = mrcnn_crop::make_sample(y1, y2, H, mh, t);
        else s_x[t - mh] = mrcnn_crop::make_sample(x1, x2, W, mw, t - mh);
    }
    __syncthreads();
    const T* img = masks + (int64_t)(r.start + g) * H * W;
    for (int e = tid; e < plane; e += kMaskBlock) {
        const mrcnn_crop::Sample Y = s_y[e / mw], X = s_x[e % mw];
        float v = 0.f;                                     // extrapolation value 0
        if (Y.inside && X.inside) {
            // 0 <= lo <= hi <= size - 1 for a finite box; a NaN box passes the inside test, so the taps are clamped all the same
            const int ylo = min(max(Y.lo, 0), H - 1), yhi = min(max(Y.hi, 0), H - 1);
            const int xlo = min(max(X.lo, 0), W - 1), xhi = min(max(X.hi, 0), W - 1);
            const int64_t top = (int64_t)ylo * W, bot = (int64_t)yhi * W;
            v = mrcnn_crop::bilerp(mask_value(img, top + xlo), mask_value(img, top + xhi), mask_value(img, bot + xlo),
                                   mask_value(img, bot + xhi), X.lerp, Y.lerp);
        }
        o[e] = rintf(v);                                   // torch.round: ties to even
    }
}

template <typename T>
int mask_targets(const char* who, const T* gt_masks, int32_t num_rows, int32_t height, int32_t width, const int32_t* gt_off,
                 int32_t batch, int32_t count, const float* rois_out, const int32_t* gt_index, const int32_t* num_pos,
                 int32_t mask_height, int32_t mask_width, float* target_mask, mrcnn_stream_t stream) {
    if (int rc = check_rows(who, num_rows, batch)) return rc;
    MRCNN_REQUIRE(count >= 1 && count <= kMaxCount, "%s: count=%d must be in [1, %d]", who, count, kMaxCount);
    MRCNN_REQUIRE(height >= 1 && height <= kMaxImageSide && width >= 1 && width <= kMaxImageSide,
                  "%s: masks of %d x %d; height and width must be in [1, %d]", who, height, width, kMaxImageSide);
    MRCNN_REQUIRE(mask_height >= 1 && mask_height <= kMaxMaskSide && mask_width >= 1 && mask_width <= kMaxMaskSide,
                  "%s: targets of %d x %d; mask_height and mask_width must be in [1, %d]", who, mask_height, mask_width, kMaxMaskSide);
    MRCNN_REQUIRE(gt_off && rois_out && gt_index && num_pos && target_mask, "%s: null pointer", who);
    MRCNN_REQUIRE(num_rows == 0 || gt_masks, "%s: null pointer", who);
    hipLaunchKernelGGL(mask_targets_kernel<T>, dim3((unsigned)count, (unsigned)batch), dim3(kMaskBlock), 0, mrcnn::as_stream(stream),
                       gt_masks, num_rows, height, width, gt_off, count, rois_out, gt_index, num_pos, mask_height, mask_width,
                       target_mask);
    return mrcnn::check_launch(who);
}

}  // namespace

extern "C" int mrcnn_detection_targets(const float* rois, const float* gt_boxes, const int32_t* gt_class_ids, const int32_t* gt_off,
                                       const int32_t* keys, int32_t batch, int32_t num_rois, int32_t num_rows, int32_t count,
                                       double positive_ratio, float pos_iou, float crowd_iou, const float std_dev[4],
                                       float* rois_out, int32_t* target_class_ids, float* target_deltas, int32_t* roi_index,
                                       int32_t* gt_index, int32_t* num_pos, int32_t* num_neg, int32_t* status,
                                       mrcnn_stream_t stream) {
    const char* who = "detection_targets";
    if (int rc = check_rows(who, num_rows, batch)) return rc;
    MRCNN_REQUIRE(num_rois >= 1 && num_rois <= kMaxRois, "%s: num_rois=%d must be in [1, %d]", who, num_rois, kMaxRois);
    MRCNN_REQUIRE(count >= 1 && count <= kMaxCount, "%s: count=%d must be in [1, %d]", who, count, kMaxCount);
    MRCNN_REQUIRE(positive_ratio > 0.0 && positive_ratio <= 1.0, "%s: positive_ratio=%g must be in (0, 1]", who, positive_ratio);
    MRCNN_REQUIRE(rois && gt_off && keys && std_dev && rois_out && target_class_ids && target_deltas && roi_index && gt_index &&
                      num_pos && num_neg && status, "%s: null pointer", who);
    MRCNN_REQUIRE(num_rows == 0 || (gt_boxes && gt_class_ids), "%s: null pointer", who);
    TargetParams p;
    p.rois = rois; p.boxes = gt_boxes; p.ids = gt_class_ids; p.gt_off = gt_off; p.keys = keys;
    p.n = num_rois; p.m = num_rows; p.count = count;
    p.pos_limit = (int32_t)((double)count * positive_ratio);          // int(TRAIN_ROIS_PER_IMAGE * ROI_POSITIVE_RATIO)
    p.r = 1.0 / positive_ratio;
    p.pos_iou = pos_iou; p.crowd_iou = crowd_iou;
    for (int i = 0; i < 4; ++i) p.std_dev[i] = std_dev[i];
    p.rois_out = rois_out; p.class_ids = target_class_ids; p.deltas = target_deltas; p.roi_index = roi_index;
    p.gt_index = gt_index; p.num_pos = num_pos; p.num_neg = num_neg; p.status = status;
    hipLaunchKernelGGL(detection_targets_kernel, dim3((unsigned)batch), dim3(kBlock), 0, mrcnn::as_stream(stream), p);
    return mrcnn::check_launch(who);
}

extern "C" int mrcnn_mask_targets_u8(const uint8_t* gt_masks, int32_t num_rows, int32_t height, int32_t width, const int32_t* gt_off,
                                     int32_t batch, int32_t count, const float* rois_out, const int32_t* gt_index,
                                     const int32_t* num_pos, int32_t mask_height, int32_t mask_width, float* target_mask,
                                     mrcnn_stream_t stream) {
    return mask_targets("mask_targets_u8", gt_masks, num_rows, height, width, gt_off, batch, count, rois_out, gt_index, num_pos,
                        mask_height, mask_width, target_mask, stream);
}

extern "C" int mrcnn_mask_targets_f32(const float* gt_masks, int32_t num_rows, int32_t height, int32_t width, const int32_t* gt_off,
                                      int32_t batch, int32_t count, const float* rois_out, const int32_t* gt_index,
                                      const int32_t* num_pos, int32_t mask_height, int32_t mask_width, float* target_mask,
                                      mrcnn_stream_t stream) {
    return mask_targets("mask_targets_f32", gt_masks, num_rows, height, width, gt_off, batch, count, rois_out, gt_index, num_pos,
                        mask_height, mask_width, target_mask, stream);
}
