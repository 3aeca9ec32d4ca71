/* maskrcnn_hip.h — C ABI of libmaskrcnn_hip.so: the MI355X (gfx950) implementation of the
 * Mask R-CNN inference hot path of delldu/MaskRCNN.
 *
 * This is the drop-in boundary. Every entry point takes plain device pointers, sizes and a HIP stream
 * (no torch types), launches asynchronously on that stream, performs no allocation and no host
 * synchronisation (safe inside hipGraph capture), and returns MRCNN_OK or a negative error code with
 * a thread-local message in mrcnn_last_error(). Nothing here ever calls exit().
 *
 * Each declaration cites the reference interface it replaces (paths relative to the reference tree).
 * The Python face (package `maskrcnn`: nms, CropFunction, _C.{nms,crop_forward,crop_backward}, and
 * torch.ops.maskrcnn.*) is a thin binding over these symbols: see INTEGRATION.md.
 */
#ifndef MASKRCNN_HIP_H
#define MASKRCNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRCNN_ABI_VERSION 38 /* 38: mrcnn_resize_u8_route, mrcnn_paste_masks_store_width */

#define MRCNN_OK 0
#define MRCNN_ERR_INVALID_ARGUMENT (-1) /* bad shape / null pointer / unsupported size          */
#define MRCNN_ERR_UNSUPPORTED (-2)      /* valid request this build has no kernel for            */
#define MRCNN_ERR_LAUNCH (-3)           /* hipLaunch / runtime error (message has hipGetErrorString) */

typedef void* mrcnn_stream_t; /* a hipStream_t; NULL = the null stream */

/* ABI version of the loaded library (== MRCNN_ABI_VERSION it was built with). */
int mrcnn_abi_version(void);
/* Message for the last non-OK return on this thread ("" if none). Never NULL. */
const char* mrcnn_last_error(void);
/* gfx target the device code was compiled for ("gfx950"). */
const char* mrcnn_arch(void);

/* ------------------------------------------------------------------------------------------------
 * NMS — replaces  at::Tensor nms(const at::Tensor& dets, const float threshold)
 *       c++ext/maskrcnn/csrc/nms.h:15-30, cpu path csrc/cpu/nms_cpu.cpp:11-79.
 *
 * Greedy NMS with the CPU path's exact arithmetic: areas (x2-x1+1)*(y2-y1+1), boxes visited in
 * descending score order (ties: lower input index first), box j suppressed by a kept box i when
 * inter/(area_i+area_j-inter) >= threshold (IEEE fp32, no FMA contraction; `>=`, not the CUDA
 * path's `>`). Survivors are reported as ASCENDING INPUT INDICES (nms_cpu.cpp:69).
 *
 * S independent segments are processed by one launch (one workgroup per segment).
 *   dets        [S][n_max] rows (y1,x1,y2,x2,score); element (s,i,c) at
 *               dets[s*seg_stride + i*row_stride + c*col_stride]   (strides in elements)
 *   seg_counts  int32[S] boxes in each segment, device memory; NULL = all n_max. An entry outside [0, n_max] is clamped
 *               into it (a negative count is 0 boxes, a count above n_max is n_max); rows at and past the count are never read
 *   class_ids   int32, element (s,i) at class_ids[s*n_max + i]; NULL = single class. When given,
 *               a box only suppresses boxes of the same class: the one-pass form of the per-class
 *               loop in MaskRCNN.mrn_refine (model.py:1454-1475).
 *   keep_out    int64[S][n_max]: first counts_out[s] entries = kept indices ascending, rest = -1
 *   counts_out  int32[S]
 *   workspace   optional device scratch of >= mrcnn_nms_workspace_bytes(S, n_max) bytes, 16-byte aligned.
 *               NULL: one LDS-resident workgroup per segment does everything (one launch, no scratch).
 *               Given (and n_max > 128): the pair tests are spread over the whole chip (sort → 64x64 pair-mask
 *               tiles → serial scan), 3 launches, several times faster at n_max >= 500. Same results.
 * Limits: 1 <= n_max <= mrcnn_nms_max_boxes() = 16384 with a workspace, 4096 without.  S >= 1.
 * ---------------------------------------------------------------------------------------------- */
int64_t mrcnn_nms_max_boxes(void);
size_t mrcnn_nms_workspace_bytes(int32_t num_segments, int64_t n_max);
int mrcnn_nms_batched_f32(const float* dets, int32_t num_segments, int64_t n_max, int64_t seg_stride,
                          int64_t row_stride, int64_t col_stride, const int32_t* seg_counts,
                          const int32_t* class_ids, float threshold, int64_t* keep_out,
                          int32_t* counts_out, void* workspace, size_t workspace_bytes,
                          mrcnn_stream_t stream);
/* What mrcnn_nms_batched_f32 launches for this n_max — the launcher's own answer (it launches from the same function), host
 * arithmetic only, no device needed. has_workspace: whether a workspace pointer is passed. n_max as limited above.
 *   plan_out[0] path: 0 the single LDS-resident launch (nms_kernel), 1 sort → pair mask → scan on the workspace
 *   plan_out[1] boxes the LDS kernel (path 0) / the sort kernel (path 1) is instantiated for: 256, 1024, 2048, 4096 (8192, 16384)
 *   plan_out[2] threads of that kernel's workgroup (256 or 1024)
 *   plan_out[3] path 1: 1 when the scan holds the segment's column words in LDS, 0 when it reads them from L2; path 0: 0 */
int mrcnn_nms_plan(int64_t n_max, int32_t has_workspace, int32_t plan_out[4]);

/* The rest of the reference's nms surface: ANY number of boxes, and float64 boxes (cpu/nms_cpu.cpp:73-79 dispatches over the
 * floating types; nms.h:15 takes a float threshold either way). One segment; arithmetic in the boxes' own type; the same
 * visiting order (descending score, ties by ascending index) and `>=` rule → the same keep set as the CPU path. No O(N^2)
 * memory: radix sort (hipCUB), then one launch per 64-box chunk of the order (csrc/nms_general.hip).
 *   dets        dtype 0: float32, 1: float64; box r = (y1,x1,y2,x2,score) at dets[r*row_stride + c*col_stride] (elements)
 *   keep_out    int64[n]: first *count_out entries = kept input indices ascending, rest = -1;  count_out: int64[1] (device)
 *   workspace   >= mrcnn_nms_general_workspace_bytes(n, dtype) bytes, 256-byte aligned.   1 <= n <= 2^31 - 65. */
size_t mrcnn_nms_general_workspace_bytes(int64_t n, int32_t dtype);
int mrcnn_nms_general(const void* dets, int32_t dtype, int64_t n, int64_t row_stride, int64_t col_stride, float threshold,
                      int64_t* keep_out, int64_t* count_out, void* workspace, size_t workspace_bytes,
                      mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * crop_and_resize ("RoIAlign") forward — replaces
 *   void crop_forward(image, boxes, box_index, extrapolation_value, crop_height, crop_width, crops)
 *   c++ext/maskrcnn/csrc/crop.h:14-34, cpu path csrc/cpu/crop_cpu.cpp:13-164.
 *
 *   image      fp32 [batch][depth][H][W]   (NCHW, contiguous)
 *   boxes      fp32 [num_boxes][4] normalised (y1,x1,y2,x2)
 *   box_index  int32[num_boxes] in [0,batch). An out-of-range index fills that box's crop with
 *              extrapolation_value (the reference CPU path printf()s and exit(-1)s, crop_cpu.cpp:47-50;
 *              its CUDA path silently skips, crop_cuda.cu:41-44).
 *   crops      fp32 [num_boxes][depth][crop_height][crop_width], fully overwritten.
 * Arithmetic is the reference's, op for op (one bilinear sample per bin, endpoint-inclusive grid,
 * strict outside test, floorf/ceilf taps, a+(b-a)*t lerps, crop size 1 → box centre in double).
 * ---------------------------------------------------------------------------------------------- */
int mrcnn_crop_forward_f32(const float* image, int32_t batch, int32_t depth, int32_t height,
                           int32_t width, const float* boxes, const int32_t* box_index,
                           int32_t num_boxes, float extrapolation_value, int32_t crop_height,
                           int32_t crop_width, float* crops, mrcnn_stream_t stream);
/* What mrcnn_crop_forward_f32 launches for these arguments — the launcher's own answer (it launches from the same function),
 * host arithmetic only, no device needed. image / crops are looked at for their 16-byte alignment only; num_boxes >= 1.
 *   plan_out[0] route: 1 the LDS-staged kernel (crop_forward_nchw_staged), 0 the gather kernel (crop_forward_nchw)
 *   plan_out[1] channels per wave (staged) / per workgroup (gather)      plan_out[2] channel slabs = ceil(depth / [1])
 *   plan_out[3] workgroup numbering of the staged kernel: 0 grid (box, slab), 1 / 2 the XCD-local 1-D grids (csrc/crop.hip)
 *   plan_out[4] 16-byte slots of a wave's LDS-DMA ring (0 on the gather route)      plan_out[5] dynamic LDS bytes
 * The process's tuning switches (MRCNN_CROP_STAGED / _CPW / _MAP / _RING, read once) are part of the answer. */
int mrcnn_crop_forward_plan(const float* image, const float* crops, int32_t depth, int32_t height, int32_t width,
                            int32_t num_boxes, int32_t crop_height, int32_t crop_width, int32_t plan_out[6]);

/* crop_and_resize backward — replaces
 *   void crop_backward(grads, boxes, box_index, grads_image)
 *   c++ext/maskrcnn/csrc/crop.h:36-53, cpu path csrc/cpu/crop_cpu.cpp:167-265.
 *   grads [num_boxes][depth][crop_h][crop_w] → grads_image [batch][depth][H][W] (zeroed here, then
 *   accumulated with fp32 atomics: summation order differs from the serial CPU loop). */
int mrcnn_crop_backward_f32(const float* grads, const float* boxes, const int32_t* box_index,
                            int32_t num_boxes, int32_t batch, int32_t depth, int32_t height,
                            int32_t width, int32_t crop_height, int32_t crop_width,
                            float* grads_image, mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Pyramid RoIAlign, channels-last — replaces the Python dispatcher
 *   roi_align(inputs, pool_size, image_shape)   model.py:276-393
 * (level = clamp(round_half_even(4 + log2(sqrt(h*w) / (224/sqrt(H_img*W_img)))), 2, 5), one
 * crop_forward per level, concat, restore order) with one launch and no host synchronisation.
 *
 *   fm[l]      fp32 [batch][H_l][W_l][depth]  (NHWC), l = 0..3 for P2..P5; depth % 4 == 0
 *   rois       fp32 [num_rois][4] normalised (y1,x1,y2,x2); roi r reads image roi_batch[r]
 *              (roi_batch NULL → image r / rois_per_image).
 *   out        fp32 [num_rois][pool][pool][depth] (NHWC), original roi order
 *   levels_out int32[num_rois] (optional, may be NULL): the level 2..5 chosen per roi
 * ---------------------------------------------------------------------------------------------- */
int mrcnn_roi_align_pyramid_nhwc_f32(const float* const fm[4], const int32_t fm_h[4],
                                     const int32_t fm_w[4], int32_t batch, int32_t depth,
                                     const float* rois, const int32_t* roi_batch, int32_t num_rois,
                                     int32_t rois_per_image, int32_t pool, float image_area,
                                     float* out, int32_t* levels_out, mrcnn_stream_t stream);
/* The same with a selectable output layout: out_layout = MRCNN_LAYOUT_NHWC (as above), MRCNN_LAYOUT_KBLOCKED
 * ([depth/8][num_rois*pool*pool][8], depth % 8 == 0 — what mrcnn_conv3x3_winograd_f32 reads: the mask head's first
 * conv then needs no layout pass), or MRCNN_LAYOUT_NHWC_F16 (NHWC, each value rounded to fp16 — `out` then points to
 * fp16 storage: the "f16" mode's heads, whose first conv would round the fp32 values the same way). */
int mrcnn_roi_align_pyramid_f32(const float* const fm[4], const int32_t fm_h[4], const int32_t fm_w[4], int32_t batch,
                                int32_t depth, const float* rois, const int32_t* roi_batch, int32_t num_rois,
                                int32_t rois_per_image, int32_t pool, float image_area, void* out, int32_t out_layout,
                                int32_t* levels_out, mrcnn_stream_t stream);
/* The same for the fixed-shape pipeline, whose rois tensor holds rois_per_image SLOTS per image of which only the first
 * roi_counts[image] carry a proposal (model.py:1366-1374: the reference's rois tensor simply ends after the boxes NMS kept):
 * slots beyond the count are skipped — nothing is read, their output rows are left untouched. roi_counts int32 [num_rois /
 * rois_per_image] device memory, or NULL (= mrcnn_roi_align_pyramid_f32); needs roi_batch == NULL. */
int mrcnn_roi_align_pyramid_counted_f32(const float* const fm[4], const int32_t fm_h[4], const int32_t fm_w[4], int32_t batch,
                                        int32_t depth, const float* rois, const int32_t* roi_batch, int32_t num_rois,
                                        int32_t rois_per_image, const int32_t* roi_counts, int32_t pool, float image_area,
                                        void* out, int32_t out_layout, int32_t* levels_out, mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of the pyramid RoIAlign to the four maps — what CropFunction.backward -> crop_backward (crop_cpu.cpp:167-265)
 * amounts to behind roi_align (model.py:276-393), level by level, on channels-last maps and with a FIXED summation order.
 *
 *   grad_out   fp32 [num_rois][pool][pool][depth] (NHWC): the gradient of mrcnn_roi_align_pyramid_counted_f32's NHWC output
 *   grad_fm[l] fp32 [batch][H_l][W_l][depth] (NHWC), l = 0..3 for P2..P5, 16-byte aligned. EVERY byte is written by the call
 *              (a pixel nothing reaches is +0): the caller does not zero the buffers.
 *   rois, roi_batch, num_rois, rois_per_image, roi_counts, pool, image_area: exactly as in the forward; the same limits
 *              (depth % 4 == 0, 1 <= pool <= 1024). The level of a RoI is the forward's (one function, csrc/crop_math.hpp).
 *   workspace  >= mrcnn_roi_align_pyramid_backward_workspace_bytes(num_rois) bytes of device memory, 16-byte aligned
 *              (32 bytes per RoI: level, image and footprint). Nothing is allocated by the library.
 *
 * The rule, bit for bit. grad_fm[l][b,y,x,c] starts from +0 and is the fp32 sum of the terms crop_cpu_backward
 * (crop_cpu.cpp:205-263) adds to that element, taken
 *   1. over the RoIs whose level is l and whose image is b, in ascending RoI index;
 *   2. within a RoI by bin row, 3. then by bin column,
 *   4. then by the taps in the order top-left, top-right, bottom-left, bottom-right.
 * Each term is separately rounded fp32, as the reference computes it: (1 - x_lerp) * ((1 - y_lerp) * g), x_lerp * ((1 - y_lerp) * g),
 * (1 - x_lerp) * (y_lerp * g), x_lerp * (y_lerp * g). All four taps are replayed, the zero-weight ones of a sample on a grid line
 * (lo == hi) included: an infinite g gives the reference's NaN there. A bin whose sample lies outside the map (the forward's strict
 * test) contributes nothing. This is the order of the reference's serial loop over each level's boxes in original order, so the
 * result equals its CPU backward bit for bit, and it depends neither on the launch geometry, nor on batch, nor on what other
 * images are in the call: two calls give the same bits.
 * A RoI in a slot at or past roi_counts[image], or whose roi_batch is outside [0, batch), contributes nothing and its grad_out rows
 * are never read into the arithmetic (the forward leaves them unwritten: they may hold NaN).
 * No floating-point atomic, no host synchronisation; two launches whatever num_rois and batch are.
 * ---------------------------------------------------------------------------------------------- */
size_t mrcnn_roi_align_pyramid_backward_workspace_bytes(int32_t num_rois);
int mrcnn_roi_align_pyramid_backward_f32(const float* grad_out, const int32_t fm_h[4], const int32_t fm_w[4], int32_t batch,
                                         int32_t depth, const float* rois, const int32_t* roi_batch, int32_t num_rois,
                                         int32_t rois_per_image, const int32_t* roi_counts, int32_t pool, float image_area,
                                         float* const grad_fm[4], void* workspace, size_t workspace_bytes,
                                         mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused convolution + bias/BatchNorm affine + residual + ReLU, channels-last, fp32 MFMA implicit
 * GEMM — the building block of Bottleneck.forward (model.py:190-211), the stem (model.py:223-226),
 * FPN laterals/smoothing (model.py:145-157), RPN and head convolutions. No reference kernel exists
 * for it (the reference calls nn.Conv2d / BatchNorm2d / ReLU / F.pad as separate modules).
 *
 *   y[b,oy,ox,co] = act( scale[co] * sum_{ky,kx,ci} x[b, oy*stride+ky-pad_top, ox*stride+kx-pad_left, ci]
 *                                                  * w[co,ky,kx,ci]  + shift[co]  (+ residual) )
 *   x        fp32 [batch][H][W][cin]           (NHWC)   cin % 4 == 0
 *   w        fp32 [cout][kh][kw][cin]          (OHWI)
 *   scale    fp32 [cout] or NULL (=1);  shift fp32 [cout] or NULL (=0)
 *            (BN eval + conv bias folded by the caller: scale = g/sqrt(var+eps),
 *             shift = (bias-mean)*scale + beta; kept as an fp32 epilogue, not folded into w)
 *   residual fp32 [batch][OH/res_div][OW/res_div][cout] or NULL, added before the activation;
 *            res_div = 1 (Bottleneck `out += residual`) or 2 (FPN top-down: nearest 2x upsample,
 *            model.py:150-152)
 *   activation 0 none, 1 ReLU, 2 sigmoid (1/(1+exp(-v)), Mask.forward's last op, model.py:914)
 *   y        fp32 [batch][OH][OW][cout],  OH = (H + pad_top + pad_bottom - kh)/stride + 1, same for OW
 * Zero padding is applied on the fly (SamePad2d, model.py:64-87, never materialised).
 * ---------------------------------------------------------------------------------------------- */
int mrcnn_conv_bn_act_nhwc_f32(const float* x, int32_t batch, int32_t height, int32_t width,
                               int32_t cin, const float* w, int32_t cout, int32_t kh, int32_t kw,
                               int32_t stride, int32_t pad_top, int32_t pad_left, int32_t pad_bottom,
                               int32_t pad_right, const float* scale, const float* shift,
                               const float* residual, int32_t res_div, int32_t activation, float* y,
                               mrcnn_stream_t stream);

/* Same contract as mrcnn_conv_bn_act_nhwc_f32, but the contraction runs on fp16-operand MFMA
 * (v_mfma_f32_32x32x16_f16, fp32 accumulate). x, residual and y stay fp32 in HBM; x is converted while it is
 * staged to LDS. The caller prepares the weights once as fp16 planes [cout][kh][kw][cin]:
 *     w_hi = fp16(w),   w_lo = fp16(w - fp32(w_hi))
 *   products = 1   plain fp16 operands, x_hi*w_hi (BASELINE config 5's "fp16 MFMA path"); w_lo may be NULL.
 *                  Error ~2^-11 relative per term: does NOT meet the 1e-4 bar of the fp32 path.
 *   products = 3   error-compensated split x_hi*w_hi + x_hi*w_lo + x_lo*w_hi: every product exact in fp32,
 *                  fp32 accumulation, ~2^-21 relative per term (fp32-grade) for |x|, |w| < 65504.
 * cin % 8 == 0 (the stem pads 3 -> 8 channels). */
int mrcnn_conv_bn_act_nhwc_f16mfma(const float* x, int32_t batch, int32_t height, int32_t width, int32_t cin,
                                   const void* w_hi, const void* w_lo, int32_t cout, int32_t kh, int32_t kw,
                                   int32_t stride, int32_t pad_top, int32_t pad_left, int32_t pad_bottom,
                                   int32_t pad_right, const float* scale, const float* shift,
                                   const float* residual, int32_t res_div, int32_t activation, int32_t products,
                                   float* y, mrcnn_stream_t stream);

/* 2x2 stride-2 transposed convolution + bias + activation, NHWC — Mask.forward's `deconv` + ReLU
 * (nn.ConvTranspose2d(256, 256, kernel_size=2, stride=2), model.py:864,906-912) as ONE GEMM whose epilogue scatters
 * straight into the up-sampled tensor (no pixel-shuffle copy):
 *     y[b, 2i+dy, 2j+dx, co] = act( sum_ci x[b,i,j,ci] * w[(dy*2+dx)*cout + co][ci] + bias4[(dy*2+dx)*cout + co] )
 *   x [batch][H][W][cin];  w fp32 [4*cout][1][1][cin] (the caller repacks the [cin][cout][2][2] weight once);
 *   bias4 fp32 [4*cout] (the bias repeated for the four taps);  y [batch][2H][2W][cout].
 * The _f16mfma form takes the split fp16 weight planes and `products` like mrcnn_conv_bn_act_nhwc_f16mfma. */
int mrcnn_deconv2x2_bias_act_nhwc_f32(const float* x, int32_t batch, int32_t height, int32_t width, int32_t cin,
                                      const float* w, int32_t cout, const float* bias4, int32_t activation,
                                      float* y, mrcnn_stream_t stream);
int mrcnn_deconv2x2_bias_act_nhwc_f16mfma(const float* x, int32_t batch, int32_t height, int32_t width,
                                          int32_t cin, const void* w_hi, const void* w_lo, int32_t cout,
                                          const float* bias4, int32_t activation, int32_t products, float* y,
                                          mrcnn_stream_t stream);

/* The plain-fp16 mode (products = 1) with fp16 ACTIVATIONS in HBM — BASELINE configs[4]'s "fp16 MFMA path":
 *   x_is_f16 / y_is_f16 choose the storage type of the input and of the output (and of the residual, which has the
 *   output's type); at least one of them is set (fp32 both ways is mrcnn_conv_bn_act_nhwc_f16mfma). fp16 tensors are
 *   NHWC like their fp32 counterparts. w_f16 = the fp16 weight plane [cout][kh][kw][cin]. Supported combinations:
 *     fp32 → fp16   no residual, activation 0/1 (the stem, the first conv behind RoIAlign)
 *     fp16 → fp16   residual (res_div 1 or 2) or none, activation 0/1; cin % 32 == 0
 *     fp16 → fp32   no residual, activation 0/1/2 (FPN smoothing, RPN heads, the FC layers, the mask sigmoid)
 *   cout must be even for an fp16 output (channel pairs are stored as 4-byte words). A conv that reads an fp16 tensor
 *   sees exactly the operand the fp32-storage path rounds to, so only residual adds, pooling and stores differ.
 * mrcnn_deconv2x2_bias_act_nhwc_f16io: the 2x2 stride-2 transposed conv, fp16 in and out.
 * mrcnn_maxpool_nhwc_f16: the zero-padded max-pool on fp16 NHWC (channels % 8 == 0). */
int mrcnn_conv_bn_act_nhwc_f16io(const void* x, int32_t x_is_f16, int32_t batch, int32_t height, int32_t width,
                                 int32_t cin, const void* w_f16, int32_t cout, int32_t kh, int32_t kw, int32_t stride,
                                 int32_t pad_top, int32_t pad_left, int32_t pad_bottom, int32_t pad_right,
                                 const float* scale, const float* shift, const void* residual, int32_t res_div,
                                 int32_t activation, void* y, int32_t y_is_f16, mrcnn_stream_t stream);
int mrcnn_deconv2x2_bias_act_nhwc_f16io(const void* x_f16, int32_t batch, int32_t height, int32_t width, int32_t cin,
                                        const void* w_f16, int32_t cout, const float* bias4, int32_t activation,
                                        void* y_f16, mrcnn_stream_t stream);
/* The pipelined form of the plain-fp16 conv (csrc/conv_f16p.hip: eight waves, LDS-DMA staging kept in flight across barriers,
 * v_mfma_f32_16x16x32_f16) — what the "f16" mode runs wherever the shape allows. fp16 NHWC input, cin % 64 == 0, cout % 64 == 0,
 * kh*kw <= 25, any stride, 0 <= pad_top < kh, 0 <= pad_left < kw;
 *   y = act(conv(x, w) * scale + shift + residual)
 * with an optional fp16 residual [batch][OH/res_div][OW/res_div][cout], res_div 1 or 2 (2 = FPN nearest-upsample-add, even OH / OW),
 * written as fp16 (y_f16) and / or fp32 (y_f32) NHWC — at least one of them non-null (the FPN smoothing convs write both: fp32
 * for RoIAlign, fp16 for the RPN). activation 0 none / 1 ReLU.
 * tile_rows x tile_cols: 0 = automatic (from M, cout, K and the CU count), or 128 / 160 / 192 / 256 pixels x 256 channels (one
 * workgroup per CU), or 128 / 256 pixels x 128 / 64 channels (128-pixel ones: two workgroups per CU).
 * Same operands and k order per output element as mrcnn_conv_bn_act_nhwc_f16io.
 * mrcnn_conv_f16_pipelined_supported: 1 when the shape is in range (incl. the 32-bit byte-offset limits), else 0. */
int mrcnn_conv_f16_pipelined_supported(int32_t batch, int32_t height, int32_t width, int32_t cin, int32_t cout, int32_t kh,
                                       int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t pad_bottom,
                                       int32_t pad_right);
int mrcnn_conv_f16_pipelined(const void* x_f16, int32_t batch, int32_t height, int32_t width, int32_t cin, const void* w_f16,
                             int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left,
                             int32_t pad_bottom, int32_t pad_right, const float* scale, const float* shift,
                             const void* residual_f16, int32_t res_div, int32_t activation, void* y_f16, float* y_f32,
                             int32_t tile_rows, int32_t tile_cols, mrcnn_stream_t stream);
/* The RPN's shared conv with its two 1x1 heads (model.py:605-607,624-641) on the pipelined fp16 kernel, one launch: stride 1,
 * cout % 256 == 0; act(conv(x, w) * scale + shift) is rounded to fp16 and multiplied, while still in registers, by w_head_f16
 * [32][cout] (rows 0-17: conv_class then conv_bbox weights, rows 18-31 zero). head_part fp32 [cout / 256][M][32], M = batch * OH *
 * OW pixels in image order: the sums over each 256-channel tile, without the head bias — for cout = 512 the input form 4 of
 * mrcnn_rpn_scores_deltas_v2_f32, which adds the two planes and the bias. Fully overwritten. The activation itself is not stored. */
int mrcnn_conv_f16_pipelined_heads(const void* x_f16, int32_t batch, int32_t height, int32_t width, int32_t cin,
                                   const void* w_f16, int32_t cout, int32_t kh, int32_t kw, int32_t pad_top, int32_t pad_left,
                                   int32_t pad_bottom, int32_t pad_right, const float* scale, const float* shift,
                                   int32_t activation, const void* w_head_f16, float* head_part, int32_t tile_rows,
                                   mrcnn_stream_t stream);
int mrcnn_maxpool_nhwc_f16(const void* x, int32_t batch, int32_t height, int32_t width, int32_t channels,
                           int32_t kernel, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t pad_bottom,
                           int32_t pad_right, void* y, mrcnn_stream_t stream);

/* Zero-padded max-pool, NHWC fp32: [batch][H][W][C] -> [batch][OH][OW][C], OH = (H+pad_top+pad_bottom-k)/s+1.
 * Covers the stem's SamePad2d(3,2) + MaxPool2d(3,2) (model.py:227-228; pads (0,1,0,1) on even sizes — the
 * caller computes the pads with the reference's formula, model.py:75-87) and P6 = MaxPool2d(1,2)
 * (model.py:109,161). Out-of-range taps read 0, exactly as F.pad(..., 'constant', 0) then max. C % 4 == 0. */
int mrcnn_maxpool_nhwc_f32(const float* x, int32_t batch, int32_t height, int32_t width, int32_t channels,
                           int32_t kernel, int32_t stride, int32_t pad_top, int32_t pad_left,
                           int32_t pad_bottom, int32_t pad_right, float* y, mrcnn_stream_t stream);
/* The same with a selectable output layout (MRCNN_LAYOUT_NHWC / MRCNN_LAYOUT_KBLOCKED [C/8][batch*OH*OW][8], C % 8 == 0:
 * P6 for the RPN's Winograd conv). */
int mrcnn_maxpool_f32(const float* x, int32_t batch, int32_t height, int32_t width, int32_t channels, int32_t kernel,
                      int32_t stride, int32_t pad_top, int32_t pad_left, int32_t pad_bottom, int32_t pad_right, float* y,
                      int32_t y_layout, mrcnn_stream_t stream);

/* Bottleneck.forward (/root/reference/model.py:190-211, residual branch :254-262) for the ResNet C2 blocks of the plain-fp16
 * path in ONE launch (csrc/bottleneck_f16.hip): planes = 64, stride 1, fp16 NHWC in and out,
 *   y = relu(conv3(relu(conv2(relu(conv1(x)*s1+t1))*s2+t2))*s3+t3 + residual),   conv2 = SamePad2d(3,1) + 3x3,
 * residual = x (cin = 256, wd_frags null) or fp16(conv_d(x)*sd+td) (cin = 64: the stage's first block, 1x1 downsample conv + BN).
 * Both 64-channel intermediates are rounded to fp16 where the per-layer path (mrcnn_conv_bn_act_nhwc_f16io /
 * mrcnn_conv_f16_pipelined, one launch per conv) rounds them; the two paths differ by the summation order inside an MFMA only.
 * Weights arrive as A fragments made by mrcnn_pack_afrags_f16 from the fp16 OHWI tensors flattened to [cout][k]
 * (k = kh*kw*cin): w1 [64][cin], w2 [64][576], w3 [256][64], wd [256][64]; s / t: the folded BN scale and shift (fp32, per output
 * channel). Image i of a batch == image i alone (a tile never spans images, one kernel for every batch size).
 * _supported: 1 when the shape is in range (planes 64, cin 256 / 64 as above, 32-bit byte offsets), else 0. */
int mrcnn_pack_afrags_f16(const void* w_f16, int32_t cout, int32_t k, void* frags_f16, mrcnn_stream_t stream);
int mrcnn_bottleneck_c2_f16_supported(int32_t batch, int32_t height, int32_t width, int32_t cin, int32_t planes,
                                      int32_t has_downsample);
int mrcnn_bottleneck_c2_f16(const void* x_f16, int32_t batch, int32_t height, int32_t width, int32_t cin, const void* w1_frags,
                            const float* s1, const float* t1, const void* w2_frags, const float* s2, const float* t2,
                            const void* w3_frags, const float* s3, const float* t3, const void* wd_frags, const float* sd,
                            const float* td, void* y_f16, mrcnn_stream_t stream);

/* The tail of Mask.forward (/root/reference/model.py:906-914) of the plain-fp16 path in ONE launch (csrc/mask_tail_f16.hip):
 *   y = sigmoid(conv5(relu(deconv(x) + bias_de)) + bias5)
 * x fp16 NHWC [rois][height][width][256]; deconv = ConvTranspose2d(256, 256, kernel 2, stride 2) given as the A fragments
 * (mrcnn_pack_afrags_f16) of its GEMM form [4*256][256], output row (dy*2 + dx)*256 + co (the weight mrcnn_deconv2x2_bias_act_nhwc_f16io
 * takes), bias_de4 [4*256] (the bias repeated per sub-pixel); conv5 1x1 256 -> classes (<= 96) given as the A fragments of its
 * weight zero-padded to [96][256], bias5 [classes]; y fp32 NHWC [rois][2*height][2*width][classes], fully overwritten.
 * The deconv's output is rounded to fp16 where the two-launch path rounds it (its HBM tensor) but never stored.
 * _supported: 1 when the shape is in range (cin 256, cout_deconv 256, classes <= 96, 32-bit byte offsets), else 0. */
int mrcnn_mask_tail_f16_supported(int32_t rois, int32_t height, int32_t width, int32_t cin, int32_t cout_deconv, int32_t classes);
int mrcnn_mask_tail_f16(const void* x_f16, int32_t rois, int32_t height, int32_t width, int32_t cin, const void* wde_frags,
                        const float* bias_de4, int32_t cout_deconv, const void* w5_frags, const float* bias5, int32_t classes,
                        float* y_f32, mrcnn_stream_t stream);

/* RPN glue, two launches.
 * mrcnn_rpn_scores_deltas_f32 — replaces the per-level permute/view/softmax/cat of RPN.forward + rpn_detect
 *   (model.py:627-641,1294-1304): heads[l] = fused head output of level l, NHWC [batch][H_l][W_l][18]
 *   (channels 0-5: (bg,fg) logits of the 3 anchor ratios, 6-17: their 4 deltas); level_hw[l] = H_l*W_l.
 *   scores [batch][A] = softmax(bg,fg)[1], deltas [batch][A][4], A = 3*sum(level_hw), anchor index
 *   = first(l) + (y*W_l + x)*3 + ratio — the reference's order (utils.py:154-160).
 * mrcnn_proposal_decode_f32 — replaces the gather + boxes_refine + boxes_clamp_ of rpn_refine
 *   (model.py:1341-1358, data.py:124-148,86-92): for the top-k anchor indices `order` [batch][k] (int64) and
 *   their scores, dets [batch][k][5] = (clip(refine(anchor, delta*std_dev), [0,H]x[0,W]), score), in the
 *   reference's fp32 op order. The clip is fminf(fmaxf(v, lo), hi): a NaN coordinate (expf overflow: -inf + inf)
 *   becomes the lower bound, where torch.clamp would keep the NaN — every output coordinate is finite and inside
 *   the image, whatever the deltas, so NMS never sees a non-finite box. The score is copied as it is. */
int mrcnn_rpn_scores_deltas_f32(const float* const heads[5], const int32_t level_hw[5], int32_t batch,
                                float* scores, float* deltas, mrcnn_stream_t stream);
/* The same with a per-level input form (level_mode[l]): 0 = NHWC [batch][H_l][W_l][18] head outputs as above;
 * 1 / 2 = the head sums of mrcnn_conv3x3_winograd_heads_f32 in tile mode 1 / 2: [2][rows][32] fp32 in that function's row
 * order, bias not yet added: logits/deltas = (sum of the two k halves) + head_bias[c]; 3 = the head sums of
 * mrcnn_conv3x3_winograd4_heads_f32: [rows][32], logits/deltas = sum + head_bias[c]; 4 = the two planes of
 * mrcnn_conv_f16_pipelined_heads (cout = 512): [2][batch*H_l*W_l][32] in pixel order, (plane 0 + plane 1) + head_bias[c].
 * level_h/level_w: H_l, W_l. */
int mrcnn_rpn_scores_deltas_v2_f32(const float* const heads[5], const int32_t level_h[5], const int32_t level_w[5],
                                   const int32_t level_mode[5], const float* head_bias, int32_t batch, float* scores,
                                   float* deltas, mrcnn_stream_t stream);
int mrcnn_proposal_decode_f32(const float* anchors, const float* deltas, const int64_t* order,
                              const float* top_scores, int32_t batch, int32_t num_anchors, int32_t k,
                              const float std_dev[4], float image_height, float image_width, float* dets,
                              mrcnn_stream_t stream);

/* Detection decode — the first half of MaskRCNN.mrn_refine (model.py:1405-1443) for a whole batch in one launch:
 * softmax + arg-max over classes, class-specific delta gather, boxes_refine(rois, delta*std_dev) (data.py:124-148),
 * scale to pixels, clip to each image's window, round (half to even), validity = class > 0 and slot <
 * roi_counts[image] (and score >= min_confidence when min_confidence > 0; config.py:204 sets 0 = no filter).
 *   logits [batch*P][num_classes] (row stride logit_stride elements), bbox [batch*P][num_classes][4] (row stride
 *   bbox_stride), rois [batch*P][4] normalised, windows [batch][4] pixels.
 *   dets [batch*P][5] = (y1,x1,y2,x2,score), class_ids int64 [batch*P] = arg-max class,
 *   nms_class_ids int32 [batch*P] = class for valid slots, a unique negative value otherwise (so that excluded
 *   slots neither suppress nor are suppressed in the class-aware NMS that follows).
 * A slot at or past roi_counts[image] gets the empty record: its dets row all zero, class_ids = 0, nms_class_ids =
 * -(slot+1); nothing of its logits / bbox rows is read. A live row whose softmax is NaN gets the same record, and
 * nothing of its bbox row is read: a row with a NaN logit or a +inf logit (the sum of exponentials is NaN), and a row
 * without an ordered maximum (all NaN, or all -inf). F.softmax gives NaN probabilities there and torch.max of an all-NaN
 * row index 0 (model.py:791,1407-1415): the reference drops the RoI as background. class_ids is therefore always in
 * [0, num_classes). -inf logits beside a finite maximum are ordinary (probability 0).
 * The window clip is fminf(fmaxf(v, lo), hi) as in mrcnn_proposal_decode_f32: a NaN coordinate becomes the window's
 * lower bound (torch.clamp would keep it), so every box of a valid slot is finite and inside its window. */
int mrcnn_detection_decode_f32(const float* logits, int64_t logit_stride, const float* bbox, int64_t bbox_stride,
                               const float* rois, const int32_t* roi_counts, const float* windows, int32_t batch,
                               int32_t rois_per_image, int32_t num_classes, const float std_dev[4],
                               float image_height, float image_width, float min_confidence, float* dets,
                               int32_t* nms_class_ids, int64_t* class_ids, mrcnn_stream_t stream);

/* 3x3 stride-1 SAME convolution + affine + ReLU as a fused Winograd F(2x2,3x3) on the fp32 MFMA: 2.25x fewer
 * multiply-adds than mrcnn_conv_bn_act_nhwc_f32 for the same layer, all arithmetic in fp32 (the result differs by the
 * transforms' rounding, a few 1e-7 relative per term). x [batch][H][W][cin] -> y [batch][H][W][cout], H and W even,
 * cin % 8 == 0. u = the filter transformed once by mrcnn_winograd_weights_f32: w [cout][3][3][cin] (OHWI) ->
 * u (16*cout*cin floats, k-blocked [cin/8][16][cout][8]). activation 0 (none) or 1 (ReLU). workspace: device memory of
 * mrcnn_conv3x3_winograd_workspace_bytes(...) bytes (the k-blocked copy of x the kernel reads). */
int mrcnn_winograd_weights_f32(const float* w, int32_t cout, int32_t cin, float* u, mrcnn_stream_t stream);
/* The same convolution with explicit tensor layouts, so that chains of 3x3 convs skip the transposition pass:
 * x_layout MRCNN_LAYOUT_NHWC (workspace needed) or MRCNN_LAYOUT_KBLOCKED = [cin/8][batch][H][W][8] (what the kernel
 * reads; no workspace). Outputs: y_nhwc and/or y_kblocked ([cout/8][batch][H][W][8], cout % 8 == 0); either may be
 * NULL, not both. mrcnn_conv_bn_act_f32 is mrcnn_conv_bn_act_nhwc_f32 with selectable output and residual layouts
 * (a k-blocked output feeds a Winograd conv directly; the FPN laterals read their half-size residual k-blocked); mrcnn_nhwc_to_kblocked_f32 is the standalone transposition. */
#define MRCNN_LAYOUT_NHWC 0
#define MRCNN_LAYOUT_KBLOCKED 1
#define MRCNN_LAYOUT_NHWC_F16 2 /* mrcnn_roi_align_pyramid_f32's output only */
int mrcnn_conv3x3_winograd_f32(const float* x, int32_t x_layout, int32_t batch, int32_t height, int32_t width,
                               int32_t cin, const float* u, int32_t cout, const float* scale, const float* shift,
                               int32_t activation, float* y_nhwc, float* y_kblocked, void* workspace,
                               size_t workspace_bytes, mrcnn_stream_t stream);
/* Winograd F(4x4, 3x3): the same convolution with 4x (instead of 2.25x) fewer multiply-adds, for maps whose height and
 * width are multiples of 4 (csrc/conv_wino4.hip; fp32 arithmetic, max |err| about 2e-5 at unit scale against the direct
 * convolution — ten times F(2x2)'s, inside the 1e-4 parity bar). Replaces the same reference lines as
 * mrcnn_conv3x3_winograd_f32 (model.py:154-157, :605,624).
 *   mrcnn_winograd4_weights_f32   w_ohwi [Cout][3][3][Cin] -> u = G g G^T in the kernel's order [Cin/4][36][2][Cout][2]
 *                                 (36 * Cout * Cin floats; evaluated in double); Cin % 4 == 0
 *   mrcnn_conv3x3_winograd4_supported   1 when H % 4 == 0, W % 4 == 0, Cin % 8 == 0, Cout % 64 == 0 and the tensors stay
 *                                 inside the kernel's 32-bit byte offsets (4*B*H*W*Cin, 4*B*H*W*Cout <= 0xFFFFFFF0 bytes)
 *   mrcnn_conv3x3_winograd4_f32   x k-blocked [Cin/8][B*H*W][8] -> relu?(conv * scale + shift) as NHWC and/or k-blocked
 *                                 [Cout/8][B*H*W][8] (either output pointer may be null, not both) */
int mrcnn_winograd4_weights_f32(const float* w_ohwi, int32_t cout, int32_t cin, float* u, mrcnn_stream_t stream);
int32_t mrcnn_conv3x3_winograd4_supported(int32_t batch, int32_t height, int32_t width, int32_t cin, int32_t cout);
int mrcnn_conv3x3_winograd4_f32(const float* x_kblocked, int32_t batch, int32_t height, int32_t width, int32_t cin,
                                const float* u, int32_t cout, const float* scale, const float* shift, int32_t activation,
                                float* y_nhwc, float* y_kblocked, mrcnn_stream_t stream);
/* conv2 + conv3 of a ResNet Bottleneck in one launch (model.py:197-209): relu(scale * conv3x3_same(x) + shift) with 64 output
 * channels stays on chip (the F(4x4) kernel's epilogue) and is multiplied by the 1x1 expansion's weights there:
 *     y = relu(scale3 * (that W3^T) + shift3 + residual)
 *   x k-blocked [Cin/8][B*H*W][8]; u = mrcnn_winograd4_weights_f32 of the [64][3][3][Cin] conv2 weight; w3 fp32 [c3][64]
 *   (OHWI of the 1x1 conv), c3 % 32 == 0; residual and y NHWC [B][H][W][c3], residual != y. The conv3 part runs the
 *   direct kernel's k order and epilogue expression: equal bit for bit to mrcnn_conv3x3_winograd4_f32 followed by
 *   mrcnn_conv_bn_act_f32 with the same residual. Same shape limits as mrcnn_conv3x3_winograd4_f32 with Cout = 64. */
int mrcnn_conv3x3_winograd4_conv3_f32(const float* x_kblocked, int32_t batch, int32_t height, int32_t width, int32_t cin,
                                      const float* u, const float* scale, const float* shift, const float* w3, int32_t c3,
                                      const float* scale3, const float* shift3, const float* residual, float* y,
                                      mrcnn_stream_t stream);
/* The F(4x4) form of mrcnn_conv3x3_winograd_heads_f32 (RPN shared conv + its two 1x1 heads, model.py:605-641, in one
 * launch): head_part fp32 [rows][32], rows = mrcnn_conv3x3_winograd4_heads_rows(batch, H, W); row of pixel (b,y,x) =
 * mt*512 + ((y/4 & 3)*8 + (x/4 & 7))*16 + (y&3)*4 + (x&3), mt = (b*ceil(H/16) + y/16)*ceil(W/32) + x/32; the sums over
 * all cout channels without the head bias — input form 3 of mrcnn_rpn_scores_deltas_v2_f32. Fully overwritten. */
int64_t mrcnn_conv3x3_winograd4_heads_rows(int32_t batch, int32_t height, int32_t width);
int mrcnn_conv3x3_winograd4_heads_f32(const float* x_kblocked, int32_t batch, int32_t height, int32_t width, int32_t cin,
                                      const float* u, int32_t cout, const float* scale, const float* shift,
                                      int32_t activation, const float* w_head32, float* head_part, mrcnn_stream_t stream);

/* Tile shape of mrcnn_conv3x3_winograd_f32 on maps of at least 8 x 8 tile positions: 1 (default) = 8 x 8 position blocks of
 * one image with the input transform done per lane out of a raw LDS region (conv3x3_wino8s_f32), 0 = 64 consecutive
 * positions with a staged transform (conv3x3_wino8_f32), -1 = back to the default / MRCNN_WINO_SPATIAL. Same results bit
 * for bit; a process-wide tuning switch, not per stream. */
int mrcnn_winograd_set_spatial(int32_t on);
int mrcnn_conv_bn_act_f32(const float* x, int32_t batch, int32_t height, int32_t width, int32_t cin, const float* w,
                          int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left,
                          int32_t pad_bottom, int32_t pad_right, const float* scale, const float* shift,
                          const float* residual, int32_t res_div, int32_t residual_layout, int32_t activation,
                          float* y, int32_t y_layout, mrcnn_stream_t stream);
/* mrcnn_conv_bn_act_nhwc_f32 for the heads' GEMMs over [image][RoI slot] rows (Classifier.forward, model.py:782-794, runs on
 * the rois that survived NMS only — model.py:1366-1374): the output rows (batch * OH * OW of them) come in groups of
 * rows_per_group slots of which the first row_counts[group] are valid; an M tile without a valid row is skipped — nothing
 * is read, its output rows are left untouched. Rows are independent in a GEMM, so the valid rows' results are bit-identical to
 * the unmasked call. row_counts int32 device memory, or NULL (= every row). */
int mrcnn_conv_bn_act_rows_f32(const float* x, int32_t batch, int32_t height, int32_t width, int32_t cin, const float* w,
                               int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left,
                               int32_t pad_bottom, int32_t pad_right, const float* scale, const float* shift,
                               int32_t activation, float* y, const int32_t* row_counts, int32_t rows_per_group,
                               mrcnn_stream_t stream);
/* Rows of the M tile mrcnn_conv_bn_act_rows_f32 gives a layer with `cout` output channels (the skip rule's granularity: a caller
 * that accounts for the work that ran — bench.py's roofline pass — counts tiles of this many rows). */
int32_t mrcnn_conv_rows_tile_m(int32_t cout);
/* The kernel instantiation mrcnn_conv_bn_act_f32 / _nhwc_f32 / _rows_f32 / mrcnn_deconv2x2_bias_act_nhwc_f32 launch for these
 * arguments on a device with `cus` compute units — the dispatcher's own answer (the launchers launch from the same function),
 * host arithmetic only, no device needed. out_mode: 0 NHWC, 1 the 2x2 transposed-conv scatter (cout = 4 x the deconv's channels,
 * kh = kw = 1), 2 k-blocked. has_residual / has_row_counts: 0 or 1. Returns -1 for arguments the entry points refuse, else
 *   bits 0-3   kernel: 0 tiled (conv_igemm_f32), 1 / 2 / 3 streaming 1x1 (conv_pw_stream_f32 for 256 -> <= 64, 64 -> <= 64,
 *              64 -> <= 256 channels)
 *   bits 4-7   tile (BM x BN, BK): 0 128x32,32  1 256x64,32  2 256x64,16  3 128x96,32  4 128x128,16  5 128x64,16  6 128x128,32
 *              7 none (streaming)
 *   bits 8-11  mode: 0 aligned taps, 1 generic (cin % 32 != 0), 2 pointwise
 *   bits 12-15 epilogue: 0 plain, 1 residual, 2 half-size residual, 3 sigmoid, 4 2x2 scatter
 *   bit 16     the two-chain sum over K (K >= 1024 on tiles 0, 5, 6). */
int32_t mrcnn_conv_route(int32_t batch, int32_t height, int32_t width, int32_t cin, int32_t cout, int32_t kh, int32_t kw,
                         int32_t stride, int32_t pad_top, int32_t pad_left, int32_t pad_bottom, int32_t pad_right,
                         int32_t has_residual, int32_t res_div, int32_t activation, int32_t out_mode, int32_t has_row_counts,
                         int32_t cus);
int mrcnn_nhwc_to_kblocked_f32(const float* x, int64_t pixels, int32_t channels, float* y, mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of the fp32 NHWC convolution with a FROZEN affine and an activation, at stride 1 — the layers train_model(layers="heads")
 * trains (model.py:1010-1016, :1218: fpn.P*, rpn.*, classifier.*, mask.*, BatchNorm in eval mode) — or 2 (the backbone's strided
 * convs, next block): gradients for the input, the weight, the shift and the residual. No gradient of `scale` is produced: BatchNorm
 * is frozen in every schedule, and its statistics are not this library's business. The reference has no kernel for any of this (autograd of nn.Conv2d / BatchNorm2d / ReLU).
 *
 * The forward is  pre = scale[co] * conv(x, w) + shift[co] (+ residual),  y = act(pre),  stride s, pads (pt, pl, pb, pr),
 * x [B][H][W][Cin], w [Cout][KH][KW][Cin], y [B][OH][OW][Cout]  (mrcnn_conv_bn_act_nhwc_f32). Given dy of y's shape:
 *
 *   stride  s = 1 or 2; OH = (H + pt + pb - KH) / s + 1, OW likewise, a remainder is legal (a 1 x 1 kernel on odd H uses the last
 *           row). mrcnn_conv_act_backward_f32 has no stride: it works on the output map.
 *   g       the gradient of pre; every operation a separately rounded fp32 operation:
 *             activation 0   g = dy          1 (ReLU)   g = y > 0 ? dy : 0          2 (sigmoid)   t = 1 - y; u = y * t; g = dy * u
 *           g is the residual's gradient at res_div = 1; at res_div = 2 (the FPN's nearest-upsample add) the residual's gradient
 *           is (g00 + g01) + (g10 + g11) of the 2 x 2 block, in fp32.
 *   z       g * scale[co] in fp32, or g where scale is NULL, stored with a channel pitch of Cout4 = roundup(Cout, 4), pad channels
 *           +0. Where no activation, no scale, no row counts and no scatter are involved and Cout % 4 == 0, z is dy itself: pass
 *           z = NULL and hand dy to the two calls below.
 *   dshift  [co] = the sum of g over the contributing output pixels, accumulated in fp64 in a fixed order that depends on the
 *           shape only (a thread's pixels in ascending order, then the threads' partials in index order, in a second launch),
 *           narrowed to fp32 last. No atomic, no last-block protocol.
 *   dx      at stride 1 [b,iy,ix,ci] = sum over (ky,kx,co) of z[b, iy+pt-ky, ix+pl-kx, co] * w[co,ky,kx,ci]. It IS the forward:
 *           mrcnn_conv_bn_act_nhwc_f32 on z as the input [B][OH][OW][Cout4] with the weight
 *           w'[ci][ky'][kx'][co] = w[co][KH-1-ky'][KW-1-kx'][ci] (co >= Cout: zero), pads (KH-1-pt, KW-1-pl, KH-1-pb, KW-1-pr), no
 *           affine, no residual, activation 0; a transform kernel writes w' into the workspace on every call (the weights change
 *           every step). dx equals that forward call on those operands bit for bit: it has the forward's routes and limits, and
 *           image i does not depend on the rest of the batch. A pad larger than K - 1 is refused.
 *           At stride 2 for the 1 x 1 kernel without padding only (every strided conv of the model whose input needs a gradient):
 *           dx is then the COMPACT gradient dxc [B][OH][OW][Cin], dxc[b,i,j,ci] = sum over co of z[b,i,j,co] * w[co,0,0,ci] — the
 *           same forward call, with w'[ci][co] = w[co][ci] a plain GEMM, bit for bit; mrcnn_dilate2_sum_f32 (below) writes the full
 *           gradient from it.
 *   dw      [co,ky,kx,ci] = sum over (b,oy,ox) of z[b,oy,ox,co] * x[b, oy*s+ky-pt, ox*s+kx-pl, ci], taps outside the image
 *           contributing nothing; any kernel size at either stride. The pixel axis M = B*OH*OW is cut into chunks of
 *           L = mrcnn_conv_backward_weights_chunk(...) pixels — a function of the shape only, chosen as for a 256-CU part, so the
 *           bits do not depend on the device; it depends on the stride through M = B*OH*OW. Inside a chunk an element is an fp32
 *           fmaf chain over the chunk's pixels in ascending order (v_mfma_f32_32x32x2_f32); a second launch adds the ceil(M / L)
 *           chunks' sums in ascending chunk order in fp64 and narrows last. Two calls give the same bits.
 *   rows    row_counts / rows_per_group as in mrcnn_conv_bn_act_rows_f32: an output row at or past its group's count contributes
 *           nothing to dw and dshift, its z and g rows are written as zero, and its rows of dy and y — and the x values of its taps
 *           in dw — are never read into the arithmetic (the forward leaves such rows unwritten: they may hold NaN). dx is then
 *           zero wherever only such rows land. Not with a residual or the scatter, and at stride 1 only.
 *   scatter (mrcnn_deconv2x2_bias_act_nhwc_f32): dy and y are [B][2*out_h][2*out_w][cout / 4]; GEMM column (dy*2+dx)*C + co of
 *           row (b,i,j) is pixel (2i+dy, 2j+dx). mrcnn_conv_act_backward_f32 gathers; after it z [M][cout] is an ordinary 1 x 1
 *           case and dshift is [cout] = [4*C] (the caller adds the four taps for the bias). Activation 0 or 1.
 *
 * mrcnn_conv_act_backward_f32: dy, y (read only with an activation) -> z, g, dresidual2, dshift; each output pointer may be NULL
 *   (not wanted). out_h, out_w, cout: the GEMM's row map and column count (with scatter: the deconv's input map and 4 * C).
 *   g fp32 [B][out_h][out_w][cout] (dense pitch, no scatter), dresidual2 fp32 [B][out_h/2][out_w/2][cout] (res_div = 2 only; out_h
 *   and out_w even). Two launches with dshift, one without, none when every output is NULL.
 * mrcnn_conv_backward_data_f32: z [B][OH][OW][Cout4] -> dx [B][H][W][Cin] (stride 2: [B][OH][OW][Cin]). Two launches.
 * mrcnn_conv_backward_weights_f32: x, z -> dw [Cout][KH][KW][Cin]. Two launches.
 * workspace: >= mrcnn_conv_backward_workspace_bytes(...) bytes of device memory, 16-byte aligned, shared by the three calls of a
 *   layer on one stream (the larger of: the dshift partials, w', ceil(M / L) * Cout * KH*KW*Cin floats of chunk sums, which are
 *   addressed with 64-bit offsets). The library allocates nothing and never synchronises; the launch counts do not depend on B.
 * Limits: stride 1 or 2, fp32, NHWC, Cin % 4 == 0, Cout >= 1, activation 0 / 1 / 2 in the forward's combinations, every tensor — z
 *   included — within the forward's 32-bit byte offsets (<= 0xFFFFFFF0 bytes). Outside them: an error before any launch.
 *   mrcnn_conv_backward_weights_chunk and _workspace_bytes return 0 for arguments the entry points refuse.
 * ---------------------------------------------------------------------------------------------- */
int mrcnn_conv_act_backward_f32(const float* dy, const float* y, int32_t batch, int32_t out_h, int32_t out_w, int32_t cout,
                                const float* scale, int32_t activation, int32_t res_div, int32_t scatter,
                                const int32_t* row_counts, int32_t rows_per_group, float* z, float* g, float* dresidual2,
                                float* dshift, void* workspace, size_t workspace_bytes, mrcnn_stream_t stream);
int mrcnn_conv_backward_data_f32(const float* z, int32_t batch, int32_t height, int32_t width, int32_t cin, const float* w,
                                 int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left,
                                 int32_t pad_bottom, int32_t pad_right, float* dx, void* workspace, size_t workspace_bytes,
                                 mrcnn_stream_t stream);
int mrcnn_conv_backward_weights_f32(const float* x, int32_t batch, int32_t height, int32_t width, int32_t cin, const float* z,
                                    int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left,
                                    int32_t pad_bottom, int32_t pad_right, const int32_t* row_counts, int32_t rows_per_group,
                                    float* dw, void* workspace, size_t workspace_bytes, mrcnn_stream_t stream);
size_t mrcnn_conv_backward_workspace_bytes(int32_t batch, int32_t height, int32_t width, int32_t cin, int32_t cout, int32_t kh,
                                           int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t pad_bottom,
                                           int32_t pad_right);
int32_t mrcnn_conv_backward_weights_chunk(int32_t batch, int32_t height, int32_t width, int32_t cin, int32_t cout, int32_t kh,
                                          int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t pad_bottom,
                                          int32_t pad_right);

/* ------------------------------------------------------------------------------------------------
 * The backbone's backward: the conv backward above at stride 2, and the two gradients that are not convolutions. With them every
 * layer of the model has a backward (model.py:174-270: conv1 and downsample.0 of the first block of C3, C4 and C5 are 1 x 1 stride
 * 2; the stem is 7 x 7 stride 2 pad 3 on the image, then SamePad2d(3,2) + MaxPool2d(3,2); P6 = MaxPool2d(1,2) of P5). BatchNorm
 * stays frozen in every schedule, so there is still no gradient of `scale`.
 *
 *   dilate  mrcnn_dilate2_sum_f32 writes the full gradient from the compact one: dx[b,2i,2j,:] = a[b,i,j,:], or a + b2 as ONE fp32
 *           add where a second compact tensor is given (conv1 and downsample.0 of a strided block read the same x: the sum of
 *           their two full-size gradients is a + b2 at the even positions and 0 + 0 elsewhere, bit for bit), and +0 at every other
 *           element. a, b2 [B][ceil(H/2)][ceil(W/2)][C], dx [B][H][W][C], C % 4 == 0, odd H and W legal. Every byte of dx is
 *           written exactly once, in 16-byte stores: no memset before it, no atomic. With one operand it is also the backward of
 *           MaxPool2d(kernel 1, stride 2) (P6): a window of one tap always takes it. One launch.
 *   pool    mrcnn_maxpool_backward_f32: the backward of the zero-padded max-pool mrcnn_maxpool_f32 computes (F.pad(..., 0) then
 *           MaxPool2d, model.py:227-228), from the saved input x [B][H][W][C] and dy [B][OH][OW][C] -> dx [B][H][W][C].
 *             which tap is taken   for every output element the window is walked in (ky, kx) row-major order, taps outside the
 *                      image reading 0; the walk starts with max = -inf at the first tap and a tap takes over when it is strictly
 *                      greater than the maximum so far (torch's `val > max`): the first of equal maxima wins.
 *             a padding tap loses the gradient   where the taken tap lies outside the image its gradient is dropped. That happens
 *                      when every real value of the window is <= 0 behind an earlier padding zero, or < 0 behind a later one: common
 *                      behind a ReLU.
 *             gather form   the thread that owns an input element adds, in fp32 from +0, the gradients of the at most
 *                      ceil(k/s)^2 windows that take it, in ascending (oy, ox) order. No atomic, every byte of dx is written (+0
 *                      where no window takes the element), two calls give the same bits.
 *             no stored indices   the argmax is recomputed from x; the forward stays the unchanged launch and saves nothing.
 *             NaN      a NaN tap takes over whatever the maximum was (torch's `|| isnan(val)`), so the LAST NaN of a window in walk
 *                      order receives its gradient. A padding tap is never NaN. (A window of -inf alone keeps its first tap.)
 *           kernel 1 .. 3, stride 1 .. 2, every pad in 0 .. kernel - 1, C % 4 == 0, fp32 NHWC. One launch.
 * Limits: every tensor <= 0xFFFFFFF0 bytes and on a 16-byte boundary. Outside them: an error before any launch. Nothing here
 *   synchronises with the host.
 * ---------------------------------------------------------------------------------------------- */
int mrcnn_dilate2_sum_f32(const float* a, const float* b2, int32_t batch, int32_t height, int32_t width, int32_t channels, float* dx,
                          mrcnn_stream_t stream);
int mrcnn_maxpool_backward_f32(const float* dy, const float* x, int32_t batch, int32_t height, int32_t width, int32_t channels,
                               int32_t kernel, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t pad_bottom,
                               int32_t pad_right, float* dx, mrcnn_stream_t stream);
size_t mrcnn_conv3x3_winograd_workspace_bytes(int32_t batch, int32_t height, int32_t width, int32_t cin);
int mrcnn_conv3x3_winograd_nhwc_f32(const float* x, int32_t batch, int32_t height, int32_t width, int32_t cin,
                                    const float* u, int32_t cout, const float* scale, const float* shift,
                                    int32_t activation, float* y, void* workspace, size_t workspace_bytes,
                                    mrcnn_stream_t stream);

/* The ResNet stem as its own kernel (model.py:223-226): conv 7x7 stride 2 pad 3, 4 input channels (RGB + one zero
 * channel) -> 64, + affine + ReLU. x [batch][H][W][4], w [64][7][7][4] (OHWI), y [batch][H/2][W/2][64]; H, W even.
 * Same arithmetic as mrcnn_conv_bn_act_nhwc_f32 on this layer (exact fp32 MFMA; the accumulation order over k is
 * identical), 3x faster: filter resident in LDS, input patch staged per 16x16 output tile, no addressing in the loop. */
int mrcnn_stem_conv7x7_s2_nhwc_f32(const float* x, int32_t batch, int32_t height, int32_t width, const float* w,
                                   const float* scale, const float* shift, int32_t activation, float* y,
                                   mrcnn_stream_t stream);
/* The same reading the molded image itself, x_nchw [batch][3][H][W] (model.py:1102-1110): no NCHW -> NHWC4 pass over the image
 * beforehand. w stays [64][7][7][4] (channel 3 zero). Bit-identical to the NHWC form on the converted image. */
int mrcnn_stem_conv7x7_s2_nchw_f32(const float* x_nchw, int32_t batch, int32_t height, int32_t width, const float* w,
                                   const float* scale, const float* shift, int32_t activation, float* y,
                                   mrcnn_stream_t stream);
/* The same with the output stored as fp16 NHWC (the "f16" mode's trunk input): fp32 products and accumulation as above, one
 * rounding at the store. */
int mrcnn_stem_conv7x7_s2_nchw_f16out(const float* x_nchw, int32_t batch, int32_t height, int32_t width, const float* w,
                                      const float* scale, const float* shift, int32_t activation, void* y_f16,
                                      mrcnn_stream_t stream);
/* The exact-fp32 stem with its max-pool in ONE launch (round 5): conv 7x7 s2 p3 + affine + ReLU + SamePad2d(3, 2) + MaxPool2d(3, 2)
 * (model.py:223-229) on the fp32 MFMA — x_nchw fp32 [batch][3][H][W] (H, W multiples of 4), w fp32 OHWI [64][7][7][4] (channel 3
 * zero, never multiplied: K = 7 x 21 real values), y fp32 NHWC [batch][ceil(H/4)][ceil(W/4)][64]. Exact fp32 products, fp32
 * accumulation in the order (ky, kx, c); the max is exact, so the result equals conv-then-pool of the same sums. The
 * full-resolution 64-channel map never reaches memory. ReLU is part of the contract (zero padding of the pool). */
int mrcnn_stem_conv7x7_s2_pool_f32(const float* x_nchw, int32_t batch, int32_t height, int32_t width, const float* w,
                                   const float* scale, const float* shift, float* y, mrcnn_stream_t stream);
/* The "f16" mode's stem in ONE launch on the fp16 MFMA: conv 7x7 s2 p3 + affine + ReLU + SamePad2d(3, 2) + MaxPool2d(3, 2)
 * (model.py:223-229) — x_nchw fp32 [batch][3][H][W] (H, W multiples of 4), w fp32 OHWI [64][7][7][4] (channel 3 zero; rounded to fp16
 * inside), y_f16 fp16 NHWC [batch][ceil(H/4)][ceil(W/4)][64]. Image and weights are rounded to fp16 once, products accumulate
 * in fp32, the conv output is rounded to fp16 once before the max (as the two-launch form stores it). The full-resolution
 * 64-channel map never reaches memory. ReLU is part of the contract (the pool's zero padding is neutral only for values >= 0). */
int mrcnn_stem_conv7x7_s2_pool_f16(const float* x_nchw, int32_t batch, int32_t height, int32_t width, const float* w,
                                   const float* scale, const float* shift, void* y_f16, mrcnn_stream_t stream);

/* ---- selection steps of the two refine stages (no library sort / top-k / gather in the step) --------------------
 * Total, deterministic order everywhere: descending score, ties by ascending index (ATen's sort, which the
 * reference calls at model.py:1346,1478, leaves ties unspecified). Any NaN, of either sign, ranks first (above +inf), as
 * in ATen's descending sort and in mrcnn_nms_*; NaNs tie with each other (ascending index). -0.0 ranks below +0.0.
 * mrcnn_topk_desc_f32 — replaces `scores.sort(descending=True)` + `[:pre_nms_limit]` of rpn_refine
 *   (model.py:1345-1350): scores [batch][n] -> top_scores [batch][k], order int64 [batch][k]. k <= 4096, k <= n;
 *   workspace >= mrcnn_topk_workspace_bytes(batch) bytes of device memory (contents irrelevant).
 * mrcnn_proposal_select_f32 — replaces keep[:proposal_count] + gather + normalise (model.py:1366-1374):
 *   dets [batch][k][5], keep int64 [batch][k] (NMS output, ascending, padded) with keep_counts [batch] ->
 *   rois [batch][proposal_count][4] = box / (H,W,H,W), zero beyond counts[b] = min(keep_counts[b], proposal_count).
 * mrcnn_detection_select_f32 — replaces the tail of mrn_refine (model.py:1475-1487) and the mask-head box
 *   normalisation (model.py:1188): among the RoIs the class-aware NMS kept (keep / keep_counts, rows of
 *   rois_per_image) that carry a foreground class (nms_class_ids > 0), the max_instances highest scores ->
 *   out_class_ids int64, out_scores, out_boxes [batch][max_instances][4] (pixels), out_rois = boxes / (H,W,H,W),
 *   out_counts [batch]; unused slots are zero. rois_per_image <= 4096. */
size_t mrcnn_topk_workspace_bytes(int32_t batch);
int mrcnn_topk_desc_f32(const float* scores, int32_t batch, int64_t n, int32_t k, float* top_scores, int64_t* order,
                        void* workspace, size_t workspace_bytes, mrcnn_stream_t stream);
int mrcnn_proposal_select_f32(const float* dets, const int64_t* keep, const int32_t* keep_counts, int32_t batch,
                              int32_t k, int32_t proposal_count, float image_height, float image_width, float* rois,
                              int32_t* counts, mrcnn_stream_t stream);
int mrcnn_detection_select_f32(const float* dets, const int32_t* nms_class_ids, const int64_t* class_ids,
                               const int64_t* keep, const int32_t* keep_counts, int32_t batch, int32_t rois_per_image,
                               int32_t max_instances, float image_height, float image_width, int64_t* out_class_ids,
                               float* out_scores, float* out_boxes, float* out_rois, int32_t* out_counts,
                               mrcnn_stream_t stream);

/* Layout conversions at the boundary (reference tensors are NCHW, model.py:1109). */
int mrcnn_nchw_to_nhwc_f32(const float* x, int32_t batch, int32_t channels, int32_t height,
                           int32_t width, int32_t channels_padded, float* y, mrcnn_stream_t stream);
int mrcnn_nhwc_to_nchw_f32(const float* x, int32_t batch, int32_t channels, int32_t height,
                           int32_t width, float* y, mrcnn_stream_t stream);

/* ---- image pre-/post-processing around the hot path --------------------------------------
 * The reference resizes 8-bit images through Pillow (scipy.misc.imresize, utils.py:73; torchvision Resize on a PIL
 * image, data.py:277,295): BILINEAR with the support stretched by the scale factor when shrinking, 22-bit fixed-point
 * coefficients, horizontal then vertical pass with an 8-bit intermediate. These entry points reproduce that
 * arithmetic bit for bit.
 *
 * mrcnn_resize_bilinear_u8: n images of one size, src[i] [in_h][in_w][channels] interleaved uint8 at
 *   src + i*src_image_stride with src_row_stride bytes between rows (so a crop of a larger image — transform.CenterCrop
 *   before Resize in decode_masks, data.py:272-277 — needs no copy) -> dst n x [out_h][out_w][channels] contiguous,
 *   channels 1..4, sizes <= 16384. Every channel is resampled on its own, PER CHANNEL: each image equals a per-band Pillow
 *   resize always, and numpy.array(Image.fromarray(src[i]).resize((out_w, out_h), Image.BILINEAR)) for 1 and 3 channels
 *   (L, RGB); for 2 and 4 channels Pillow reads LA / RGBA and premultiplies by alpha around the resample, so that call
 *   gives the same bytes only where alpha is 255. */
size_t mrcnn_resize_u8_workspace_bytes(int32_t n, int32_t in_h, int32_t in_w, int32_t channels, int32_t out_h,
                                       int32_t out_w);
int mrcnn_resize_bilinear_u8(const uint8_t* src, int32_t n, int32_t in_h, int32_t in_w, int32_t channels,
                             int64_t src_image_stride, int64_t src_row_stride, uint8_t* dst, int32_t out_h,
                             int32_t out_w, void* workspace, size_t workspace_bytes, mrcnn_stream_t stream);
/* Which launch sequence mrcnn_resize_bilinear_u8 takes for these arguments — the launcher's own answer (it chooses through the
 * same function), host arithmetic only, no device needed. dst_alignment / workspace_alignment: the two pointers' addresses
 * modulo 16 (0: 16-byte aligned). Returns -1 for shapes the entry point refuses (n 1..65536), else
 *   0 fused: both passes in one launch, the 8-bit intermediate in LDS (1 channel, not shrinking, out_w % 16 == 0, aligned dst)
 *   1 h-fast + v-fast      2 h-fast + v-generic      3 h-generic + v-fast      4 h-generic + v-generic
 * h-fast: 1 channel, not shrinking in width, out_w % 4 == 0.  v-fast: out_w * channels % 16 == 0, dst and workspace aligned. */
int mrcnn_resize_u8_route(int32_t n, int32_t in_h, int32_t in_w, int32_t channels, int32_t out_h, int32_t out_w,
                          int32_t dst_alignment, int32_t workspace_alignment);
/* Replaces utils.resize_image's resize + pad (utils.py:72-88), mold_image (model.py:1750-1754) and the HWC -> CHW
 * float conversion of detect() (model.py:1108-1110) for one RGB image: src uint8 [in_h][in_w][3] is resized to
 * new_h x new_w (no resample when that equals the input size), placed at (top, left) of a zero canvas out_h x out_w,
 * and dst[c][y][x] = float(double(pixel) - mean_pixel[c]) (the reference subtracts a float64 MEAN_PIXEL array).
 * The caller computes scale / new size / pads exactly as utils.py:56-85 does (host integers).
 * workspace: mrcnn_resize_u8_workspace_bytes(1, in_h, in_w, 3, new_h, new_w) bytes; may be NULL when no resize. */
int mrcnn_mold_image_u8(const uint8_t* src, int32_t in_h, int32_t in_w, int32_t new_h, int32_t new_w, int32_t top,
                        int32_t left, int32_t out_h, int32_t out_w, const double mean_pixel[3], float* dst,
                        void* workspace, size_t workspace_bytes, mrcnn_stream_t stream);
/* The same for n images of ONE size (a batch from one camera / dataset: detect() on a list, model.py:1097-1110): src image i
 * at src + i * src_image_stride, dst n x [3][out_h][out_w]; one set of coefficient tables, one horizontal pass and one
 * vertical + mold pass for the whole batch. workspace: mrcnn_resize_u8_workspace_bytes(n, in_h, in_w, 3, new_h, new_w). */
int mrcnn_mold_images_u8(const uint8_t* src, int32_t n, int64_t src_image_stride, int32_t in_h, int32_t in_w, int32_t new_h,
                         int32_t new_w, int32_t top, int32_t left, int32_t out_h, int32_t out_w, const double mean_pixel[3],
                         float* dst, void* workspace, size_t workspace_bytes, mrcnn_stream_t stream);
/* Replaces datalib.full_masks (data.py:287-314). For detection i: the class_ids[i] channel of its mask_h x mask_w
 * sigmoid mask (element (i,y,x,c) at masks[i*stride_n + y*stride_y + x*stride_x + c*stride_c], so both the
 * reference's [N,C,h,w] and this library's [N,h,w,C] layouts are accepted) is multiplied by 255, converted to 8 bits
 * (clamp, truncate: Image.fromarray(F).convert('L')), resized to the box's int(y2-y1) x int(x2-x1) and pasted at
 * (int(y1), int(x1)) of a zero height x width canvas; out[i][y][x] = on_value where the 8-bit value > 127, else 0
 * (on_value 1: the boolean mask of data.py:308; 255: the same mask as the 'L' image decode_masks starts from).
 * Boxes the reference cannot paste (empty, or not inside the canvas: PIL raises; a NaN or infinite coordinate) give an
 * all-zero mask, as do class ids outside [0, num_classes) — so padded detection slots (class 0, zero box) cost nothing and stay empty.
 * A NaN mask value is grey level 0 (defined here; the reference leaves it to the platform's conversion, 0 on x86).
 * mask_h, mask_w <= 64; width % 4 == 0. */
int mrcnn_paste_masks_u8(const float* masks, int64_t stride_n, int64_t stride_y, int64_t stride_x, int64_t stride_c,
                         int32_t n, int32_t mask_h, int32_t mask_w, int32_t num_classes, const int64_t* class_ids,
                         const float* boxes, int32_t height, int32_t width, int32_t on_value, uint8_t* out,
                         mrcnn_stream_t stream);
/* Bytes per store of mrcnn_paste_masks_u8 for a canvas of this width at an `out` whose address modulo 16 is out_alignment:
 * 16 (width % 16 == 0 and an aligned out) or 4. The launcher's own answer; host arithmetic only. */
int mrcnn_paste_masks_store_width(int32_t width, int32_t out_alignment);
/* COCO run-length encoding of n single-channel 8-bit masks — replaces maskUtils.encode(np.asfortranarray(mask)) per
 * detection in build_coco_results (coco.py:40-60): rleEncode, rleToString, rleArea and rleToBbox of
 * cocoapi/common/maskApi.c applied to the mask binarised as byte > threshold (0: the 0/1 and 0/255 masks of
 * mrcnn_paste_masks_u8; 127: the grey levels decode_masks returns, the full_masks threshold of data.py:308).
 *   masks   mask i at masks + i*image_stride, rows row_stride bytes apart (>= width), pixels contiguous: a cropped view
 *           needs no copy. Pixels are visited in column-major order j = x*height + y; counts = diff([0, transitions.., H*W]).
 *   num_runs      int32 [n]               the true number of runs, also beyond capacity
 *   counts        uint32 [n][capacity]    run lengths (off run first: a mask whose first pixel is on starts with 0); may be NULL
 *   strings       uint8 [n][6*capacity]   rleToString's characters, no terminator; may be NULL
 *   string_bytes  int32 [n]               length of the string
 *   areas         int32 [n]               on pixels;   bboxes int32 [n][4]  tight (x, y, w, h), zeros for an empty mask
 * A mask with more runs than capacity: num_runs, areas and bboxes are exact, string_bytes is 0, and its counts and strings
 * rows are not written at all; the other masks of the call are unaffected. Nothing is written past a row's capacity.
 * Fixed capacity per mask: no mask depends on another, no atomics decide a position (same bits from run to run), no host sync.
 * 1 <= height, width <= 16384; n <= 65535 (0: nothing is launched); threshold in [0,254]; capacity >= 1.
 * workspace: mrcnn_rle_workspace_bytes(n, height, width) bytes of device memory, 16-byte aligned. */
size_t mrcnn_rle_workspace_bytes(int32_t n, int32_t height, int32_t width);
int mrcnn_rle_encode_u8(const uint8_t* masks, int64_t image_stride, int64_t row_stride, int32_t n, int32_t height,
                        int32_t width, int32_t threshold, int32_t capacity, int32_t* num_runs, uint32_t* counts,
                        uint8_t* strings, int32_t* string_bytes, int32_t* areas, int32_t* bboxes, void* workspace,
                        size_t workspace_bytes, mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * COCO evaluation — replaces the per-pair and per-group work of COCOeval.evaluate()
 * (cocoapi/PythonAPI/pycocotools/cocoeval.py:122-162): maskUtils.iou (rleIou / bbIou of cocoapi/common/maskApi.c:77-120)
 * and the matching loop of evaluateImg (cocoeval.py:251-300). csrc/cocoeval.hip.
 *
 * All three entry points are GROUPED: one call serves `groups` = K groups, a group being one (image, category).
 *   dt_off   int32 [K+1]   group k owns detections   [dt_off[k], dt_off[k+1]) of the detection table (n_dt rows)
 *   gt_off   int32 [K+1]   and ground truths          [gt_off[k], gt_off[k+1]) of the ground-truth table (n_gt rows)
 *   out_off  int64 [K+1]   its IoU matrix starts at element out_off[k] (non-decreasing; out_off[k+1] - out_off[k] >= m*n)
 * all in device memory. The matrix of a group of m detections and n ground truths is maskApi's o[g*m + d] (detection
 * fastest: what _mask.pyx:239 reshapes to [m, n] in Fortran order). A group with m == 0 or n == 0 writes nothing, and so do
 * elements of `out` (out_len doubles) that belong to no group's matrix. Offsets that point outside the tables read nothing.
 *
 * mrcnn_rle_iou_f64: rleIou on two run-list tables in the layout mrcnn_rle_encode_u8 writes — counts uint32 [n][capacity]
 *   (off run first), num_runs int32 [n]. iscrowd uint8 [n_gt] or NULL. Every value has the bits of rleIou:
 *   (double)i / (double)u with i the intersection pixels and u the union pixels (the detection's area where the ground truth
 *   is a crowd; 1 when i == 0). A pair in which either mask has num_runs > capacity (the encoder wrote no counts for it)
 *   gets -1, the reference's "cannot compare" value; nothing is read past a row's capacity. Contract: both masks of a pair
 *   cover the same pixel count (< 2^32) and have no zero-length runs other than a leading one.
 *   workspace: mrcnn_rle_iou_workspace_bytes(n_dt, dt_capacity, n_gt, gt_capacity) bytes of device memory, 16-byte aligned.
 * mrcnn_bbox_iou_f64: bbIou on float64 (x, y, w, h) boxes [n][4], operation by operation (no FMA contraction).
 * mrcnn_coco_match: evaluateImg's matching for every group x area range x IoU threshold in one launch.
 *   ious, ious_len        the matrices above (out / out_len of an IoU call with the same offsets)
 *   dt_area  double [n_dt]; gt_area double [n_gt]; gt_iscrowd uint8 [n_gt] (the ground truth's `ignore`, cocoeval.py:109-110)
 *   area_ranges double [A][2], thresholds double [T]: device memory, used as those very doubles
 *   the detections of a group are already sorted by descending score (stable) and cut at maxDet
 *   dt_match int32 [A][T][n_dt], gt_match int32 [A][T][n_gt]: the matched partner's 1-based position within the group in
 *   INPUT order (0 = none); dt_ignore uint8 [A][T][n_dt]; gt_ignore uint8 [A][n_gt]. Every element that belongs to a group
 *   is written. The ground truths are visited regular first, then ignored, each in input order (the stable argsort of
 *   cocoeval.py:258); the host applies that permutation when it builds evalImgs.
 * No atomics (same bits from run to run), no allocation, no host synchronisation.
 * ---------------------------------------------------------------------------------------------- */
size_t mrcnn_rle_iou_workspace_bytes(int32_t n_dt, int32_t dt_capacity, int32_t n_gt, int32_t gt_capacity);
int mrcnn_rle_iou_f64(const int32_t* dt_num_runs, const uint32_t* dt_counts, int32_t n_dt, int32_t dt_capacity,
                      const int32_t* gt_num_runs, const uint32_t* gt_counts, int32_t n_gt, int32_t gt_capacity,
                      const uint8_t* iscrowd, const int32_t* dt_off, const int32_t* gt_off, const int64_t* out_off,
                      int32_t groups, double* out, int64_t out_len, void* workspace, size_t workspace_bytes,
                      mrcnn_stream_t stream);
int mrcnn_bbox_iou_f64(const double* dt_boxes, int32_t n_dt, const double* gt_boxes, int32_t n_gt, const uint8_t* iscrowd,
                       const int32_t* dt_off, const int32_t* gt_off, const int64_t* out_off, int32_t groups, double* out,
                       int64_t out_len, mrcnn_stream_t stream);
int mrcnn_coco_match(const double* ious, int64_t ious_len, const int32_t* dt_off, const int32_t* gt_off,
                     const int64_t* out_off, int32_t groups, const double* dt_area, int32_t n_dt, const double* gt_area,
                     const uint8_t* gt_iscrowd, int32_t n_gt, const double* area_ranges, int32_t num_ranges,
                     const double* thresholds, int32_t num_thresholds, int32_t* dt_match, int32_t* gt_match,
                     uint8_t* dt_ignore, uint8_t* gt_ignore, mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * COCO polygon ground truth to run lengths — replaces COCO.annToRLE's per-annotation maskUtils.frPyObjects + maskUtils.merge
 * (pycocotools/coco.py:406-425): rleFrPoly / rleFrBbox and rleMerge of cocoapi/common/maskApi.c:162-202, :49-70, for all
 * parts of a data set in one call each. csrc/poly.hip. Run-list tables are in the layout mrcnn_rle_encode_u8 writes and
 * mrcnn_rle_iou_f64 reads: num_runs int32 [n], counts uint32 [n][capacity]. Every count has the bits of the reference's
 * codec (fp64, operation by operation, no FMA contraction). No allocation, no host synchronisation; the same bits from
 * run to run.
 *
 * mrcnn_rle_from_poly_f64: rleFrPoly for n polygon parts.
 *   xy        double [total_vertices][2]  all parts' vertices, x then y
 *   vert_off  int32 [n+1]                 part i owns vertices [vert_off[i], vert_off[i+1])
 *   heights, widths  int32 [n]            every part has its own image size
 *   num_runs  int32 [n]                   the true number of runs, also beyond capacity
 *   counts    uint32 [n][capacity]        a part with more runs than capacity: its row is not written; the other parts
 *                                         are unaffected and nothing is written past a row (the encoder's rule)
 *   num_keys  int32 [n]                   the column crossings kept before the parity rule. A part with at most
 *                                         mrcnn_rle_from_poly_onchip_keys() of them is sorted on chip in one piece; one
 *                                         with more is sorted range by range of the key space (same bits).
 *   Limits. Checked on the host (an error): 0 <= n <= 2^22, 0 <= total_vertices <= 2^28, capacity >= 1. The values in
 *   device memory cannot be read without a synchronisation, so a part past one of the following limits is refused ON THE
 *   DEVICE: it reports num_runs = num_keys = -1, writes nothing else and reads nothing outside its arrays —
 *   1 <= height, width <= 16384; 0 <= vert_off[i] < vert_off[i+1] <= total_vertices (at least one vertex);
 *   every coordinate finite with |5*v + .5| < 2^31; at most 2^24 boundary points (sum over the edges of
 *   max(|dX|, |dY|) + 1 in the 5x grid), so that every point index fits int32. (ops.rle_from_poly checks the same limits
 *   on the host whenever it reads the arguments.)
 *   n == 0 launches nothing. workspace: mrcnn_rle_from_poly_workspace_bytes(n, total_vertices), 16-byte aligned.
 *
 * mrcnn_rle_merge: rleMerge for `groups` groups: group g merges rows [group_off[g], group_off[g+1]) of the input table
 *   (group_off int32 [groups+1] in device memory) into row g of the output table [groups][out_capacity]; intersect 0 =
 *   union, 1 = intersection. The output is canonical: only a leading run may be empty and the last run reaches the end.
 *   A group of one row is a copy; an empty group gives num_runs = 0; a group with more runs than out_capacity reports its
 *   true num_runs and its row is not written; a group containing a row that was over ITS capacity (or whose offsets point
 *   outside the table) reports num_runs = -1 and writes nothing. Contract on the input, as for mrcnn_rle_iou_f64: the rows
 *   of a group cover the same pixel count (< 2^32) and only a leading run may be empty.
 *   workspace: mrcnn_rle_merge_workspace_bytes(n_rows, capacity), 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
int32_t mrcnn_rle_from_poly_onchip_keys(void);
size_t mrcnn_rle_from_poly_workspace_bytes(int32_t n, int32_t total_vertices);
int mrcnn_rle_from_poly_f64(const double* xy, int32_t total_vertices, const int32_t* vert_off, const int32_t* heights,
                            const int32_t* widths, int32_t n, int32_t capacity, int32_t* num_runs, uint32_t* counts,
                            int32_t* num_keys, void* workspace, size_t workspace_bytes, mrcnn_stream_t stream);
size_t mrcnn_rle_merge_workspace_bytes(int32_t n_rows, int32_t capacity);
int mrcnn_rle_merge(const int32_t* num_runs, const uint32_t* counts, int32_t n_rows, int32_t capacity,
                    const int32_t* group_off, int32_t groups, int32_t intersect, int32_t out_capacity,
                    int32_t* out_num_runs, uint32_t* out_counts, void* workspace, size_t workspace_bytes,
                    mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The rest of the COCO RLE codec on run-list TABLES — rleFrString, rleToString, rleArea + rleToBbox and rleDecode of
 * cocoapi/common/maskApi.c:218-231, :204-216, :72-75 + :133-147, :43-47 — for n rows in one call each. csrc/codec.hip.
 * Tables are in the layout mrcnn_rle_encode_u8 writes: num_runs int32 [n], counts uint32 [n][capacity], off run first. A row
 * with num_runs < 0 (refused) or num_runs > capacity (never written) is called UNUSABLE below. Strings travel packed:
 * bytes uint8 [total], str_off int64 [n+1]; string i is bytes[str_off[i] : str_off[i+1]), not NUL-terminated, possibly empty.
 * Every value has the bits of the reference's codec. No allocation, no host synchronisation, no atomics; the same bits from run
 * to run. Host-checked limits (an error): 0 <= n <= 2^24 (mrcnn_rle_decode_u8: 65535), capacity >= 1. n == 0 launches nothing
 * (mrcnn_rle_to_string still writes str_off[0] = 0).
 *
 * mrcnn_rle_from_string: rleFrString for n strings. A token ends at a character c with (c - 48) & 0x20 == 0; its value is the
 *   little-endian 5-bit groups, sign-extended when the last group has 0x10; cnts[m] = x[m] + cnts[m-2] for m > 2, in uint32
 *   wrap-around. heights / widths int32 [n] are used for the checks only. status int32 [n] is a bit set:
 *     refused on the device — num_runs = -1, the row untouched, the other rows unaffected:
 *       1  a byte outside 48..111          2  a token longer than 6 characters (the reference's int shift is undefined from
 *       4  the string ends inside a token     the seventh; a difference of a mask of at most 2^28 pixels fits in 6)
 *       8  height or width outside [1, 16384]      64  str_off[i] > str_off[i+1], or outside [0, total_bytes]
 *     flagged, the row still written:
 *       16 an empty run after the first    32 the runs' sum (taken in 64 bits) differs from heights[i] * widths[i]
 *   A row with more runs than capacity reports its true num_runs and status 0 and is not written (the encoder's rule; bits
 *   16 and 32 are not computed for it). Nothing is written past num_runs in a row.
 * mrcnn_rle_area_bbox: rleArea and rleToBbox of every row: areas int32 [n], bboxes int32 [n][4] (x, y, w, h), the encoder's
 *   types, with per-row heights / widths. uint32 arithmetic as the reference's, its quirks kept: m = (m/2)*2 (the last run of
 *   an odd row is ignored), m == 0 gives four zeros, t = cc - j%2, an on run whose end lies in a later column than its start
 *   sets ys = 0, ye = h-1. An unusable row, or one with a height or width outside [1, 16384], gets area -1 and bbox -1.
 * mrcnn_rle_to_string: rleToString of every row into the packed buffer bytes [bytes_capacity]. str_off [n+1] always holds the
 *   true offsets, str_off[n] the true total; an unusable row contributes 0 bytes. A row with str_off[i+1] > bytes_capacity is
 *   not written, and nothing is written past the buffer (bytes may be NULL with bytes_capacity 0: offsets only).
 *   row_stride > 0 selects the encoder's fixed-stride layout instead of the packed one: row i is written at bytes +
 *   i*row_stride (str_off still holds the packed offsets, so str_off[i+1] - str_off[i] is its length); a row longer than
 *   row_stride, or whose slot crosses bytes_capacity, is not written. have_offsets = 1: str_off already holds the offsets of
 *   THIS table (an earlier call wrote them) and only the write pass is launched.
 *   workspace: mrcnn_rle_to_string_workspace_bytes(n), 16-byte aligned.
 * mrcnn_rle_decode_u8: rleDecode of n rows of ONE size into row-major 0 / 1 masks: mask i at out + i*image_stride, rows
 *   row_stride bytes apart (>= width), pixels contiguous (what mrcnn_rle_encode_u8 reads). Every byte of every mask is written
 *   and none outside; runs past height*width are clipped, pixels the runs do not reach are 0, an unusable row decodes to zeros.
 *   1 <= height, width <= 16384. workspace: mrcnn_rle_decode_workspace_bytes(n, capacity), 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
int mrcnn_rle_from_string(const uint8_t* bytes, int64_t total_bytes, const int64_t* str_off, const int32_t* heights,
                          const int32_t* widths, int32_t n, int32_t capacity, int32_t* num_runs, uint32_t* counts,
                          int32_t* status, mrcnn_stream_t stream);
int mrcnn_rle_area_bbox(const int32_t* num_runs, const uint32_t* counts, int32_t n, int32_t capacity, const int32_t* heights,
                        const int32_t* widths, int32_t* areas, int32_t* bboxes, mrcnn_stream_t stream);
size_t mrcnn_rle_to_string_workspace_bytes(int32_t n);
int mrcnn_rle_to_string(const int32_t* num_runs, const uint32_t* counts, int32_t n, int32_t capacity, uint8_t* bytes,
                        int64_t bytes_capacity, int64_t row_stride, int32_t have_offsets, int64_t* str_off, void* workspace,
                        size_t workspace_bytes, mrcnn_stream_t stream);
size_t mrcnn_rle_decode_workspace_bytes(int32_t n, int32_t capacity);
int mrcnn_rle_decode_u8(const int32_t* num_runs, const uint32_t* counts, int32_t n, int32_t capacity, int32_t height,
                        int32_t width, uint8_t* out, int64_t image_stride, int64_t row_stride, void* workspace,
                        size_t workspace_bytes, mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Ground-truth masks for training straight from run-length rows — what CocoMaskRCNNDataset.load and encode_masks do per
 * annotation on the host (data.py:797-876, :246-262: annToMask, np.fliplr, a Pillow BILINEAR Resize, a zero Pad) — for n rows of
 * a table (the layout and the UNUSABLE-row rule of the codec block above) with PER-ROW sizes, in one call. csrc/gt_masks.hip.
 *   heights, widths  int32 [n]     each row's source size
 *   geom             int32 [n][5]  (new_h, new_w, top, left, flip) per row
 *   out              uint8: mask k at out + k*image_stride, rows row_stride bytes apart (>= out_w), pixels contiguous. Every
 *                    byte of the out_h x out_w extent of every mask is written and none outside it.
 * Mask k on [top, top+new_h) x [left, left+new_w) is numpy.array(Image.fromarray(m).resize((new_w, new_h), Image.BILINEAR)),
 * m being rleDecode of the row at heights[k] x widths[k] (runs past h*w clipped, pixels the runs do not reach 0), mirrored left
 * to right when flip != 0 — Pillow's bits: fp64 coefficients, 22-bit fixed point, the 8-bit intermediate of its horizontal pass
 * with its rounding. An axis whose new size equals its source size is not resampled, as Pillow skips that pass. The mask is 0
 * elsewhere. status int32 [n] is a bit set; a row with a bit set is REFUSED — its mask all zeros, the other rows unaffected:
 *     1  an unusable row                          2  heights / widths / new_h / new_w outside [1, 16384]
 *     4  the placement is not inside the canvas   8  a source size above 16 times the new size, on either axis
 * Two launches whatever n is and however many sizes occur; no allocation, no host synchronisation, no atomics, the same bits
 * from run to run. Neither a dense source mask nor the horizontal pass's intermediate is written to memory: workspace —
 * mrcnn_rle_resample_workspace_bytes(n, capacity), 16-byte aligned — holds the run-end positions only.
 * Host-checked limits (an error): 0 <= n <= 65535, capacity >= 1, 1 <= out_h, out_w <= 16384. n == 0 launches nothing.
 * ---------------------------------------------------------------------------------------------- */
size_t mrcnn_rle_resample_workspace_bytes(int32_t n, int32_t capacity);
int mrcnn_rle_resample_u8(const int32_t* num_runs, const uint32_t* counts, int32_t n, int32_t capacity, const int32_t* heights,
                          const int32_t* widths, const int32_t* geom, uint8_t* out, int32_t out_h, int32_t out_w,
                          int64_t image_stride, int64_t row_stride, int32_t* status, void* workspace, size_t workspace_bytes,
                          mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Rendering detections onto the image — data.blend_image / data.blend_mask (data.py:346-403: per instance a PIL Image.blend at
 * 0.2, two Image.composite and an inverted 3x3 ImageFilter.CONTOUR with the frame zeroed, then ImageDraw.rectangle at width 1)
 * without the labels, the bits Pillow gives, in ONE launch. csrc/overlay.hip.
 *   image   uint8 [height][width][3], rows image_row_stride bytes apart;  out likewise, rows out_row_stride bytes apart
 *   masks   uint8, mask i at masks + i*mask_image_stride, rows mask_row_stride bytes apart, pixels contiguous; a pixel is ON
 *           where its byte > threshold (0 for 0 / 1 masks, 127 for grey levels). mask_image_stride 0 reads one mask n times.
 *   colors  uint8 [n][3];   boxes int32 [n][4] (y0, x0, y1, x1), or NULL: no rectangles
 * For each pixel p, px starting as the image's, for i = 0 .. n-1 in order:
 *   mask i on at p:  px = (uint8) trunc(float(px) + 0.2f * float(int(c_i) - int(px))) per channel, in fp32 (no FMA)
 *   else:            px = c_i if one of p's 8 neighbours is on in mask i (outside the image: off) and p is not on the image
 *                    frame (0 < y < height-1, 0 < x < width-1) — so an image with height < 3 or width < 3 has no outline.
 * Then the rectangles for i = 0 .. n-1 in order (a later one overwrites an earlier one): rows y0 and y1 over columns x0..x1,
 * columns x0 and x1 over rows min(y0+1, y1) .. max(y0+1, y1) (Pillow's: a box with y0 == y1 also colours row y0+1 at its two end
 * columns), clipped to the image; y0+1 is taken in 64 bits, so any int32 coordinates are safe. y1 < y0 or x1 < x0 draws nothing.
 * Every byte of out's height x 3*width region is written and none outside it; n == 0 copies the image. out == image with equal
 * row strides is allowed (a pixel reads only its own image bytes); any other overlap of out with an input is the caller's error.
 * Host-checked limits (an error): 1 <= height, width <= 16384; 0 <= n <= 65535; 0 <= threshold <= 254; image_row_stride and
 * out_row_stride >= 3*width; mask_row_stride >= width; mask_image_stride >= 0. Operands whose base and strides are multiples of
 * 16 bytes are read and written 16 bytes at a time (masks on their own, image and out together), the others byte by byte: the
 * same bits. No workspace, no allocation, no host synchronisation, no atomics; the same bits from run to run.
 * ---------------------------------------------------------------------------------------------- */
int mrcnn_blend_instances_u8(const uint8_t* image, int64_t image_row_stride, const uint8_t* masks, int64_t mask_image_stride,
                             int64_t mask_row_stride, const uint8_t* colors, const int32_t* boxes, int32_t n, int32_t height,
                             int32_t width, int32_t threshold, uint8_t* out, int64_t out_row_stride, mrcnn_stream_t stream);

/* RPN conv_shared + both 1x1 heads in one launch on the Winograd kernel (RPN.forward, model.py:605-607,624-641):
 * relu(conv3x3_same(x) * scale + shift) is never stored — each 64-channel output tile is transposed through LDS and
 * multiplied by w_head32 ([32][cout]: rows 0..17 = conv_class (6) then conv_bbox (12) weights, other rows zero) while
 * on chip; a workgroup owns whole M tiles and adds the contribution of each of its cout/64 N tiles to the M tile's sums.
 *   x_kblocked  fp32 [cin/8][batch][H][W][8];  u = mrcnn_winograd_weights_f32 of the [cout][3][3][cin] filter
 *   tile_mode   1: an M tile is 64 consecutive tile positions; 2: an 8 x 8 block of positions of one image (the faster
 *               kernel; maps of at least 8 x 8 positions). mrcnn_conv3x3_winograd_heads_tile_mode(H, W) returns the
 *               recommended one (follows mrcnn_winograd_set_spatial).
 *   head_part   fp32 [2][rows][32], rows = mrcnn_conv3x3_winograd_heads_rows(batch, H, W, tile_mode): the two k halves of
 *               the sums (without the head bias); row of pixel (b,y,x): mode 1 = ((b*H/2 + y/2)*W/2 + x/2)*4 + (y&1)*2 +
 *               (x&1); mode 2 = mt*256 + ((y/2 & 7)*8 + (x/2 & 7))*4 + (y&1)*2 + (x&1) with mt the block index
 *               (b*ceil(H/16) + y/16)*ceil(W/16) + x/16 — the input forms 1 / 2 of mrcnn_rpn_scores_deltas_v2_f32.
 *               Fully overwritten; no zero-fill needed.
 *   H, W even; cin % 8 == 0; cout % 64 == 0. Deterministic (fixed summation order). */
int64_t mrcnn_conv3x3_winograd_heads_rows(int32_t batch, int32_t height, int32_t width, int32_t tile_mode);
int32_t mrcnn_conv3x3_winograd_heads_tile_mode(int32_t height, int32_t width);
int mrcnn_conv3x3_winograd_heads_f32(const float* x_kblocked, int32_t batch, int32_t height, int32_t width, int32_t cin,
                                     const float* u, int32_t cout, const float* scale, const float* shift,
                                     int32_t activation, const float* w_head32, int32_t tile_mode, float* head_part,
                                     mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Whole-block fused Bottleneck — replaces the module composite  Bottleneck.forward  (model.py:190-211):
 *   out = relu( bn3(conv3(relu(bn2(conv2_same(relu(bn1(conv1(x)))))))) + x )
 * for the stride-1 IDENTITY blocks (no downsample branch) with planes = 64 and Cin = 4 * planes = 256 (ResNet C2 blocks
 * after the first): ONE launch, both 64-channel intermediates stay in LDS (csrc/bottleneck.hip). BatchNorm (eval) and
 * the conv biases are the folded fp32 (scale, shift) epilogues; conv2 runs as Winograd F(2x2,3x3) on the fp32 MFMA.
 * The result equals the three-launch path (mrcnn_conv_bn_act_f32 → mrcnn_conv3x3_winograd_f32 → mrcnn_conv_bn_act_f32
 * with residual) bit for bit.
 *   x   fp32 [batch][height][width][cin] NHWC;  y  fp32 [batch][height][width][4*planes], y != x
 *   w1  [planes][cin] (conv1, OHWI 1x1);  u2 = mrcnn_winograd_weights_f32(conv2 weights [planes][3][3][planes]);
 *   w3  [4*planes][planes] (conv3, OHWI 1x1);  scaleN, shiftN: per output channel of conv N (NULL = 1 / 0)
 * mrcnn_bottleneck_fused_supported() tells whether a shape is covered (planes == 64, cin == 256, height and width
 * multiples of 16); other blocks run the per-layer entry points.
 * ---------------------------------------------------------------------------------------------- */
int mrcnn_bottleneck_fused_supported(int32_t height, int32_t width, int32_t cin, int32_t planes);
int mrcnn_bottleneck_fused_f32(const float* x, int32_t batch, int32_t height, int32_t width, int32_t cin,
                               const float* w1, const float* scale1, const float* shift1, const float* u2,
                               const float* scale2, const float* shift2, const float* w3, const float* scale3,
                               const float* shift3, int32_t planes, float* y, mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Bottleneck.forward as ONE call — replaces the module composite  Bottleneck.forward  (model.py:174-211, downsample branch
 * :254-262) for EVERY block of the trunk; the implementation of torch.ops.maskrcnn.bottleneck_forward (csrc/bottleneck_op.hip).
 * The call plans the block and enqueues its launches on `stream`:
 *   ResNet C2 (planes = 64, maps of >= winograd4_min_tiles tiles of 16 x 32 pixels per image, u4 given, fuse_conv3 != 0):
 *       conv1 (+ downsample) on the direct kernel, then conv2 + conv3 + residual + ReLU in ONE launch
 *       (mrcnn_conv3x3_winograd4_conv3_f32): 2 launches per identity block;
 *   elsewhere: conv1 (+ downsample), conv2 by F(4x4) (u4, same size rule) / F(2x2) (u2, even maps) Winograd or, with neither
 *       transform given, the exact direct kernel, then conv3 + residual + ReLU: 3 (4) launches.
 * The plan depends on the shape per image and on which transforms are passed, never on the batch.
 *   x   fp32 NHWC [batch][height][width][cin];  y  fp32 NHWC [batch][ceil(H/s)][ceil(W/s)][4*planes], y != x
 *   weights[14] (device pointers, fp32; scale / shift = folded BatchNorm + bias per output channel, NULL = 1 / 0):
 *       0 w1 [planes][cin]          1 scale1   2 shift1
 *       3 w2 [planes][3][3][planes] (OHWI)     4 u2 = mrcnn_winograd_weights_f32(w2) or NULL     5 u4 = mrcnn_winograd4_weights_f32(w2) or NULL
 *       6 scale2   7 shift2         8 w3 [4*planes][planes]   9 scale3   10 shift3
 *       11 wd [4*planes][cin] or NULL (identity block: stride 1, cin == 4*planes)   12 scale_d   13 shift_d
 *   workspace: >= mrcnn_bottleneck_workspace_bytes(...) bytes of device memory, 256-byte aligned (the block's intermediates).
 * ---------------------------------------------------------------------------------------------- */
size_t mrcnn_bottleneck_workspace_bytes(int32_t batch, int32_t height, int32_t width, int32_t cin, int32_t planes,
                                        int32_t stride, int32_t has_downsample);
/* The plan mrcnn_bottleneck_forward_f32 follows for these arguments, as bits: 1 = conv2 on the F(4x4) kernel, 2 = conv2 on the
 * F(2x2) kernel (neither: direct kernel), 4 = conv2 + conv3 + residual in one launch; -1 = bad shape. */
int32_t mrcnn_bottleneck_plan(int32_t batch, int32_t height, int32_t width, int32_t cin, int32_t planes, int32_t stride,
                              int32_t have_u2, int32_t have_u4, int32_t winograd4_min_tiles, int32_t fuse_conv3);
int mrcnn_bottleneck_forward_f32(const float* x, int32_t batch, int32_t height, int32_t width, int32_t cin, int32_t planes,
                                 int32_t stride, const float* const weights[14], int32_t winograd4_min_tiles,
                                 int32_t fuse_conv3, void* workspace, size_t workspace_bytes, float* y, mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * RPN training targets — replaces  data.rpn_samples(anchors, gt_class_ids, gt_boxes, config)  (data.py:449-591, called per item
 * at data.py:727) and its IoU helper  data.boxes_overlaps  (data.py:151-189), for a batch of B images (csrc/targets.hip).
 *
 * Shared by the three calls: anchors fp64 [A][4] (y1,x1,y2,x2), the reference's create_pyramid_anchors, one set for the batch;
 * ground truth packed as the grouped calls of this library pack it: gt_boxes fp32 [M][4], gt_class_ids int32 [M], gt_off int32
 * [B+1] (image b owns rows gt_off[b] .. gt_off[b+1]). The rule for one image:
 *   1 crowd rule: with an id < 0 in the image, crowd rows = id < 0, kept rows = id > 0, id == 0 dropped; without one every row is
 *     kept. no_crowd[a] = (max IoU of a over the crowd rows) < crowd_iou (true where there is no crowd row).
 *   2 IoU of every anchor, NARROWED to fp32 (round to nearest), with every kept row, fp32, each operation rounded on its own:
 *     y1 = max(a_y1, g_y1) ..., inter = max(x2-x1, 0) * max(y2-y1, 0), union = (a_area + g_area) - inter, inter / union correctly
 *     rounded. 3 iou_argmax[a] = the FIRST kept row with the largest IoU, iou_max[a] that IoU.
 *   4 match[a] = -1 where iou_max[a] < neg_iou and no_crowd[a], else 0. 5 for every kept row the FIRST anchor with the largest
 *     IoU gets match 1 (a row no anchor touches: anchor 0). 6 match[a] = 1 where iou_max[a] >= pos_iou.
 *   7 more than count/2 positives: the ones with the smallest (key, anchor index) stay, the rest become 0. 8 more than
 *     count - (positives left) negatives: likewise. (The reference draws the ones to reset with np.random.choice; here the caller
 *     hands in one non-negative int32 key per anchor — independent uniform keys give the same distribution.)
 *   9 deltas of the positives in ascending anchor index against kept row iou_argmax[a], NumPy >= 2 promotion: gt_h = g_y2 - g_y1
 *     and gt_cy = g_y1 + 0.5f * gt_h in fp32; a_h, a_cy from the fp64 anchors; dy = ((double)gt_cy - a_cy) / a_h, dh =
 *     log((double)gt_h / a_h) (dx, dw alike), each divided by its fp64 std_dev and narrowed to fp32. A zero-height box: -inf.
 * Preconditions for the reference's values: finite anchors with positive area, finite boxes with y2 >= y1, x2 >= x1. On anything
 * else the calls stay memory-safe: every index is checked, row offsets are clamped into [0, M] and to 1024 rows per image.
 * Limits: A in [1, 2^24], B in [1, 65535], B * A < 2^31, M <= 1024 * B (at most 1024 rows per image), count >= 1.
 * No call synchronises with the host; the number of launches does not depend on B. Workspaces: device memory, 16-byte aligned.
 * (mrcnn_sample_by_key_workspace_bytes: the histograms of the radix select, about 14.5 KB per image.)
 *
 * mrcnn_anchor_match — steps 1-6.
 *   match int32 [B][A]; iou_argmax int32 [B][A]: the row's position within its image (counting all of the image's rows);
 *   iou_max fp32 [B][A]; gt_argmax int32 [M]: step 5's anchor, -1 for crowd and dropped rows; status int32 [B]: bit 0 = the image
 *   has no kept row (the reference's np.argmax raises): its match is 0, iou_argmax -1, iou_max 0.
 * mrcnn_sample_by_key — steps 7-8 on match int32 [B][A] with keys int32 [B][A] → out int32 [B][A] (out == match: in place).
 * mrcnn_rpn_deltas — step 9: rpn_bbox fp32 [B][count][4] (16-byte aligned; rows past the positives are 0), num_pos int32 [B] the
 *   number of positives of the image. Positives beyond `count` rows are not written (they occur only when the sampling was
 *   skipped); num_pos still counts them. std_dev: 4 host doubles.
 * ---------------------------------------------------------------------------------------------- */
size_t mrcnn_anchor_match_workspace_bytes(int32_t num_rows);
int mrcnn_anchor_match(const double* anchors, int32_t num_anchors, const float* gt_boxes, const int32_t* gt_class_ids,
                       const int32_t* gt_off, int32_t num_rows, int32_t batch, float neg_iou, float pos_iou, float crowd_iou,
                       int32_t* match, int32_t* iou_argmax, float* iou_max, int32_t* gt_argmax, int32_t* status,
                       void* workspace, size_t workspace_bytes, mrcnn_stream_t stream);
size_t mrcnn_sample_by_key_workspace_bytes(int32_t batch);
int mrcnn_sample_by_key(const int32_t* match, const int32_t* keys, int32_t batch, int32_t num_anchors, int32_t count,
                        int32_t* out, void* workspace, size_t workspace_bytes, mrcnn_stream_t stream);
size_t mrcnn_rpn_deltas_workspace_bytes(int32_t batch, int32_t num_anchors);
int mrcnn_rpn_deltas(const double* anchors, int32_t num_anchors, const float* gt_boxes, const int32_t* gt_off, int32_t num_rows,
                     int32_t batch, const int32_t* match, const int32_t* iou_argmax, int32_t count, const double std_dev[4],
                     float* rpn_bbox, int32_t* num_pos, void* workspace, size_t workspace_bytes, mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Detection training targets — replaces  model.mrn_samples(rpn_rois, gt_class_ids, gt_boxes, gt_masks, config)  (model.py:396-576,
 * called from MaskRCNN.extract at model.py:1270; batch size 1 there) for a batch of B images (csrc/detection_targets.hip).
 *
 * Inputs: rois fp32 [B][N][4] (y1,x1,y2,x2), one N for the batch; zero rows are ordinary RoIs, as in the reference. Ground truth
 * packed as for mrcnn_anchor_match: gt_boxes fp32 [M][4] in the RoIs' coordinates (the reference normalises both), gt_class_ids
 * int32 [M], gt_off int32 [B+1]. gt_masks [M][H][W], one byte per pixel (uint8 / bool: the byte's value as a float) or fp32; row m
 * is the mask of ground-truth row m; one H x W for the call. keys int32 [B][N], non-negative. The rule for one image:
 *   1 crowd rule, exactly as mrcnn_anchor_match step 1 (crowd_iou is 0.001 in the reference): with an id < 0 in the image, crowd
 *     rows = id < 0, kept rows = id > 0, id == 0 dropped; without one every row is kept, id 0 included. An image without a kept row
 *     gets status bit 0, num_pos = num_neg = 0 and outputs that are all 0 / -1 (the reference raises there).
 *   2 IoU of every RoI with every kept row: boxes_overlaps (data.py:151-189) in fp32, every operation rounded on its own, the
 *     division correctly rounded, no contraction. iou_max[r] = the largest, gt_index[r] = the FIRST kept row that has it
 *     (torch.max(dim=1) on the CPU takes the first), counted within ALL of the image's rows.
 *   3 a RoI is positive where iou_max >= pos_iou (0.5), negative where iou_max < pos_iou and its largest IoU over the crowd rows
 *     is < crowd_iou, otherwise neither.
 *   4 pos_limit = (int)((double)count * positive_ratio) (Python's int(count * ratio): 100, 0.33 -> 33). The positives with the
 *     smallest (key, roi index) are kept, at most pos_limit, and written IN THAT ORDER (the reference's
 *     positive_indices[randperm][:pos_limit] is a random order; the key order stands in for it, as in mrcnn_sample_by_key).
 *     num_pos = the number kept.
 *   5 num_pos == 0: nothing is kept at all (the reference's "BugFixed" rule, model.py:516). Otherwise neg_limit =
 *     (int)(r * num_pos - num_pos) with r = 1.0 / positive_ratio, in fp64, the product and the difference rounded separately,
 *     truncated (0.33: 0, 2, 4, ... 62, 64, 67 for num_pos = 0 ... 33). The negatives with the smallest (key, roi index), at most
 *     neg_limit (and at most count - num_pos: memory safety only), follow the positives in that order. num_neg = their number.
 *   6 outputs, count rows per image; rows past num_pos + num_neg are 0 (indices -1):
 *       rois_out fp32 [B][count][4]: the chosen RoIs' bits.   target_class_ids int32 [B][count]: the id of row gt_index for a
 *       positive, 0 for a negative.   target_deltas fp32 [B][count][4]: boxes_deltas (data.py:103-121) in fp32 operation by
 *       operation — h = y2 - y1, cy = y1 + 0.5f * h for the RoI and the row, dy = (gt_cy - cy) / h, dh = log(gt_h / h) with the
 *       quotient in fp32 and the logarithm in fp64, narrowed — then each divided by its fp32 std_dev; 0 for a negative.
 *       roi_index int32 [B][count]: the RoI's position in its image.   gt_index int32 [B][count]: the matched row's position in
 *       its image for a positive, -1 for a negative.   num_pos, num_neg, status int32 [B].
 *   7 mask targets (mrcnn_mask_targets_*): target_mask fp32 [B][count][mh][mw]. For a positive slot s it is
 *     CropFunction(mh, mw, 0) — crop_per_box, crop_cpu.cpp:13-116, the arithmetic of mrcnn_crop_forward_f32 — of mask
 *     gt_off[b] + gt_index[s] with box rois_out[s], then torch.round (ties to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2). Every other
 *     slot is zeros. The mask is read in place through the index; no [P][H][W] gather exists.
 * Preconditions for the reference's values: finite boxes with y2 >= y1, x2 >= x1, and no RoI / row pair whose union is 0 (the
 * reference gives NaN there; here such a pair never wins a maximum). On anything else the calls stay memory-safe: row offsets are
 * clamped into [0, M] and to 1024 rows per image, every index read from memory (gt_index, num_pos) is checked before it is
 * followed, mask offsets are computed in 64 bits.
 * Limits: N in [1, 4096], at most 1024 rows per image (M <= 1024 * B), count in [1, 1024], B in [1, 65535], H, W in [1, 16384],
 * mh, mw in [1, 64], positive_ratio in (0, 1]. No call synchronises with the host; each call is ONE launch, whatever B is, and
 * needs no workspace.
 *
 * mrcnn_detection_targets — steps 1-6. std_dev: 4 host floats.
 * mrcnn_mask_targets_u8 / _f32 — step 7 for byte / fp32 masks; rois_out, gt_index, num_pos as mrcnn_detection_targets wrote them.
 * ---------------------------------------------------------------------------------------------- */
int mrcnn_detection_targets(const float* rois, const float* gt_boxes, const int32_t* gt_class_ids, const int32_t* gt_off,
                            const int32_t* keys, int32_t batch, int32_t num_rois, int32_t num_rows, int32_t count,
                            double positive_ratio, float pos_iou, float crowd_iou, const float std_dev[4], float* rois_out,
                            int32_t* target_class_ids, float* target_deltas, int32_t* roi_index, int32_t* gt_index,
                            int32_t* num_pos, int32_t* num_neg, int32_t* status, mrcnn_stream_t stream);
int mrcnn_mask_targets_u8(const uint8_t* gt_masks, int32_t num_rows, int32_t height, int32_t width, const int32_t* gt_off,
                          int32_t batch, int32_t count, const float* rois_out, const int32_t* gt_index, const int32_t* num_pos,
                          int32_t mask_height, int32_t mask_width, float* target_mask, mrcnn_stream_t stream);
int mrcnn_mask_targets_f32(const float* gt_masks, int32_t num_rows, int32_t height, int32_t width, const int32_t* gt_off,
                           int32_t batch, int32_t count, const float* rois_out, const int32_t* gt_index, const int32_t* num_pos,
                           int32_t mask_height, int32_t mask_width, float* target_mask, mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Training losses — replace  RPN.class_loss / RPN.boxes_loss  (model.py:652-718),  Classifier.class_loss / Classifier.boxes_loss
 * (model.py:802-845) and  Mask.mask_loss  (model.py:922-953), the five losses train_epoch adds up (model.py:1622-1629), forward and
 * backward for a batch of B images (csrc/losses.hip). They read the padded [B][count][...] outputs of the target calls above in
 * place: no torch.nonzero, no gather, no host read.
 *
 * The rule. Every contributing element's term and derivative is evaluated in fp64 from the fp32 inputs. The terms of an image are
 * summed in fp64 in a FIXED order by store-and-sum: a workgroup writes its partial sum with plain stores, a later launch adds the
 * partials in index order (each thread a run of consecutive partials, the runs in thread order); no floating-point atomic, no
 * ticket or last-block protocol — two calls on the same inputs return the same bits. Quotients and gradients are narrowed to fp32
 * last. The per-element definitions are those of the stock torch functions the reference calls:
 *   cross entropy (RPN class loss over 2 logits, head class loss over C): term log(sum_j exp(x_j - max)) - (x_c - max);
 *     derivative softmax(x)_j - [j == c].
 *   smooth L1, beta 1, d = pred - target: term 0.5 d^2 if |d| < 1, else |d| - 0.5; derivative d if |d| < 1, else sign(d).
 *   binary cross entropy on a probability p with target y (y need not be 0 or 1):
 *     term -(y max(log p, -100) + (1 - y) max(log(1 - p), -100)), log(1 - p) taken as log1p(-p) as torch takes it;
 *     derivative (p - y) / max(p (1 - p), 1e-12).
 * Which elements contribute, for image b:
 *   RPN class loss: anchors with match != 0, class 1 if match == 1, else 0. count: n_cls[b].
 *   RPN box loss: anchors with match == 1 in ascending anchor index, the k-th paired with target_bbox[b][k][:] (mrcnn_rpn_deltas
 *     writes them in that order); 4 elements each, count 4 P[b]. A positive whose rank is >= count has no target row: it is left
 *     out and bit 0 of status[b] is set.
 *   head class loss: slots s < num_rois[b] (the caller passes num_pos + num_neg; clamped into [0, count]), class
 *     target_class_ids[b][s]; padding slots never contribute, whatever their logits hold. A class id outside 0 .. C-1 sets status
 *     bit 1 and the slot is skipped in all three losses.
 *   head box loss: those slots with target_class_ids > 0: pred_bbox[b][s][class][:] against target_deltas[b][s][:].
 *   mask loss: the same slots: pred_masks[b][s][class][:][:] against target_mask[b][s][:][:], mh * mw elements per slot.
 * An element that does not contribute is never read into the arithmetic (a select, not a multiply by zero): a NaN or Inf in a
 * neutral anchor's logits, in a padding slot or in another class's plane changes nothing.
 * Reductions are the caller's: the calls return per loss the per-image fp64 sums and int32 counts. loss = sum / count over the
 * batch ("mean": the reference's functions on the concatenation of the images, the reference itself at B = 1) or per image.
 * DEVIATION: a loss without a contributing element is 0 with all-zero gradients. The reference's head losses say so themselves
 * for an empty input, but F.cross_entropy / F.smooth_l1_loss / F.binary_cross_entropy over nothing — its RPN losses on an image
 * without a sampled anchor, its head box and mask losses on negatives only — return NaN, the mean of nothing.
 * The backward calls write EVERY element of the dense gradients (a non-contributing element is +0) with full-width stores, and
 * scale by the upstream gradient and the forward's counts, both read from device memory: grad_out fp32 [kLosses] and the counts
 * summed over the batch (per_image == 0), or grad_out fp32 [B][kLosses] and the image's own counts (per_image != 0).
 * Limits: A in [1, 2^24], B in [1, 65535], B * A < 2^31, count in [1, 1024], C in [2, 4096], mh, mw in [1, 64]; offsets are 64-bit.
 * No call synchronises with the host or allocates; two launches forward and one backward per family, whatever B is.
 * Alignment: float4 rows (pred_bbox, target_bbox, target_deltas, grad_bbox) 16 bytes, RPN logits and their gradient 8, workspaces 8.
 *
 * mrcnn_rpn_loss_forward: match int32 [B][A], logits fp32 [B][A][2], pred_bbox fp32 [B][A][4], target_bbox fp32 [B][count][4] →
 *   sums fp64 [B][2] (class, box), counts int32 [B][2] (n_cls, 4 min(P, count)), status int32 [B], and chunk_pos int32
 *   [B][mrcnn_rpn_loss_chunks(A)]: the positives of each chunk of 1024 anchors, from which the backward call ranks the positives
 *   in its single launch (the scan over match == 1 across workgroups, as mrcnn_rpn_deltas does it). Only the contributing anchors'
 *   logits and deltas are loaded; the pass over the rest reads match alone.
 * mrcnn_rpn_loss_backward → grad_logits fp32 [B][A][2], grad_bbox fp32 [B][A][4]; chunk_pos and counts as the forward wrote them.
 * mrcnn_head_loss_forward: target_class_ids int32 [B][count], num_rois int32 [B], target_deltas fp32 [B][count][4], target_mask
 *   fp32 [B][count][mh][mw], logits fp32 [B][count][C], pred_bbox fp32 [B][count][C][4], pred_masks fp32 [B][count][C][mh][mw]
 *   (the reference's [R, C, ...] with R = B * count) → sums fp64 [B][3] (class, box, mask), counts int32 [B][3] (slots, 4 positives,
 *   mh mw positives), status int32 [B]. One workgroup per slot stores the slot's three partial sums; a second launch adds the
 *   slots of each image in slot order.
 * mrcnn_head_loss_backward → grad_logits, grad_bbox, grad_masks in the predictions' shapes: zeros but the slot's logits row, the
 *   class's row of pred_bbox and the class's plane of pred_masks; the mask gradient is written with 16-byte stores.
 * The classifier alone: target_mask and pred_masks may BOTH be null (and then grad_masks must be). The mask sum and count are 0
 *   and no mask gradient is written; the class and box columns, their launches and their bits are those of the full call.
 * ---------------------------------------------------------------------------------------------- */
int32_t mrcnn_rpn_loss_chunks(int32_t num_anchors);
size_t mrcnn_rpn_loss_workspace_bytes(int32_t batch, int32_t num_anchors, int32_t count);
int mrcnn_rpn_loss_forward(const int32_t* match, const float* logits, const float* pred_bbox, const float* target_bbox,
                           int32_t batch, int32_t num_anchors, int32_t count, double* sums, int32_t* counts, int32_t* status,
                           int32_t* chunk_pos, void* workspace, size_t workspace_bytes, mrcnn_stream_t stream);
int mrcnn_rpn_loss_backward(const int32_t* match, const float* logits, const float* pred_bbox, const float* target_bbox,
                            const int32_t* chunk_pos, const int32_t* counts, const float* grad_out, int32_t per_image,
                            int32_t batch, int32_t num_anchors, int32_t count, float* grad_logits, float* grad_bbox,
                            mrcnn_stream_t stream);
size_t mrcnn_head_loss_workspace_bytes(int32_t batch, int32_t count);
int mrcnn_head_loss_forward(const int32_t* target_class_ids, const int32_t* num_rois, const float* target_deltas,
                            const float* target_mask, const float* logits, const float* pred_bbox, const float* pred_masks,
                            int32_t batch, int32_t count, int32_t num_classes, int32_t mask_height, int32_t mask_width,
                            double* sums, int32_t* counts, int32_t* status, void* workspace, size_t workspace_bytes,
                            mrcnn_stream_t stream);
int mrcnn_head_loss_backward(const int32_t* target_class_ids, const int32_t* num_rois, const float* target_deltas,
                             const float* target_mask, const float* logits, const float* pred_bbox, const float* pred_masks,
                             const int32_t* counts, const float* grad_out, int32_t per_image, int32_t batch, int32_t count,
                             int32_t num_classes, int32_t mask_height, int32_t mask_width, float* grad_logits, float* grad_bbox,
                             float* grad_masks, mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Clipped SGD (csrc/optim.hip): what the reference does after every loss.backward() (model.py:1542-1557, 1632-1637) —
 * torch.nn.utils.clip_grad_norm_(parameters, max_norm), then on every BATCH_SIZE-th iteration optim.SGD(momentum, weight decay on
 * the non-BN group only).step() and zero_grad() — on a table of T tensors in three launches, whatever T is.
 *
 * The rule. Tensor t has an fp32 parameter p, an fp32 gradient g, an fp32 momentum buffer b, all of numel_t elements, and an fp64
 * weight decay wd_t; lr, momentum and max_norm are fp64 and shared.
 *   1. S = the sum over every element of every tensor that has a gradient of double(g) * double(g). A product is exact in fp64. S
 *      is summed in fp64 in a FIXED order, a function of the sizes and their order in the table alone (neither of the grid nor of
 *      timing), by store-and-sum as the losses above: tensor t is cut into tiles of TILE = mrcnn_optim_tile() consecutive elements,
 *      the last one short; a tile's 256 threads each add their elements — thread k owns elements (256 i + k) 4 + j of the tile,
 *      i = 0 .. TILE / 1024 - 1 outer, j = 0 .. 3 inner, in that order from +0 —, the thread sums are added per wave by the shuffle
 *      scan of csrc/workgroup.hpp (lane 63's value: the balanced tree over the 64 lanes) and the wave sums in wave order; the tile
 *      sum is stored. A finishing launch of one workgroup of 256 threads adds the tile sums in index order: thread k the run
 *      [k chunk, (k + 1) chunk), chunk = ceil(tiles / 256), then the runs by the same scan. No floating-point atomic, no ticket.
 *   2. norm = sqrt(S), c = min(1, max_norm / (norm + 1e-6)), both in fp64: clip_grad_norm_'s formula.
 *   3. DEVIATION: if S is not finite (NaN or +Inf), bit 0 of status is set and the apply launch leaves parameters, momentum buffers
 *      and (modes clip and step) gradients untouched; a requested zeroing of the gradients still happens. In the reference the NaN
 *      flows into every weight.
 *   4. Otherwise, per element in fp64 from the fp32 inputs, each operation rounded on its own, narrowed last:
 *        d = c g + wd_t p,  B = momentum b + d,  b' = fp32(B),  p' = fp32(p - lr B) (from the unrounded B),  g' = fp32(c g).
 *      torch's SGD with dampening 0 and nesterov False; a zero buffer gives B = d, torch's clone on the first step.
 * mode 0 (clip) writes g' only; 1 (step) writes p', b' and g'; 2 (step_zero) writes p', b' and +0 into g. A store of g' that would
 * not change a bit (c == 1) is left out. A tensor whose gradient address is 0 is skipped entirely — no decay, no momentum update, no
 * term in S —, as torch skips grad is None. A tensor of 0 elements is legal.
 *
 * The tensor table lives in device memory: table int64 [T][4] = (address of p, address of g or 0, address of b, numel), wd fp64
 * [T], tile_off int64 [T + 1] = the exclusive prefix sum of ceil(numel_t / TILE) (a skipped tensor keeps its tiles: tile_off
 * depends on the sizes only), tiles = tile_off[T]. A workgroup finds its tile's tensor by a uniform binary search in tile_off.
 * Tensors whose three addresses are 16-byte aligned are read and written with 16-byte accesses, the others element by element;
 * both forms give the same bits. Element offsets are 64-bit.
 *
 * mrcnn_optim_clip_coef: steps 1-3 in two launches → info fp64 [3] = (S, norm, c), status int32 [1]. workspace: tiles doubles of
 *   device memory, 8-byte aligned.
 * mrcnn_optim_sgd_apply: step 4 in one launch; c and status are read from device memory (info, status: as clip_coef wrote them,
 *   on the same stream; null: c = 1 and no non-finite check — max_norm None).
 * Limits, checked before any launch: T in [1, 65535], tiles in [0, 2^24], max_norm > 0, lr finite, momentum in [0, 1), mode in
 * 0 .. 2. What only the table's builder can see — numel_t < 2^31, wd_t finite, tile_off as defined — is the builder's to check.
 * No call synchronises with the host or allocates.
 * ---------------------------------------------------------------------------------------------- */
int32_t mrcnn_optim_tile(void);
int mrcnn_optim_clip_coef(const int64_t* table, const int64_t* tile_off, int32_t num_tensors, int64_t tiles, double max_norm,
                          double* workspace, double* info, int32_t* status, mrcnn_stream_t stream);
int mrcnn_optim_sgd_apply(const int64_t* table, const double* wd, const int64_t* tile_off, int32_t num_tensors, int64_t tiles,
                          const double* info, const int32_t* status, double lr, double momentum, int32_t mode,
                          mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The RPN's training branch on the sampled anchors alone (csrc/rpn_train.hip). The reference's RPN losses read the anchors with
 * rpn_match != 0 only (model.py:652-718: torch.nonzero, then gathers), and nothing else carries a gradient into the RPN (the
 * proposals are made from .data, model.py:1349-1365). So the shared 3x3 conv and the two 1x1 heads are differentiated on those
 * anchors alone: their 3x3xC input patches are gathered into GEMM rows, and the patch gradients are scattered back into the maps.
 *
 * Anchor order is mrcnn_rpn_scores_deltas_v2_f32's: level l has H_l x W_l pixels and apl anchors per pixel, anchor
 * a = first[l] + (y W_l + x) apl + r with first[0] = 0, first[l+1] = first[l] + H_l W_l apl; A = first[levels].
 *
 * mrcnn_anchor_compact: match int32 [batch][num_anchors] -> index int32 [batch][capacity], num int32 [batch], status int32 [batch].
 *   index[b] holds the anchors of image b with match != 0 in ASCENDING anchor index (so the k-th positive in anchor order is still
 *   the k-th positive of the compacted row, which is how mrcnn_rpn_loss_forward pairs it with target_bbox[b][k]); num[b] =
 *   min(capacity, their number); the slots at or past num[b] are -1. status bit 0: the image has more than capacity such anchors
 *   (the first capacity are kept). One launch of one workgroup per image, whatever batch is; no host synchronisation.
 *
 * mrcnn_pyramid_patch_gather_f32: maps[l] fp32 [batch][H_l][W_l][channels] (NHWC) -> patches fp32 [batch * capacity][9 * channels].
 *   Row (b, k) with anchor index[b][k] on pixel (py, px) of level l holds, at (ky 3 + kx) channels + c, the value
 *   maps[l][b][py + ky - 1][px + kx - 1][c]: SamePad2d(3, 1) and the 3x3 window, in the order in which an OHWI weight
 *   [Cout][3][3][channels] flattens, so that weight viewed as [Cout][1][1][9 channels] is the GEMM's. A tap outside the map is +0.
 *   A slot k >= num[b], or whose index is outside [0, A), is an empty slot: all +0. EVERY byte of patches is written. It is a
 *   copy: the bits of the map, -0 and NaN payloads included. One launch.
 *
 * mrcnn_pyramid_patch_scatter_f32: the gather's backward. dpatch fp32 [batch * capacity][9 * channels] -> grad_maps[l] fp32
 *   [batch][H_l][W_l][channels]; a null grad_maps[l] means that level's gradient is not needed. The rule, bit for bit:
 *   grad_maps[l][b][y][x][c] is the fp32 sum, starting from +0, each add separately rounded, in ascending slot k < num[b], over the
 *   entries index[b][k] of level l whose pixel (py, px) has |py - y| <= 1 and |px - x| <= 1, of dpatch[b][k][y - py + 1][x - px + 1][c].
 *   The thread that owns a map element takes that sum itself (map-stationary, as mrcnn_roi_align_pyramid_backward_f32): no atomic,
 *   no memset beforehand — EVERY byte of every requested map is written, +0 where nothing lands —, two calls give the same bits,
 *   and an image's gradient does not depend on the rest of the batch. The rows of empty slots are never read. index[b][0, num[b])
 *   must be ascending, as mrcnn_anchor_compact writes it (the entries that can reach a pixel are then three contiguous ranges, one
 *   per map row, whose ends are the numbers of entries below six keys); a row that is not is memory-safe and its gradient unspecified. One launch (none when
 *   every grad_maps[l] is null).
 *
 * Limits, checked before any launch: levels in [1, 8], every H_l and W_l in [1, 16384], channels % 4 == 0, anchors_per_location in
 * [1, 16], capacity in [1, 1024], batch in [1, 65535], batch * num_anchors < 2^31 (compact), A < 2^31, every map and the patch
 * matrix 16-byte aligned and at most 2^30 elements (the 4 GiB range of the conv forward). No call synchronises with the host or
 * allocates.
 * ---------------------------------------------------------------------------------------------- */
int mrcnn_anchor_compact(const int32_t* match, int32_t batch, int32_t num_anchors, int32_t capacity, int32_t* index, int32_t* num,
                         int32_t* status, mrcnn_stream_t stream);
int mrcnn_pyramid_patch_gather_f32(const float* const maps[8], const int32_t map_h[8], const int32_t map_w[8], int32_t levels,
                                   int32_t batch, int32_t channels, int32_t anchors_per_location, const int32_t* index,
                                   const int32_t* num, int32_t capacity, float* patches, mrcnn_stream_t stream);
int mrcnn_pyramid_patch_scatter_f32(const float* dpatch, const int32_t map_h[8], const int32_t map_w[8], int32_t levels,
                                    int32_t batch, int32_t channels, int32_t anchors_per_location, const int32_t* index,
                                    const int32_t* num, int32_t capacity, float* const grad_maps[8], mrcnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The mask head's class-plane branch in training (csrc/mask_train.hip). Mask.mask_loss (model.py:922-953) gathers, of the positive
 * slots, the plane of the slot's own class, and nothing else carries a gradient into the mask head. So conv5 (the 1x1 conv to C
 * planes) and the loss are computed for ONE plane per slot, on the first P slots of an image alone (mrcnn_detection_targets puts
 * the positives first).
 *
 * Notation. S = batch * P plane slots, P = plane_slots per image, 1 <= P <= count. Plane slot (b, s) belongs to target slot (b, s)
 * of the [batch][count] target tensors ids (target_class_ids) and target_mask, which are read in place with stride count; num is
 * int32 [batch] (num_pos, or num_pos + num_neg: a negative's id is 0), clamped into [0, count]. Q = mask_height * mask_width.
 * Slot (b, s) is ACTIVE when s < min(num[b], P) and 0 < ids[b][s] < C; k = ids[b][s] is its class. The data of a slot that is not
 * active — its rows of x, y, dy, p and target_mask — is never read, whatever it holds.
 * status int32 [batch] (the forward calls): bit 1 (value 2): a class id outside 0 .. C-1 in a slot below num[b], as
 * mrcnn_head_loss_forward reports it (the slot is skipped); bit 2 (value 4): a slot s >= P below num[b] with ids > 0, a positive the
 * planes have no room for (left out).
 *
 * mrcnn_class_plane_conv_f32: x fp32 [S][mh][mw][cin] (NHWC), w fp32 [C][cin], bias fp32 [C] or null -> y fp32 [S][mh][mw].
 *   Active slot: z = fp32(double(bias[k]) + T) (z = fp32(T) without a bias), T the fp64 sum of the products double(x[..][c]) *
 *   double(w[k][c]), each exact in fp64, in this order, a function of cin alone: lane l of 64 adds, from +0, the channels
 *   4 (l + 64 i) + j for i = 0, 1, .. outer and j = 0 .. 3 inner (a lane without a channel holds +0); then the lane sums
 *   meet in a butterfly, v[l] = v[l] + v[l xor d] for d = 32, 16, 8, 4, 2, 1, each add rounded in fp64. y = z for act 0;
 *   y = 1.0f / (1.0f + expf(-z)) for act 2, the sigmoid epilogue of the conv forward (the library is built without fast-math, so the
 *   same bits). A slot that is not active: its y rows are +0. EVERY byte of y is written. One launch.
 * mrcnn_class_plane_conv_backward_f32: dy and y fp32 [S][mh][mw] (y read at act 2 only, may be null at act 0), x, w as above ->
 *   dx fp32 [S][mh][mw][cin], dw fp32 [C][cin], dbias fp32 [C], each optional (null: not needed; x may be null when dw is).
 *   g = dy at act 0; at act 2 t = 1 - y, u = y t, g = dy u, three separately rounded fp32 operations (mrcnn_conv_act_backward_f32's
 *   rule). dx[s][q][c] = g[s][q] w[k][c], one fp32 product: what the dense data gradient gives, an fmaf chain whose other terms
 *   are zero. dw[k][c] = fp32(the fp64 sum, from +0 in ascending (b, s), over the active slots of class k of D[s][c]), with D[s][c]
 *   the fp64 sum of the exact products double(g[s][q]) double(x[s][q][c]) in this order, a function of Q alone: the pixels are cut
 *   into chunks of 64; within a chunk v = 0 .. 3 adds the pixels 64 chunk + v + 4 j, j ascending, from +0, and the four sums are
 *   added as ((v0 + v1) + v2) + v3; the chunk sums are added from +0 in ascending chunk. dbias[k] is the same with g alone. Rows
 *   of a class without an active slot, dx rows of a slot that is not active: +0. EVERY byte of every requested output is written.
 *   Store-and-sum: one pass over x writes dx and the per-(slot, chunk) sums into the workspace
 *   (mrcnn_class_plane_conv_backward_workspace_bytes, 8-byte aligned; not needed for dx alone); a finishing launch has the owner
 *   of (k, c) add its class's slots, found by ballots over ids. Two launches whatever batch is (one for dx alone); two calls give
 *   the same bits.
 * mrcnn_mask_plane_loss_forward: p fp32 [batch][P][mh][mw], target_mask fp32 [batch][count][mh][mw] -> sums fp64 [batch], counts
 *   int32 [batch] (Q x the active slots), status. Term and derivative are the mask rule of mrcnn_head_loss_forward, word for word
 *   and in the same code (csrc/loss_math.hpp): binary cross entropy in fp64 from the fp32 p, max(log p, -100), log1p(-p);
 *   derivative (p - y) / max(p (1 - p), 1e-12). A slot's terms are summed as there (thread t of 256 adds elements t, t + 256, ..,
 *   then the workgroup sum), and a second launch adds an image's slots in slot order: sums equals the mask column of
 *   mrcnn_head_loss_forward on the dense tensor bit for bit. An empty loss is 0. workspace: mrcnn_mask_plane_loss_workspace_bytes.
 * mrcnn_mask_plane_loss_backward -> grad_p fp32 [batch][P][mh][mw] in one launch: the derivative times grad_out / count in fp64,
 *   narrowed last; grad_out fp32 [1] and the counts summed over the batch (per_image == 0) or grad_out fp32 [batch] and the image's
 *   own count (per_image != 0), both read from device memory; 0 for an empty loss. Slots that are not active: +0. EVERY byte written.
 *
 * Limits, checked before any launch: batch in [1, 65535], count in [1, 1024], P in [1, count], C in [2, 4096], mh and mw in [1, 64],
 * cin % 4 == 0 in [4, 4096], act 0 or 2; x, dx and w 16-byte aligned; offsets are 64-bit. No floating-point atomic, no memset, no
 * last-block ticket; no call synchronises with the host or allocates.
 * ---------------------------------------------------------------------------------------------- */
int mrcnn_class_plane_conv_f32(const float* x, const float* w, const float* bias, const int32_t* ids, const int32_t* num,
                               int32_t batch, int32_t count, int32_t plane_slots, int32_t num_classes, int32_t mask_height,
                               int32_t mask_width, int32_t cin, int32_t act, float* y, int32_t* status, mrcnn_stream_t stream);
size_t mrcnn_class_plane_conv_backward_workspace_bytes(int32_t batch, int32_t plane_slots, int32_t mask_height, int32_t mask_width,
                                                       int32_t cin);
int mrcnn_class_plane_conv_backward_f32(const float* dy, const float* y, const float* x, const float* w, const int32_t* ids,
                                        const int32_t* num, int32_t batch, int32_t count, int32_t plane_slots, int32_t num_classes,
                                        int32_t mask_height, int32_t mask_width, int32_t cin, int32_t act, float* dx, float* dw,
                                        float* dbias, void* workspace, size_t workspace_bytes, mrcnn_stream_t stream);
size_t mrcnn_mask_plane_loss_workspace_bytes(int32_t batch, int32_t plane_slots);
int mrcnn_mask_plane_loss_forward(const float* p, const float* target_mask, const int32_t* ids, const int32_t* num, int32_t batch,
                                  int32_t count, int32_t plane_slots, int32_t num_classes, int32_t mask_height, int32_t mask_width,
                                  double* sums, int32_t* counts, int32_t* status, void* workspace, size_t workspace_bytes,
                                  mrcnn_stream_t stream);
int mrcnn_mask_plane_loss_backward(const float* p, const float* target_mask, const int32_t* ids, const int32_t* num,
                                   const int32_t* counts, const float* grad_out, int32_t per_image, int32_t batch, int32_t count,
                                   int32_t plane_slots, int32_t num_classes, int32_t mask_height, int32_t mask_width, float* grad_p,
                                   mrcnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MASKRCNN_HIP_H */
