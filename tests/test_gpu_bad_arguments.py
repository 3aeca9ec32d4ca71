"""Every binding refuses a malformed tensor argument BEFORE anything is launched: tiny valid calls with exactly one thing wrong —
a wrong dtype, one dimension off by one, one rank too few, or (for `out=`) a view of the right shape with other strides. Each
refusal is a RuntimeError that starts with the op's name and names the argument, and ops.CONV_PROFILE, switched on around the call,
stays empty. The rows are refusals that the wrappers made before the binding modules were split (then partly as `assert`); the
float4 readers (the losses) repair a misaligned tensor rather than refuse it, so alignment has no row."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, F32, F64, I32, I64, U8 = torch.float16, torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
OTHER = {F32: F64, F64: F32, I32: I64, I64: I32, U8: I32, F16: F32, torch.bool: I32}


def dev(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def zeros(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def other_strides(t):
    """A view of t's shape and dtype that is not contiguous: the last two dimensions transposed, or every second element."""
    if t.dim() >= 2:
        v = torch.zeros(*t.shape[:-2], t.shape[-1], t.shape[-2], dtype=t.dtype, device=t.device).transpose(-1, -2)
    else:
        v = torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)[::2]
    assert v.shape == t.shape and not v.is_contiguous(), "the row needs a shape whose transposed view is not contiguous"
    return v


FAULTS = {
    "dtype": lambda t: t.to(OTHER[t.dtype]),
    "rank": lambda t: t[0],
    "view": other_strides,
    **{f"dim{d}": (lambda t, d=d: torch.cat([t, t.narrow(d, 0, 1)], d)) for d in range(5)},
    "short": lambda t: t[:-1],
}


@functools.lru_cache(maxsize=None)
def table():
    from maskrcnn_amd import ops
    masks = zeros(3, 4, 5, dtype=U8)
    masks[0, 1:3, 1:4] = 1
    masks[1, :, 2] = 1
    masks[2, 3, :] = 1
    enc = ops.rle_encode(masks)
    return masks, enc[0], enc[1]


@functools.lru_cache(maxsize=None)
def case(name):
    """(callable, keyword arguments) of a tiny VALID call: B = 2, A = N = 8, M = 3, masks 4 x 5, count 4, C = 3."""
    from maskrcnn_amd import ops
    masks, nr, counts = table()
    offs = dict(dt_off=dev([0, 3], I32), gt_off=dev([0, 3], I32), out_off=dev([0, 9], I64), out_len=9)
    sizes = dict(heights=dev([4, 4, 4], I32), widths=dev([5, 5, 5], I32))
    boxes = dev([[1, 1, 2, 2], [0, 0, 3, 3], [2, 1, 2, 3]], F64)
    anchors = dev([[i, i, i + 4, i + 5] for i in range(8)], F64)
    gt = dict(gt_boxes=dev([[0, 0, 4, 5], [2, 2, 9, 9], [1, 3, 6, 8]], F32), gt_off=dev([0, 2, 3], I32))
    ids = dev([1, 2, 1], I32)
    maps = dict(match=dev([[1, -1, 0, 1, -1, -1, 0, 1], [-1, 1, 1, 0, -1, -1, -1, 0]], I32), keys=dev(np.arange(16).reshape(2, 8), I32))
    rpn = dict(match=maps["match"], logits=zeros(2, 8, 2), pred_bbox=zeros(2, 8, 4), target_bbox=zeros(2, 4, 4))
    head = dict(target_class_ids=dev([[1, 2, 0, 0], [2, 0, 0, 0]], I32), num_rois=dev([3, 2], I32), target_deltas=zeros(2, 4, 4),
                target_mask=zeros(2, 4, 4, 4), logits=zeros(2, 4, 3), pred_bbox=zeros(2, 4, 3, 4), pred_masks=zeros(2, 4, 3, 4, 4))
    x, w = zeros(1, 8, 8, 64), zeros(64, 1, 1, 64)
    xk, u4 = zeros(8, 1, 8, 8, 8), zeros(16, 36, 2, 64, 2)
    if name == "rle_encode":
        return ops.rle_encode, dict(masks=masks)
    if name == "rle_iou":
        return ops.rle_iou, dict(dt=(nr, counts), gt=(nr, counts), iscrowd=dev([0, 1, 0], U8), **offs, out=zeros(9, dtype=F64))
    if name == "bbox_iou":
        return ops.bbox_iou, dict(dt=boxes, gt=boxes, iscrowd=dev([0, 1, 0], U8), **offs, out=zeros(9, dtype=F64))
    if name == "coco_match":
        return ops.coco_match, dict(ious=zeros(9, dtype=F64), dt_off=offs["dt_off"], gt_off=offs["gt_off"], out_off=offs["out_off"],
                                    dt_area=dev([4, 9, 2], F64), gt_area=dev([4, 9, 2], F64), gt_iscrowd=dev([0, 1, 0], U8),
                                    area_ranges=dev([[0, 1e10], [0, 32]], F64), thresholds=dev([0.5, 0.75], F64),
                                    out=(zeros(2, 2, 3, dtype=I32), zeros(2, 2, 3, dtype=I32), zeros(2, 2, 3, dtype=U8), zeros(2, 3, dtype=U8)))
    if name == "rle_from_poly":
        tri = [[0, 0], [3, 0], [0, 3]]
        return ops.rle_from_poly, dict(xy=dev(tri + tri, F64), vert_off=dev([0, 3, 6], I32), heights=dev([4, 4], I32),
                                       widths=dev([5, 5], I32), capacity=8)
    if name == "rle_merge":
        return ops.rle_merge, dict(num_runs=nr, counts=counts, group_off=dev([0, 2, 3], I32), capacity=21)
    if name == "rle_from_string":
        data, str_off = ops.rle_to_string(nr, counts)
        return ops.rle_from_string, dict(bytes=data, str_off=str_off, **sizes, capacity=21)
    if name == "rle_area_bbox":
        return ops.rle_area_bbox, dict(num_runs=nr, counts=counts, **sizes)
    if name == "rle_to_string":
        return ops.rle_to_string, dict(num_runs=nr, counts=counts, total_bytes=64)
    if name == "rle_to_string_rows":
        return ops.rle_to_string_rows, dict(num_runs=nr, counts=counts)
    if name == "rle_decode":
        return ops.rle_decode, dict(num_runs=nr, counts=counts, height=4, width=5, out=zeros(3, 4, 5, dtype=U8))
    if name == "anchor_match":
        return ops.anchor_match, dict(anchors=anchors, gt_boxes=gt["gt_boxes"], gt_class_ids=ids, gt_off=gt["gt_off"])
    if name == "sample_by_key":
        return ops.sample_by_key, dict(**maps, count=4, out=zeros(2, 8, dtype=I32))
    if name == "rpn_deltas":
        return ops.rpn_deltas, dict(anchors=anchors, **gt, match=maps["match"], iou_argmax=zeros(2, 8, dtype=I32), count=4)
    if name == "detection_targets":
        out = (zeros(2, 4, 4), zeros(2, 4, dtype=I32), zeros(2, 4, 4), zeros(2, 4, dtype=I32), zeros(2, 4, dtype=I32),
               zeros(2, dtype=I32), zeros(2, dtype=I32), zeros(2, dtype=I32))
        return ops.detection_targets, dict(rois=zeros(2, 8, 4), gt_boxes=gt["gt_boxes"], gt_class_ids=ids, gt_off=gt["gt_off"],
                                           keys=maps["keys"], count=4, out=out)
    if name == "mask_targets":
        return ops.mask_targets, dict(gt_masks=masks, gt_off=gt["gt_off"], rois_out=zeros(2, 4, 4), gt_index=zeros(2, 4, dtype=I32),
                                      num_pos=dev([1, 1], I32), mask_shape=(4, 4), out=zeros(2, 4, 4, 4))
    if name == "rpn_loss":
        return ops.rpn_loss, rpn
    if name == "rpn_loss_backward":
        _, cnt, _, chunk_pos = ops.rpn_loss(**rpn)
        return ops.rpn_loss_backward, dict(**rpn, chunk_pos=chunk_pos, counts=cnt, grad_out=zeros(2))
    if name == "head_loss":
        return ops.head_loss, head
    if name == "head_loss_backward":
        return ops.head_loss_backward, dict(**head, counts=zeros(2, 3, dtype=I32), grad_out=zeros(3))
    # the inference side: one 1 x 8 x 8 x 64 conv input
    if name == "conv_bn_act":
        return ops.conv_bn_act, dict(x=x, w=w, scale=zeros(64), shift=zeros(64), residual=zeros(1, 8, 8, 64), out=zeros(1, 8, 8, 64))
    if name == "conv_bn_act_rows":
        return ops.conv_bn_act, dict(x=x, w=w, scale=None, shift=None, row_counts=dev([8], I32), rows_per_group=64)
    if name == "conv_bn_act_f16mfma":
        return ops.conv_bn_act_f16mfma, dict(x=x, w_hi=w.half(), w_lo=w.half(), scale=None, shift=None, residual=zeros(1, 8, 8, 64))
    if name == "conv_f16_pipelined":
        return ops.conv_f16_pipelined, dict(x=x.half(), w=w.half(), scale=None, shift=None, residual=zeros(1, 8, 8, 64, dtype=F16))
    if name == "pack_afrags_f16":
        return ops.pack_afrags_f16, dict(w=w.half())
    if name == "maxpool":
        return ops.maxpool, dict(x=x, kernel=1, stride=2)
    if name == "nchw_to_nhwc":
        return ops.nchw_to_nhwc, dict(x=x)
    if name == "nhwc_to_nchw":
        return ops.nhwc_to_nchw, dict(x=x)
    if name == "nhwc_to_kblocked":
        return ops.nhwc_to_kblocked, dict(x=x)
    if name == "bottleneck_native":
        v16, v64 = zeros(16), zeros(64)
        return ops.bottleneck_native, dict(x=x, w1=zeros(16, 1, 1, 64), s1=v16, t1=v16, w2=zeros(16, 3, 3, 16), u2=None, u4=None, s2=v16,
                                           t2=v16, w3=zeros(64, 1, 1, 16), s3=v64, t3=v64, wd=None, sd=None, td=None, stride=1)
    if name == "bottleneck_fused":
        v16, v64 = zeros(16), zeros(64)
        return ops.bottleneck_fused, dict(x=x, w1=zeros(16, 1, 1, 64), s1=v16, t1=v16, u2=zeros(16, 16, 16), s2=v16, t2=v16,
                                          w3=zeros(64, 1, 1, 16), s3=v64, t3=v64)
    if name == "bottleneck_c2_f16":
        h16 = lambda n: zeros(n, dtype=F16)
        return ops.bottleneck_c2_f16, dict(x=zeros(1, 8, 8, 256, dtype=F16), w1f=h16(64 * 256), s1=zeros(64), t1=zeros(64), w2f=h16(64 * 576),
                                           s2=zeros(64), t2=zeros(64), w3f=h16(256 * 64), s3=zeros(256), t3=zeros(256))
    if name == "mask_tail_f16":
        return ops.mask_tail_f16, dict(x=zeros(2, 4, 4, 256, dtype=F16), wde_frags=zeros(1024 * 256, dtype=F16), bias_de4=zeros(1024),
                                       w5_frags=zeros(96 * 256, dtype=F16), bias5=zeros(3))
    if name == "conv_f16_pipelined_heads":
        return ops.conv_f16_pipelined_heads, dict(x=x.half(), w=zeros(512, 3, 3, 64, dtype=F16), scale=None, shift=None,
                                                  w_head32=zeros(32, 512, dtype=F16))
    if name == "conv3x3_winograd_heads":
        return ops.conv3x3_winograd_heads, dict(x_kblocked=zeros(8, 1, 16, 16, 8), u=zeros(16, 64, 64), scale=None, shift=None,
                                                w_head32=zeros(32, 64))
    if name == "conv3x3_winograd4_heads":
        return ops.conv3x3_winograd4_heads, dict(x_kblocked=xk, u4=u4, scale=None, shift=None, w_head32=zeros(32, 64))
    if name == "stem_pool_f16":
        return ops.stem_pool_f16, dict(x=zeros(1, 3, 8, 8), w=zeros(64, 7, 7, 4), scale=None, shift=None)
    if name == "detection_decode":
        return ops.detection_decode, dict(logits=zeros(8, 3), bbox=zeros(8, 3, 4), rois=zeros(2, 4, 4), roi_counts=dev([4, 4], I32),
                                          windows=zeros(2, 4), std_dev=(0.1, 0.1, 0.2, 0.2), image_height=64, image_width=64)
    if name == "mold_images_u8":
        return ops.mold_images_u8, dict(images=zeros(2, 4, 5, 3, dtype=U8), new_h=4, new_w=5, top=0, left=0, out=zeros(2, 3, 8, 8),
                                        mean_pixel=(1.0, 2.0, 3.0))
    if name == "winograd_weights":
        return ops.winograd_weights, dict(w_ohwi=zeros(64, 3, 3, 64))
    if name == "winograd4_weights":
        return ops.winograd4_weights, dict(w_ohwi=zeros(64, 3, 3, 64))
    if name == "conv3x3_winograd":
        return ops.conv3x3_winograd, dict(x=x, u=zeros(16, 64, 64), scale=None, shift=None)
    if name == "conv3x3_winograd4":
        return ops.conv3x3_winograd4, dict(x_kblocked=xk, u4=u4, scale=None, shift=None)
    if name == "conv3x3_winograd4_conv3":
        return ops.conv3x3_winograd4_conv3, dict(x_kblocked=xk, u4=u4, scale=None, shift=None, w3=zeros(256, 1, 1, 64), scale3=None,
                                                 shift3=None, residual=zeros(1, 8, 8, 256))
    if name == "stem_conv":
        return ops.stem_conv, dict(x=zeros(1, 8, 8, 4), w=zeros(64, 7, 7, 4), scale=None, shift=None)
    if name == "stem_pool_f32":
        return ops.stem_pool_f32, dict(x=zeros(1, 3, 8, 8), w=zeros(64, 7, 7, 4), scale=None, shift=None)
    if name == "deconv2x2":
        return ops.deconv2x2, dict(x=x, w=zeros(64, 1, 1, 64), bias4=zeros(64))
    if name == "topk_desc":
        return ops.topk_desc, dict(scores=zeros(2, 8), k=4)
    if name == "proposal_decode":
        return ops.proposal_decode, dict(anchors=zeros(8, 4), deltas=zeros(2, 8, 4), order=zeros(2, 4, dtype=I64), top_scores=zeros(2, 4),
                                         std_dev=(0.1, 0.1, 0.2, 0.2), image_height=64, image_width=64)
    if name == "proposal_select":
        return ops.proposal_select, dict(dets=zeros(2, 8, 5), keep=zeros(2, 8, dtype=I64), keep_counts=zeros(2, dtype=I32),
                                         proposal_count=4, image_height=64, image_width=64)
    if name == "detection_select":
        return ops.detection_select, dict(dets=zeros(2, 8, 5), nms_class_ids=zeros(2, 8, dtype=I32), class_ids=zeros(2, 8, dtype=I64),
                                          keep=zeros(2, 8, dtype=I64), keep_counts=zeros(2, dtype=I32), max_instances=4, image_height=64,
                                          image_width=64)
    if name == "nms_batched":
        return ops.nms_batched, dict(dets=zeros(2, 8, 5), threshold=0.5, seg_counts=dev([8, 8], I32), class_ids=zeros(2, 8, dtype=I32))
    if name == "nms_general":
        return ops.nms_general, dict(dets=zeros(8, 5), threshold=0.5)
    if name == "roi_align_pyramid":
        return ops.roi_align_pyramid, dict(feature_maps=[zeros(1, 8 >> i, 8 >> i, 64) for i in range(4)], rois=zeros(8, 4), pool=2,
                                           image_area=64.0, rois_per_image=8, roi_counts=dev([8], I32))
    if name == "rpn_scores_deltas":
        return ops.rpn_scores_deltas, dict(heads=[zeros(1, 8 >> i, 8 >> i, 18) for i in range(4)] + [zeros(1, 1, 1, 18)])
    if name == "mold_image_u8":
        return ops.mold_image_u8, dict(image=zeros(4, 5, 3, dtype=U8), new_h=4, new_w=5, top=0, left=0, out=zeros(3, 8, 8),
                                       mean_pixel=(1.0, 2.0, 3.0))
    if name == "paste_masks":
        return ops.paste_masks, dict(masks=zeros(3, 2, 4, 4), class_ids=dev([0, 1, 1], I64), boxes=zeros(3, 4), height=8, width=8,
                                     channels_last=False)
    if name == "blend_instances":
        return ops.blend_instances, dict(image=zeros(4, 5, 3, dtype=U8), masks=masks, colors=zeros(3, 3, dtype=U8),
                                         boxes=zeros(3, 4, dtype=I32), out=zeros(4, 5, 3, dtype=U8))
    raise KeyError(name)


def rows(name, *specs, op=None):
    """(case, op name in the message, argument — `name.i` for an entry of a tuple —, fault, what the message names)."""
    out = []
    for spec in specs:
        arg, faults = spec[0], spec[1].split()
        names = spec[2] if len(spec) > 2 else arg.split(".")[0]
        out += [pytest.param(name, op or name, arg, f, names, id=f"{name}-{arg}-{f}") for f in faults]
    return out


TABLE_ROWS = [("{}.0", "dtype rank", "num_runs"), ("{}.1", "dtype dim0 rank", "counts")]
TABLE_ARGS = [("num_runs", "dtype rank"), ("counts", "dtype dim0 rank")]
OFFSETS = [("dt_off", "dtype rank"), ("dt_off", "dim0", "_off"), ("gt_off", "dtype dim0"), ("out_off", "dtype dim0")]   # one K for the three
GROUND_TRUTH = [("gt_boxes", "dtype dim1 rank"), ("gt_off", "dtype rank")]
SIZES = [("heights", "dtype dim0 rank"), ("widths", "dtype dim0 rank")]
ROWS = (
    rows("rle_encode", ("masks", "dtype"))
    + rows("rle_iou", *[(a.format(t), f, n) for t in ("dt", "gt") for a, f, n in TABLE_ROWS], ("iscrowd", "dtype dim0 rank"), *OFFSETS,
           ("out", "dtype short view"))
    + rows("bbox_iou", ("dt", "dtype dim1 rank"), ("gt", "dtype dim1 rank"), ("iscrowd", "dtype dim0 rank"), *OFFSETS,
           ("out", "dtype short view"))
    + rows("coco_match", ("ious", "dtype"), ("dt_area", "dtype"), ("gt_area", "dtype"), ("gt_iscrowd", "dtype dim0"),
           ("area_ranges", "dtype dim1 rank"), ("thresholds", "dtype rank"), *OFFSETS,
           ("out.0", "dtype dim2 view", "dt_match"), ("out.1", "dtype dim2", "gt_match"), ("out.2", "dtype dim2", "dt_ignore"),
           ("out.3", "dtype dim1 view", "gt_ignore"))
    + rows("rle_from_poly", ("xy", "dtype dim1"), ("vert_off", "dtype rank"), ("vert_off", "dim0", "offsets"),
           ("heights", "dtype dim0 rank"), ("widths", "dtype dim0 rank"))
    + rows("rle_merge", *TABLE_ARGS, ("group_off", "dtype rank"))
    + rows("rle_from_string", ("bytes", "dtype rank"), ("str_off", "dtype rank"), *SIZES)
    + rows("rle_area_bbox", *TABLE_ARGS, *SIZES)
    + rows("rle_to_string", *TABLE_ARGS)
    + rows("rle_to_string_rows", *TABLE_ARGS)
    + rows("rle_decode", *TABLE_ARGS, ("out", "dtype dim2 view"))
    + rows("anchor_match", ("anchors", "dtype dim1 rank"), *GROUND_TRUTH, ("gt_class_ids", "dtype dim0 rank"))
    + rows("sample_by_key", ("match", "dtype rank"), ("keys", "dtype dim1 rank"), ("out", "dtype dim1 view"))
    + rows("rpn_deltas", ("anchors", "dtype dim1 rank"), *GROUND_TRUTH, ("match", "dtype dim1 rank"), ("iou_argmax", "dtype dim1 rank"))
    + rows("detection_targets", ("rois", "dtype dim2 rank"), ("gt_boxes", "dtype dim1 rank"), ("gt_class_ids", "dtype dim0 rank"),
           ("gt_off", "dtype dim0 rank"), ("keys", "dtype dim1 rank"), ("out.0", "dtype dim1 view", "rois_out"),
           ("out.5", "dtype dim0", "num_pos"))
    + rows("mask_targets", ("gt_masks", "dtype rank"), ("gt_off", "dtype dim0 rank"), ("rois_out", "dtype dim2 rank"),
           ("gt_index", "dtype dim1 rank"), ("num_pos", "dtype dim0 rank"), ("out", "dtype dim3 view", "target_mask"))
    + rows("rpn_loss", ("match", "dtype rank"), ("logits", "dtype dim2 rank"), ("pred_bbox", "dtype dim2 rank"),
           ("target_bbox", "dtype dim2 rank"))
    + rows("rpn_loss_backward", ("match", "dtype rank"), ("logits", "dtype dim2 rank"), ("pred_bbox", "dtype dim2 rank"),
           ("target_bbox", "dtype dim2 rank"), ("chunk_pos", "dtype dim1 rank"), ("counts", "dtype dim1"), ("grad_out", "dtype dim0"))
    + rows("head_loss", ("target_class_ids", "dtype rank"), ("num_rois", "dtype dim0 rank"), ("target_deltas", "dtype dim2 rank"),
           ("target_mask", "dtype dim1 rank"), ("logits", "dtype dim1 rank"), ("pred_bbox", "dtype dim3 rank"),
           ("pred_masks", "dtype dim4 rank"))
    + rows("head_loss_backward", ("target_class_ids", "dtype rank"), ("num_rois", "dtype dim0 rank"), ("target_deltas", "dtype dim2 rank"),
           ("target_mask", "dtype dim1 rank"), ("logits", "dtype dim1 rank"), ("pred_bbox", "dtype dim3 rank"),
           ("pred_masks", "dtype dim4 rank"), ("counts", "dtype dim1"), ("grad_out", "dtype dim0"))
    # one row per group of asserts that became a refusal on the inference side
    + rows("conv_bn_act", ("x", "dtype view rank"), ("w", "dtype rank"), ("scale", "dtype dim0"), ("shift", "dim0"),
           ("residual", "dtype dim3 view"), ("out", "dim3 view"))
    + rows("conv_bn_act_rows", ("row_counts", "dtype dim0"), op="conv_bn_act")
    + rows("conv_bn_act_f16mfma", ("x", "view"), ("w_hi", "dtype"), ("w_lo", "dtype dim0"), ("residual", "dim3 view"))
    + rows("conv_f16_pipelined", ("x", "dtype view"), ("w", "dtype"), ("residual", "dtype dim3"))
    + rows("pack_afrags_f16", ("w", "dtype"))
    + rows("maxpool", ("x", "view rank"))
    + rows("nchw_to_nhwc", ("x", "dtype view rank"))
    + rows("nhwc_to_nchw", ("x", "dtype view rank"))
    + rows("nhwc_to_kblocked", ("x", "dtype dim3 rank"))
    + rows("bottleneck_native", ("x", "dtype view rank"), ("w1", "dim3 dtype"), ("w2", "dim0 view"), ("w3", "dim3"), ("s1", "dtype"),
           ("t3", "dtype"))
    + rows("bottleneck_fused", ("x", "dtype view rank"), ("w1", "dim3"), ("u2", "dim0 view"), ("w3", "dim0"), ("s1", "dtype dim0"),
           ("t3", "dtype dim0"))
    + rows("bottleneck_c2_f16", ("x", "dtype view rank"))
    + rows("mask_tail_f16", ("x", "dtype view rank"), ("bias_de4", "dtype view"), ("bias_de4", "dim0", "biases"), ("bias5", "dtype view"))
    + rows("conv_f16_pipelined_heads", ("x", "dtype view"), ("w", "dtype dim0 dim3"), ("w_head32", "dtype dim0 view"))
    + rows("conv3x3_winograd_heads", ("x_kblocked", "dtype rank view"), ("u", "dim2 view"), ("w_head32", "dim0 dim1 view"))
    + rows("conv3x3_winograd4_heads", ("x_kblocked", "dtype rank"), ("u4", "dim0"), ("w_head32", "dim0 view"))
    + rows("stem_pool_f16", ("x", "dtype dim1 dim2"), ("w", "dtype dim3"))
    + rows("detection_decode", ("logits", "view"), ("bbox", "view"), ("rois", "view"), ("roi_counts", "dtype"), ("windows", "dtype view"))
    + rows("mold_images_u8", ("images", "dtype dim3 rank view"), ("out", "dtype dim0 dim1 view"))
    + rows("winograd_weights", ("w_ohwi", "dtype dim1 view"))
    + rows("winograd4_weights", ("w_ohwi", "dtype dim2 view"))
    + rows("conv3x3_winograd", ("x", "dtype view"), ("u", "dim2"))
    + rows("conv3x3_winograd4", ("x_kblocked", "dtype rank"), ("u4", "dim0"))
    + rows("conv3x3_winograd4_conv3", ("x_kblocked", "dtype rank"), ("u4", "dim3"), ("w3", "dim0"), ("residual", "dtype dim3"))
    + rows("stem_conv", ("x", "dtype dim3 view"), ("w", "dtype dim0"))
    + rows("stem_pool_f32", ("x", "dtype dim2 dim1"), ("w", "dtype dim3"))
    + rows("deconv2x2", ("x", "view"), ("w", "dim3"), ("bias4", "dim0"))
    + rows("topk_desc", ("scores", "dtype view rank"))
    + rows("proposal_decode", ("anchors", "view"), ("deltas", "dtype"), ("order", "dtype view"), ("top_scores", "view"))
    + rows("proposal_select", ("dets", "view"), ("keep", "dtype view"), ("keep_counts", "dtype"))
    + rows("detection_select", ("dets", "view"), ("nms_class_ids", "dtype view"), ("class_ids", "dtype view"), ("keep", "dtype view"),
           ("keep_counts", "dtype"))
    + rows("nms_batched", ("dets", "rank"), ("seg_counts", "dtype dim0"), ("class_ids", "dtype dim1"))
    + rows("nms_general", ("dets", "rank"))
    + rows("roi_align_pyramid", ("feature_maps.1", "dtype dim3 view", "feature_maps"), ("roi_counts", "dtype dim0"))
    + rows("rpn_scores_deltas", ("heads.2", "dtype dim3 view", "heads"))
    + rows("mold_image_u8", ("image", "dtype dim2 rank"), ("out", "dtype dim0 view"))
    + rows("paste_masks", ("masks", "dtype rank"), ("class_ids", "dim0"), ("boxes", "dim1"))
    + rows("blend_instances", ("image", "dtype dim2"), ("masks", "dtype dim2 rank"), ("colors", "dtype dim0 rank"),
           ("boxes", "dtype dim1 rank"), ("out", "dtype dim1"))
)


@pytest.mark.parametrize("name, op, arg, fault, names", ROWS)
def test_one_bad_argument_is_refused_before_any_launch(name, op, arg, fault, names):
    from maskrcnn_amd import ops
    fn, kwargs = case(name)
    kwargs = dict(kwargs)
    key, _, index = arg.partition(".")
    if index:
        entries = list(kwargs[key])
        entries[int(index)] = FAULTS[fault](entries[int(index)])
        kwargs[key] = type(kwargs[key])(entries)
    else:
        kwargs[key] = FAULTS[fault](kwargs[key])
    ops.CONV_PROFILE = []
    try:
        with pytest.raises(RuntimeError) as e:
            fn(**kwargs)
        launched = list(ops.CONV_PROFILE)
    finally:
        ops.CONV_PROFILE = None
    msg = str(e.value)
    assert msg.startswith(op + ": ") and names in msg, msg
    assert not isinstance(e.value, ops.MaskrcnnHipError), f"refused by the library, not by the binding: {msg}"
    assert launched == [], f"{len(launched)} launches were booked before the refusal"
