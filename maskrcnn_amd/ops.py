"""torch.ops.maskrcnn.* — thin bindings of the C ABI (include/maskrcnn_hip.h) for torch tensors.

Signatures mirror the reference's pybind module c++ext/maskrcnn/csrc/vision.cpp:11-15:
    nms(Tensor dets, float threshold) -> Tensor                                   (nms.h:15)
    crop_forward(image, boxes, box_index, extrapolation_value, crop_height, crop_width, crops) -> ()
                                                                                    (crop.h:14-22)
    crop_backward(grads, boxes, box_index, grads_image) -> ()                      (crop.h:36-41)
plus functional / batched forms used by the sync-free pipeline.

PyTorch is plumbing here: device memory, the current HIP stream, and the dispatcher. All arithmetic
happens in libmaskrcnn_hip.so. The three reference entry points also take CPU tensors, as the reference's dispatch
does (nms.h:15-30, crop.h:14-53: CPU in -> CPU out): they are staged host -> device, run the SAME HIP kernels and
come back as CPU tensors — there is no CPU arithmetic in this build, and without a visible GPU such a call raises
(the mirror of the reference's "Not compiled with GPU support", nms.h:24). The ops without a reference counterpart
(conv_bn_act, bottleneck_forward, the batched forms) take GPU tensors only.
"""
from __future__ import annotations

import ctypes
import functools
import math
import os
import weakref

import numpy as np
import torch

from ._lib import MaskrcnnHipError, c_f32, c_i32, c_vp, check, lib

__all__ = ["nms_batched", "nms_general", "crop", "roi_align_pyramid", "MaskrcnnHipError",
           "conv_bn_act", "conv_bn_act_f16mfma", "split_f16", "same_pad", "maxpool", "nchw_to_nhwc", "nhwc_to_nchw",
           "bottleneck_forward", "bottleneck_fused", "bottleneck_fused_supported", "bottleneck_native", "bottleneck_plan",
           "rpn_scores_deltas", "proposal_decode", "conv3x3_winograd_heads", "HeadSums",
           "detection_decode", "topk_desc", "proposal_select", "detection_select", "deconv2x2", "rpn_level_fused",
           "rle_encode", "rle_iou", "bbox_iou", "coco_match", "rle_from_poly", "rle_merge",
           "rle_from_string", "rle_area_bbox", "rle_to_string", "rle_decode", "blend_instances",
           "anchor_match", "sample_by_key", "rpn_deltas", "detection_targets", "mask_targets",
           "rpn_loss", "rpn_loss_backward", "head_loss", "head_loss_backward"]

_LIB = torch.library.Library("maskrcnn", "DEF")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


class HeadSums:
    """Output of conv3x3_winograd_heads for one pyramid level: the two k halves of the 1x1-head sums (without bias) in
    position-major pixel order, [2, rows, 32] fp32, for a [B, H, W] level. Consumed by rpn_scores_deltas."""

    def __init__(self, part: torch.Tensor, batch: int, height: int, width: int, tile_mode: int = 1):
        self.part, self.batch, self.height, self.width, self.tile_mode = part, batch, height, width, tile_mode

    def to_nhwc(self, bias: torch.Tensor) -> torch.Tensor:
        """[B,H,W,18] = (half 0 + half 1) + bias, in image order (tests / debugging; the pipeline never needs it)."""
        b, h, w = self.batch, self.height, self.width
        if self.tile_mode == 4:                                            # two planes in pixel order (conv_f16_pipelined_heads)
            return ((self.part[0, :, :18] + self.part[1, :, :18]) + bias).view(b, h, w, 18).contiguous()
        th, tw = h // 2, w // 2
        if self.tile_mode == 1:
            t = b * th * tw
            v = (self.part[0, :t * 4, :18] + self.part[1, :t * 4, :18]) + bias
            return v.view(b, th, tw, 2, 2, 18).permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, 18).contiguous()
        if self.tile_mode == 3:                                            # F(4x4): rows (b, tyb, txb, py4, px8, i4, j4)
            tyb, txb = -(-(h // 4) // 4), -(-(w // 4) // 8)
            v = self.part[:, :18] + bias
            v = v.view(b, tyb, txb, 4, 8, 4, 4, 18).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(b, tyb * 16, txb * 32, 18)
            return v[:, :h, :w].contiguous()
        tyb, txb = -(-th // 8), -(-tw // 8)
        v = (self.part[0, :, :18] + self.part[1, :, :18]) + bias          # rows: (b, tyb, txb, py, px, a, c)
        v = v.view(b, tyb, txb, 8, 8, 2, 2, 18).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(b, tyb * 16, txb * 16, 18)
        return v[:, :h, :w].contiguous()


def _tensors(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, HeadSums):
        yield obj.part
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            yield from _tensors(o)


def _on_device(fn):
    """Device guard for a binding: every GPU tensor argument must live on ONE device, and the call — output
    allocation, torch.cuda.current_stream() and the kernel launch — runs with that device current, whatever the
    caller's current device is (a launch on cuda:0's stream against cuda:1's pointers is a memory fault, or silent
    peer traffic over xGMI)."""
    @functools.wraps(fn)
    def guarded(*args, **kwargs):
        dev = None
        for t in _tensors(args + tuple(kwargs.values())):
            if t.is_cuda:
                if dev is None:
                    dev = t.device
                elif t.device != dev:
                    raise RuntimeError(f"maskrcnn_amd.{fn.__name__}: tensor arguments on different devices "
                                       f"({dev} and {t.device})")
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return guarded


def _staging_device() -> torch.device:
    """Where a CPU-tensor call of a reference entry point is computed: the current GPU. No GPU → the call fails loudly; there
    is no CPU kernel to fall back to."""
    if not torch.cuda.is_available():
        raise RuntimeError("maskrcnn_amd: Not compiled with CPU support — CPU tensors are staged to the GPU and run the HIP "
                           "kernels, and no GPU is visible")
    return torch.device("cuda", torch.cuda.current_device())


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("maskrcnn_amd: Not compiled with CPU support (tensor is on %s); "
                               "move tensors to the GPU" % t.device)


# --------------------------------------------------------------------------------------------------
# NMS
# --------------------------------------------------------------------------------------------------
@_on_device
def nms_batched(dets: torch.Tensor, threshold: float, seg_counts: torch.Tensor | None = None,
                class_ids: torch.Tensor | None = None, use_workspace: bool = True):
    """dets [S, N, 5] fp32 (any strides) → (keep int64 [S, N] ascending indices padded with -1,
    counts int32 [S]). No host synchronisation. use_workspace=False forces the single-launch LDS path."""
    _need_gpu(dets, seg_counts, class_ids)
    if dets.dtype != torch.float32:
        raise RuntimeError(f'"nms" GPU path implemented for Float only, got {dets.dtype}')
    assert dets.dim() == 3 and dets.size(2) >= 5
    s, n = dets.size(0), dets.size(1)
    keep = torch.empty(s, n, dtype=torch.int64, device=dets.device)
    counts = torch.empty(s, dtype=torch.int32, device=dets.device)
    if seg_counts is not None:
        assert seg_counts.dtype == torch.int32 and seg_counts.is_contiguous() and seg_counts.numel() == s
    if class_ids is not None:
        assert class_ids.dtype == torch.int32 and class_ids.is_contiguous() and class_ids.numel() == s * n
    ws, ws_bytes = None, 0
    if use_workspace and n > 128:
        ws_bytes = int(lib.mrcnn_nms_workspace_bytes(s, n))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dets.device)
    check(lib.mrcnn_nms_batched_f32(dets.data_ptr(), s, n, dets.stride(0), dets.stride(1),
                                    dets.stride(2), _ptr(seg_counts), _ptr(class_ids),
                                    float(threshold), keep.data_ptr(), counts.data_ptr(), _ptr(ws), ws_bytes,
                                    _stream()))
    return keep, counts


NMS_MAX_BOXES = int(lib.mrcnn_nms_max_boxes())   # per segment on the fp32 LDS / pair-mask paths (csrc/nms.hip)


@_on_device
def nms_general(dets: torch.Tensor, threshold: float):
    """dets [N, >=5] float32 or float64, any strides, any N → (keep int64 [N] ascending input indices padded with -1, count
    int64 [1]); arithmetic in dets' own type (cpu/nms_cpu.cpp:73-79). csrc/nms_general.hip; no host synchronisation."""
    _need_gpu(dets)
    if dets.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f'"nms" not implemented for {dets.dtype}')   # AT_DISPATCH_FLOATING_TYPES
    assert dets.dim() == 2 and dets.size(1) >= 5
    n = dets.size(0)
    dt = 0 if dets.dtype == torch.float32 else 1
    keep = torch.empty(n, dtype=torch.int64, device=dets.device)
    count = torch.empty(1, dtype=torch.int64, device=dets.device)
    nbytes = int(lib.mrcnn_nms_general_workspace_bytes(n, dt))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dets.device)
    check(lib.mrcnn_nms_general(dets.data_ptr(), dt, n, dets.stride(0), dets.stride(1), float(threshold), keep.data_ptr(),
                                count.data_ptr(), ws.data_ptr(), nbytes, _stream()))
    return keep, count


def _nms(dets: torch.Tensor, threshold: float) -> torch.Tensor:
    """Reference call shape: [N,5] → int64 [K] ascending input indices on dets.device; float32 or float64 boxes, any N
    (nms.h:15-30, cpu/nms_cpu.cpp:73-79). fp32 with N <= 16384 — everything model.py asks for — runs csrc/nms.hip, the
    rest csrc/nms_general.hip. (The data-dependent output length costs one D2H read; use nms_batched to stay async.)"""
    _need_gpu(dets)
    if dets.numel() == 0:  # nms.h:20-21
        return torch.empty(0, dtype=torch.int64, device=dets.device)
    if dets.dim() != 2 or dets.size(1) < 5:
        raise RuntimeError("nms: dets must be [N, 5]")
    if dets.dtype == torch.float32 and dets.size(0) <= NMS_MAX_BOXES:
        keep, counts = nms_batched(dets.unsqueeze(0), threshold)
        return keep[0, :int(counts.item())]
    keep, count = nms_general(dets, threshold)
    return keep[:int(count.item())]


_LIB.define("nms(Tensor dets, float threshold) -> Tensor")
_LIB.impl("nms", _nms, "CUDA")


def _nms_cpu(dets: torch.Tensor, threshold: float) -> torch.Tensor:
    """CPU tensor in → CPU int64 out (nms.h:26-29 → nms_cpu, cpu/nms_cpu.cpp:69: ascending input indices): H2D, the HIP kernel,
    D2H. float32 / float64 in their own arithmetic like the reference's AT_DISPATCH_FLOATING_TYPES (cpu/nms_cpu.cpp:73-79)."""
    dev = _staging_device()
    if dets.numel() == 0:   # nms_cpu.cpp:16-18
        return torch.empty(0, dtype=torch.int64)
    return _nms(dets.to(dev), threshold).cpu()


_LIB.impl("nms", _nms_cpu, "CPU")


# --------------------------------------------------------------------------------------------------
# crop_and_resize
# --------------------------------------------------------------------------------------------------
def _check_crop_inputs(image, boxes, box_index, gpu: bool = True):
    if gpu:
        _need_gpu(image, boxes, box_index)
    if image.dtype != torch.float32 or boxes.dtype != torch.float32:
        raise RuntimeError("crop: expected scalar type Float for image and boxes")
    if box_index.dtype != torch.int32:
        raise RuntimeError("crop: expected scalar type Int for box_index")
    if image.dim() != 4 or boxes.dim() != 2 or boxes.size(1) != 4 or box_index.numel() != boxes.size(0):
        raise RuntimeError("crop: image [B,C,H,W], boxes [N,4], box_index [N] expected")


@_on_device
def crop(image: torch.Tensor, boxes: torch.Tensor, box_index: torch.Tensor,
         extrapolation_value: float, crop_height: int, crop_width: int) -> torch.Tensor:
    """Functional form: returns a fresh [N, C, crop_height, crop_width] tensor."""
    _check_crop_inputs(image, boxes, box_index)
    crops = torch.empty(boxes.size(0), image.size(1), crop_height, crop_width, dtype=torch.float32, device=image.device)
    _crop_launch(image, boxes, box_index, extrapolation_value, crop_height, crop_width, crops)
    return crops


def _crop_launch(image, boxes, box_index, extrapolation_value, crop_height, crop_width, crops) -> None:
    """The one launch behind crop and crop_forward: checked inputs (any strides), crops contiguous [N,C,crop_height,crop_width]."""
    image, boxes, box_index = image.contiguous(), boxes.contiguous(), box_index.contiguous()
    b, c, h, w = image.shape
    check(lib.mrcnn_crop_forward_f32(image.data_ptr(), b, c, h, w, boxes.data_ptr(),
                                     box_index.data_ptr(), boxes.size(0), float(extrapolation_value),
                                     int(crop_height), int(crop_width), crops.data_ptr(), _stream()))


@_on_device
def _crop_forward(image, boxes, box_index, extrapolation_value, crop_height, crop_width, crops):
    """Out-param form of crop.h:14-22: `crops` is resized to [N,C,h,w] and overwritten
    (crop_cpu.cpp:141-143)."""
    _check_crop_inputs(image, boxes, box_index)
    _need_gpu(crops)
    if crops.dtype != torch.float32:
        raise RuntimeError("crop_forward: expected scalar type Float for crops")
    crops.resize_(boxes.size(0), image.size(1), crop_height, crop_width)
    _crop_launch(image, boxes, box_index, extrapolation_value, crop_height, crop_width, crops)


@_on_device
def _crop_backward(grads, boxes, box_index, grads_image):
    _need_gpu(grads, boxes, box_index, grads_image)
    if grads.dtype != torch.float32 or boxes.dtype != torch.float32 or grads_image.dtype != torch.float32:
        raise RuntimeError("crop_backward: expected scalar type Float")
    if box_index.dtype != torch.int32:
        raise RuntimeError("crop_backward: expected scalar type Int for box_index")
    if not grads_image.is_contiguous() or grads_image.dim() != 4:
        raise RuntimeError("crop_backward: grads_image must be a contiguous [B,C,H,W] tensor")
    grads, boxes, box_index = grads.contiguous(), boxes.contiguous(), box_index.contiguous()
    b, c, h, w = grads_image.shape
    n, gc, ch, cw = grads.shape
    if gc != c:
        raise RuntimeError("crop_backward: channel mismatch")
    check(lib.mrcnn_crop_backward_f32(grads.data_ptr(), boxes.data_ptr(), box_index.data_ptr(), n, b,
                                      c, h, w, ch, cw, grads_image.data_ptr(), _stream()))


_LIB.define("crop_forward(Tensor image, Tensor boxes, Tensor box_index, float extrapolation_value, "
            "int crop_height, int crop_width, Tensor(a!) crops) -> ()")
_LIB.impl("crop_forward", _crop_forward, "CUDA")


def _crop_forward_cpu(image, boxes, box_index, extrapolation_value, crop_height, crop_width, crops):
    """crop.h:24-33 with CPU tensors: staged through the GPU; `crops` (a CPU float tensor of any shape) is resized in place
    to [N,C,h,w] and overwritten, as crop_cpu.cpp:141-143 does. (A box_index outside [0, B) makes the reference exit(-1),
    crop_cpu.cpp:47-50; here that box's crop is extrapolation_value, as on the GPU path.)"""
    _check_crop_inputs(image, boxes, box_index, gpu=False)
    if crops.dtype != torch.float32:
        raise RuntimeError("crop_forward: expected scalar type Float for crops")
    dev = _staging_device()
    out = crop(image.to(dev), boxes.to(dev), box_index.to(dev), extrapolation_value, crop_height, crop_width)
    crops.resize_(out.shape)
    crops.copy_(out)


_LIB.impl("crop_forward", _crop_forward_cpu, "CPU")
_LIB.define("crop_backward(Tensor grads, Tensor boxes, Tensor box_index, Tensor(a!) grads_image) -> ()")
_LIB.impl("crop_backward", _crop_backward, "CUDA")


def _crop_backward_cpu(grads, boxes, box_index, grads_image):
    """crop.h:43-52 with CPU tensors: grads_image [B,C,H,W] is zeroed and accumulated on the GPU, then copied back in place."""
    dev = _staging_device()
    if not grads_image.is_contiguous() or grads_image.dim() != 4:
        raise RuntimeError("crop_backward: grads_image must be a contiguous [B,C,H,W] tensor")
    gi = torch.empty(grads_image.shape, dtype=grads_image.dtype, device=dev)
    _crop_backward(grads.to(dev), boxes.to(dev), box_index.to(dev), gi)
    grads_image.copy_(gi)


_LIB.impl("crop_backward", _crop_backward_cpu, "CPU")
_LIB.define("crop(Tensor image, Tensor boxes, Tensor box_index, float extrapolation_value, "
            "int crop_height, int crop_width) -> Tensor")
_LIB.impl("crop", crop, "CUDA")


def _crop_cpu(image, boxes, box_index, extrapolation_value, crop_height, crop_width):
    _check_crop_inputs(image, boxes, box_index, gpu=False)
    dev = _staging_device()
    return crop(image.to(dev), boxes.to(dev), box_index.to(dev), extrapolation_value, crop_height, crop_width).cpu()


_LIB.impl("crop", _crop_cpu, "CPU")


@_on_device
def roi_align_pyramid(feature_maps, rois: torch.Tensor, pool: int, image_area: float,
                      rois_per_image: int | None = None, roi_batch: torch.Tensor | None = None,
                      return_levels: bool = False, out_kblocked: bool = False, out_f16: bool = False,
                      roi_counts: torch.Tensor | None = None):
    """model.py:276-393 in one launch on channels-last maps.

    feature_maps: [P2,P3,P4,P5], each a contiguous fp32 [B, H_l, W_l, C] (NHWC) tensor.
    rois [R,4] normalised. Returns [R, pool, pool, C] (NHWC) in roi order (+ int32 levels); out_kblocked=True returns
    [C/8, R, pool, pool, 8] instead (the layout conv3x3_winograd reads: no layout pass before the mask head); out_f16=True
    returns the NHWC result rounded to fp16 (the "f16" mode's heads: what their first conv would round the values to).
    roi_counts int32 [images] (with rois_per_image): only the first roi_counts[i] slots of image i hold a RoI; the others are
    skipped and their rows of the output (and of `levels`) are left UNWRITTEN — unspecified values, possibly NaN bit patterns:
    hand such a tensor only to consumers that skip the same rows (conv_bn_act(row_counts=...))."""
    assert len(feature_maps) == 4
    _need_gpu(rois, roi_batch, *feature_maps)
    rois = rois.contiguous()
    b, _, _, c = feature_maps[0].shape
    for fm in feature_maps:
        assert fm.is_contiguous() and fm.dtype == torch.float32 and fm.size(0) == b and fm.size(3) == c
    r = rois.size(0)
    if out_kblocked:
        assert c % 8 == 0 and not out_f16
        out = torch.empty(c // 8, r, pool, pool, 8, dtype=torch.float32, device=rois.device)
    elif out_f16:
        out = torch.empty(r, pool, pool, c, dtype=torch.float16, device=rois.device)
    else:
        out = torch.empty(r, pool, pool, c, dtype=torch.float32, device=rois.device)
    levels = torch.empty(r, dtype=torch.int32, device=rois.device) if return_levels else None
    ptrs = (c_vp * 4)(*[fm.data_ptr() for fm in feature_maps])
    hs = (c_i32 * 4)(*[fm.size(1) for fm in feature_maps])
    ws = (c_i32 * 4)(*[fm.size(2) for fm in feature_maps])
    if roi_batch is not None:
        assert roi_batch.dtype == torch.int32 and roi_batch.is_contiguous()
    if roi_counts is not None:   # only the first roi_counts[image] slots of an image hold a RoI: the others are skipped
        assert roi_counts.dtype == torch.int32 and roi_counts.is_contiguous() and roi_batch is None and rois_per_image
        assert roi_counts.numel() * rois_per_image == r
    check(lib.mrcnn_roi_align_pyramid_counted_f32(ptrs, hs, ws, b, c, rois.data_ptr(), _ptr(roi_batch), r,
                                                  int(rois_per_image or 0), _ptr(roi_counts), int(pool), float(image_area),
                                                  out.data_ptr(), 1 if out_kblocked else 2 if out_f16 else 0, _ptr(levels),
                                                  _stream()))
    return (out, levels) if return_levels else out


# --------------------------------------------------------------------------------------------------
# conv + BN + ReLU (+ residual), channels-last
# --------------------------------------------------------------------------------------------------
# When set to a list, every conv launch appends (start_event, end_event, algorithmic_flops, (M, N, K),
# algorithmic_bytes = each operand/result tensor once, kernel tag) —
# HIP events recorded on the launch stream; used by bench.py's roofline pass, never in the timed region.
CONV_PROFILE: list | None = None


def _launch(fn, args, book) -> None:
    """check(fn(*args)) for an entry point whose launches the profiling pass times. While CONV_PROFILE is a list, HIP events
    go on the stream right before and right after the launch and the row (start, end, *book()) is appended; book() ->
    (algorithmic FLOPs, (M, N, K), algorithmic bytes, kernel tag[, executed FLOPs[, dict]]). book runs only then, and only after
    the end event is on the stream: it may synchronise (row_counts.tolist()) or call back into the library."""
    prof = CONV_PROFILE
    if prof is None:
        check(fn(*args))
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(fn(*args))
    e1.record()
    prof.append((e0, e1, *book()))


def _pad_out_hw(pad, h: int, w: int, kh: int, kw: int, stride: int = 1):
    """pad = (top, left, bottom, right) as ints, and the output height and width of a kh x kw window at this stride."""
    pt, pl, pb, pr = [int(v) for v in pad]
    return (pt, pl, pb, pr), (h + pt + pb - kh) // stride + 1, (w + pl + pr - kw) // stride + 1


@_on_device
def conv_bn_act(x: torch.Tensor, w: torch.Tensor, scale: torch.Tensor | None,
                shift: torch.Tensor | None, stride: int = 1, pad=(0, 0, 0, 0), relu: bool = False,
                residual: torch.Tensor | None = None, res_div: int = 1,
                out: torch.Tensor | None = None, algo_cin: int | None = None,
                out_kblocked: bool = False, row_counts: torch.Tensor | None = None,
                rows_per_group: int = 0) -> torch.Tensor:
    """y = act(scale * conv(x, w) + shift + residual).

    row_counts / rows_per_group: the output rows come in groups of rows_per_group RoI slots of which the first row_counts[g]
    are valid (int32 device tensor); 128-row tiles without a valid row are skipped and their output rows left untouched.

    out_kblocked: write y as [Cout/8,B,OH,OW,8] (what conv3x3_winograd reads) instead of NHWC.

    relu: False/0 none, True/1 ReLU, 2 sigmoid.
    x [B,H,W,Cin] NHWC fp32 contiguous; w [Cout,KH,KW,Cin] (OHWI) contiguous; scale/shift [Cout] or
    None; pad = (top, left, bottom, right) zero padding applied on the fly; residual [B,OH/res_div,
    OW/res_div,Cout] (or the same tensor k-blocked, 5-d). Returns y [B,OH,OW,Cout] NHWC."""
    _need_gpu(x, w, scale, shift, residual)
    assert x.dtype == torch.float32 and w.dtype == torch.float32
    assert x.is_contiguous() and w.is_contiguous() and x.dim() == 4 and w.dim() == 4
    b, h, wd, cin = x.shape
    cout, kh, kw, wcin = w.shape
    if wcin != cin:
        raise RuntimeError(f"conv_bn_act: weight Cin {wcin} != input Cin {cin}")
    (pt, pl, pb, pr), oh, ow = _pad_out_hw(pad, h, wd, kh, kw, stride)
    if out_kblocked:
        assert out is None and cout % 8 == 0
        out = torch.empty(cout // 8, b, oh, ow, 8, dtype=torch.float32, device=x.device)
    elif out is None:
        out = torch.empty(b, oh, ow, cout, dtype=torch.float32, device=x.device)
    else:
        assert out.is_contiguous() and tuple(out.shape) == (b, oh, ow, cout)
    for t in (scale, shift):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == cout)
    res_kblocked = residual is not None and residual.dim() == 5
    if residual is not None:
        assert residual.is_contiguous() and residual.dtype == torch.float32
        want = (cout // 8, b, oh // res_div, ow // res_div, 8) if res_kblocked else (b, oh // res_div, ow // res_div, cout)
        assert tuple(residual.shape) == want, \
            f"residual {tuple(residual.shape)} vs output {(b, oh, ow, cout)} / {res_div}"
    if row_counts is not None:
        assert residual is None and not out_kblocked and row_counts.dtype == torch.int32 and row_counts.is_contiguous()
        assert rows_per_group >= 1 and row_counts.numel() * rows_per_group == b * oh * ow

        def book_rows():
            # Book what RAN: the kernel returns early for M tiles without a valid row (conv.hip), so the MFMA work is the
            # executed tiles' rows and the problem the reference poses is the valid rows only (model.py:1366-1374). The host
            # read of row_counts synchronises — profiling pass only, after the end event is on the stream.
            m, k = b * oh * ow, kh * kw * (algo_cin or cin)
            bm = int(lib.mrcnn_conv_rows_tile_m(cout))
            rows_exec, rows_valid = rows_executed(row_counts.tolist(), int(rows_per_group), m, bm)
            kk = kh * kw * cin
            nbytes = 4 * (rows_exec * (kk + cout) + w.numel())
            return (2.0 * rows_valid * k * cout, (rows_valid, cout, k), nbytes, "direct", 2.0 * rows_exec * k * cout,
                    {"rows_slots": m, "rows_executed": rows_exec, "rows_valid": rows_valid})
        _launch(lib.mrcnn_conv_bn_act_rows_f32,
                (x.data_ptr(), b, h, wd, cin, w.data_ptr(), cout, kh, kw, int(stride), pt, pl, pb, pr, _ptr(scale), _ptr(shift),
                 int(relu), out.data_ptr(), row_counts.data_ptr(), int(rows_per_group), _stream()), book_rows)
        return out

    def book():
        m, k = b * oh * ow, kh * kw * (algo_cin or cin)  # algorithmic: 2*MACs of the un-padded conv
        nbytes = 4 * (x.numel() + w.numel() + out.numel() + (residual.numel() if residual is not None else 0))
        return 2.0 * m * k * cout, (m, cout, k), nbytes, "direct"
    _launch(lib.mrcnn_conv_bn_act_f32,
            (x.data_ptr(), b, h, wd, cin, w.data_ptr(), cout, kh, kw, int(stride), pt, pl, pb, pr, _ptr(scale), _ptr(shift),
             _ptr(residual), int(res_div), 1 if res_kblocked else 0, int(relu), out.data_ptr(), 1 if out_kblocked else 0,
             _stream()), book)
    return out


def rows_executed(counts, rows_per_group: int, m: int, bm: int):
    """Host restatement of conv_common.hpp::tile_has_rows for the profiling pass: output rows come in groups of rows_per_group
    slots of which the first counts[g] are valid; an M tile [t*bm, (t+1)*bm) runs iff it holds a valid row. → (rows of the
    tiles that run — what the MFMA pipe computes, capped at m —, valid rows — the problem the reference poses)."""
    assert rows_per_group >= 1 and len(counts) * rows_per_group == m and bm >= 1
    rows = 0
    for t in range(-(-m // bm)):
        m0, last = t * bm, min((t + 1) * bm, m) - 1
        g0, g1 = m0 // rows_per_group, last // rows_per_group
        live = (m0 - g0 * rows_per_group) < counts[g0] or any(counts[g] > 0 for g in range(g0 + 1, g1 + 1))
        if live:
            rows += last + 1 - m0
    return rows, int(sum(min(max(int(c), 0), rows_per_group) for c in counts))


def split_f16(w: torch.Tensor):
    """fp32 → (hi, lo) fp16 planes: hi = fp16(w), lo = fp16(w - fp32(hi)); hi + lo carries 22 mantissa bits."""
    hi = w.to(torch.float16)
    lo = (w - hi.to(torch.float32)).to(torch.float16)
    return hi.contiguous(), lo.contiguous()


@_on_device
def conv_bn_act_f16mfma(x: torch.Tensor, w_hi: torch.Tensor, w_lo: torch.Tensor | None,
                        scale: torch.Tensor | None, shift: torch.Tensor | None, stride: int = 1,
                        pad=(0, 0, 0, 0), relu: bool = False, residual: torch.Tensor | None = None,
                        res_div: int = 1, products: int = 3, algo_cin: int | None = None,
                        out_f16: bool = False) -> torch.Tensor:
    """conv_bn_act on fp16-operand MFMA. w_hi/w_lo fp16 OHWI planes (split_f16).
    products = 3: error-compensated split (fp32-grade accuracy); x / residual / y fp32 NHWC.
    products = 1: plain fp16 operands; x may be fp32 or fp16 NHWC, y is fp16 when out_f16 (the residual has y's type):
    the fp16-activation form of BASELINE config 5's "fp16 MFMA path"."""
    _need_gpu(x, w_hi, w_lo, scale, shift, residual)
    x_f16 = x.dtype == torch.float16
    assert (x_f16 or x.dtype == torch.float32) and w_hi.dtype == torch.float16 and x.is_contiguous() and w_hi.is_contiguous()
    assert w_lo is None or (w_lo.dtype == torch.float16 and w_lo.is_contiguous() and w_lo.shape == w_hi.shape)
    b, h, wd, cin = x.shape
    cout, kh, kw, wcin = w_hi.shape
    if wcin != cin:
        raise RuntimeError(f"conv_bn_act_f16mfma: weight Cin {wcin} != input Cin {cin}")
    (pt, pl, pb, pr), oh, ow = _pad_out_hw(pad, h, wd, kh, kw, stride)
    io16 = x_f16 or out_f16
    if io16 and products != 1:
        raise RuntimeError("conv_bn_act_f16mfma: fp16 activations belong to the plain-fp16 mode (products = 1)")
    out = torch.empty(b, oh, ow, cout, dtype=torch.float16 if out_f16 else torch.float32, device=x.device)
    if residual is not None:
        assert residual.is_contiguous() and tuple(residual.shape) == (b, oh // res_div, ow // res_div, cout)
        assert residual.dtype == out.dtype, "the residual has the output's storage type"

    def book():
        m, k = b * oh * ow, kh * kw * (algo_cin or cin)
        nbytes = x.numel() * x.element_size() + out.numel() * out.element_size() + \
            (residual.numel() * residual.element_size() if residual is not None else 0) + \
            2 * w_hi.numel() * (2 if products == 3 else 1)
        return 2.0 * m * k * cout, (m, cout, k), nbytes, "f16"
    if io16:
        _launch(lib.mrcnn_conv_bn_act_nhwc_f16io,
                (x.data_ptr(), 1 if x_f16 else 0, b, h, wd, cin, w_hi.data_ptr(), cout, kh, kw, int(stride), pt, pl, pb, pr,
                 _ptr(scale), _ptr(shift), _ptr(residual), int(res_div), int(relu), out.data_ptr(), 1 if out_f16 else 0,
                 _stream()), book)
    else:
        _launch(lib.mrcnn_conv_bn_act_nhwc_f16mfma,
                (x.data_ptr(), b, h, wd, cin, w_hi.data_ptr(), _ptr(w_lo), cout, kh, kw, int(stride), pt, pl, pb, pr,
                 _ptr(scale), _ptr(shift), _ptr(residual), int(res_div), int(relu), int(products), out.data_ptr(), _stream()),
                book)
    return out


def conv_f16_pipelined_supported(b: int, h: int, w: int, cin: int, cout: int, kh: int, kw: int, pad=(0, 0, 0, 0),
                                 stride: int = 1) -> bool:
    """Shape gate of conv_f16_pipelined (Cin % 64 == 0, Cout % 64 == 0, <= 25 taps, 32-bit byte offsets)."""
    pt, pl, pb, pr = [int(v) for v in pad]
    return bool(lib.mrcnn_conv_f16_pipelined_supported(int(b), int(h), int(w), int(cin), int(cout), int(kh), int(kw),
                                                       int(stride), pt, pl, pb, pr))


@_on_device
def conv_f16_pipelined(x: torch.Tensor, w: torch.Tensor, scale: torch.Tensor | None, shift: torch.Tensor | None,
                       pad=(0, 0, 0, 0), relu: bool = False, residual: torch.Tensor | None = None,
                       out_f16: bool = True, out_f32: bool = False, tile_rows: int = 0, algo_cin: int | None = None,
                       stride: int = 1, res_div: int = 1, tile_cols: int = 0):
    """The pipelined plain-fp16 conv (csrc/conv_f16p.hip): x fp16 NHWC, w fp16 OHWI, fp16 residual of the output's size
    (res_div 1) or half of it (res_div 2). Returns the fp16 output, the fp32 output, or the pair (fp16, fp32)."""
    _need_gpu(x, w, scale, shift, residual)
    assert x.dtype == torch.float16 and w.dtype == torch.float16 and x.is_contiguous() and w.is_contiguous()
    assert out_f16 or out_f32
    b, h, wd, cin = x.shape
    cout, kh, kw, wcin = w.shape
    if wcin != cin:
        raise RuntimeError(f"conv_f16_pipelined: weight Cin {wcin} != input Cin {cin}")
    (pt, pl, pb, pr), oh, ow = _pad_out_hw(pad, h, wd, kh, kw, stride)
    y16 = torch.empty(b, oh, ow, cout, dtype=torch.float16, device=x.device) if out_f16 else None
    y32 = torch.empty(b, oh, ow, cout, dtype=torch.float32, device=x.device) if out_f32 else None
    if residual is not None:
        assert residual.dtype == torch.float16 and residual.is_contiguous()
        assert tuple(residual.shape) == (b, oh // res_div, ow // res_div, cout)

    def book():
        m, k = b * oh * ow, kh * kw * (algo_cin or cin)
        nbytes = x.numel() * 2 + (y16.numel() * 2 if out_f16 else 0) + (y32.numel() * 4 if out_f32 else 0) + \
            (residual.numel() * 2 if residual is not None else 0) + 2 * w.numel()
        return 2.0 * m * k * cout, (m, cout, k), nbytes, "f16p"
    _launch(lib.mrcnn_conv_f16_pipelined,
            (x.data_ptr(), b, h, wd, cin, w.data_ptr(), cout, kh, kw, int(stride), pt, pl, pb, pr, _ptr(scale), _ptr(shift),
             _ptr(residual), int(res_div), int(relu), _ptr(y16), _ptr(y32), int(tile_rows), int(tile_cols), _stream()), book)
    if out_f16 and out_f32:
        return y16, y32
    return y16 if out_f16 else y32


def pack_afrags_f16(w: torch.Tensor) -> torch.Tensor:
    """fp16 weights [Cout, ...] (OHWI, flattened to [Cout][K], Cout % 32 == 0, K % 32 == 0) -> the A fragments
    csrc/bottleneck_f16.hip reads: [K/32][Cout/16][64 lanes][8]."""
    _need_gpu(w)
    assert w.dtype == torch.float16 and w.is_contiguous()
    cout, k = w.size(0), w.numel() // w.size(0)
    out = torch.empty(k // 32, cout // 16, 64, 8, dtype=torch.float16, device=w.device)
    with torch.cuda.device(w.device):
        check(lib.mrcnn_pack_afrags_f16(w.data_ptr(), cout, k, out.data_ptr(), _stream()))
    return out


def bottleneck_c2_f16_supported(b: int, h: int, w: int, cin: int, planes: int, has_downsample: bool) -> bool:
    """Shape gate of bottleneck_c2_f16 (planes 64, stride 1, Cin 256 identity / 64 with the downsample branch)."""
    return bool(lib.mrcnn_bottleneck_c2_f16_supported(int(b), int(h), int(w), int(cin), int(planes), int(bool(has_downsample))))


@_on_device
def bottleneck_c2_f16(x: torch.Tensor, w1f, s1, t1, w2f, s2, t2, w3f, s3, t3, wdf=None, sd=None, td=None) -> torch.Tensor:
    """Bottleneck.forward (model.py:190-211) of a ResNet C2 block in ONE launch, plain-fp16 path (csrc/bottleneck_f16.hip):
    x fp16 NHWC [B,H,W,256] (identity block) or [B,H,W,64] (the stage's first block: wdf / sd / td = its downsample branch);
    w*f: pack_afrags_f16 of the fp16 OHWI weights; s* / t*: folded BN (fp32). → fp16 NHWC [B,H,W,256]."""
    _need_gpu(x, w1f, w2f, w3f, wdf, s1, t1, s2, t2, s3, t3, sd, td)
    assert x.dtype == torch.float16 and x.is_contiguous() and x.dim() == 4
    b, h, w, cin = x.shape
    if w1f.numel() != 64 * cin or w2f.numel() != 64 * 576 or w3f.numel() != 256 * 64 or (wdf is not None and wdf.numel() != 256 * 64):
        raise RuntimeError("bottleneck_c2_f16: weight fragments do not belong to a planes-64 block of this Cin")
    for v, n in ((s1, 64), (t1, 64), (s2, 64), (t2, 64), (s3, 256), (t3, 256), (sd, 256), (td, 256)):
        if v is not None and not (v.dtype == torch.float32 and v.numel() == n and v.is_contiguous()):
            raise RuntimeError("bottleneck_c2_f16: scale / shift vectors must be contiguous fp32 of the layer's Cout")
    y = torch.empty(b, h, w, 256, dtype=torch.float16, device=x.device)

    def book():
        m = b * h * w
        kk = cin * 64 + 576 * 64 + 64 * 256 + (cin * 256 if wdf is not None else 0)       # multiply-adds per pixel
        nbytes = x.numel() * 2 + y.numel() * 2 + 2 * kk
        # the reference's layers inside this launch, each as the per-layer path books it (FLOPs, bytes: input + output (+ residual)
        # + weights) — bench.py prices a fused launch against ITS bytes and, beside that, against the layers' own floors
        layers = [(2.0 * m * cin * 64, 2 * (m * cin + m * 64 + cin * 64)), (2.0 * m * 576 * 64, 2 * (2 * m * 64 + 576 * 64)),
                  (2.0 * m * 64 * 256, 2 * (m * 64 + 2 * m * 256 + 64 * 256))]
        if wdf is not None:
            layers.append((2.0 * m * cin * 256, 2 * (m * cin + m * 256 + cin * 256)))
        return 2.0 * m * kk, (m, 256, kk // 256), nbytes, "f16blk", 2.0 * m * kk, {"layers": layers}
    _launch(lib.mrcnn_bottleneck_c2_f16,
            (x.data_ptr(), b, h, w, cin, w1f.data_ptr(), _ptr(s1), _ptr(t1), w2f.data_ptr(), _ptr(s2), _ptr(t2), w3f.data_ptr(),
             _ptr(s3), _ptr(t3), _ptr(wdf), _ptr(sd), _ptr(td), y.data_ptr(), _stream()), book)
    return y


def mask_tail_f16_supported(rois: int, h: int, w: int, cin: int, cout_deconv: int, classes: int) -> bool:
    """Shape gate of mask_tail_f16 (Cin 256, deconv Cout 256, classes <= 96, 32-bit byte offsets)."""
    return bool(lib.mrcnn_mask_tail_f16_supported(int(rois), int(h), int(w), int(cin), int(cout_deconv), int(classes)))


@_on_device
def mask_tail_f16(x: torch.Tensor, wde_frags: torch.Tensor, bias_de4: torch.Tensor, w5_frags: torch.Tensor, bias5: torch.Tensor) -> torch.Tensor:
    """The tail of Mask.forward (model.py:906-914) in ONE launch, plain-fp16 path (csrc/mask_tail_f16.hip): deconv 2x2 stride 2
    + bias + ReLU (fp16, in registers) -> conv5 1x1 + bias -> sigmoid. x fp16 NHWC [R,h,w,256]; wde_frags: pack_afrags_f16 of the
    deconv's GEMM weight [4*256,1,1,256]; w5_frags: pack_afrags_f16 of conv5's weight zero-padded to 96 rows; → fp32 [R,2h,2w,classes]."""
    _need_gpu(x, wde_frags, bias_de4, w5_frags, bias5)
    assert x.dtype == torch.float16 and x.is_contiguous() and x.dim() == 4
    r, h, w, cin = x.shape
    classes = bias5.numel()
    if wde_frags.numel() != 1024 * cin or w5_frags.numel() != 96 * cin or bias_de4.numel() != 1024:
        raise RuntimeError("mask_tail_f16: weight fragments / biases do not belong to a 256 -> 256 deconv and a <= 96-class conv5")
    assert bias_de4.dtype == torch.float32 and bias5.dtype == torch.float32 and bias_de4.is_contiguous() and bias5.is_contiguous()
    y = torch.empty(r, 2 * h, 2 * w, classes, dtype=torch.float32, device=x.device)

    def book():
        m = r * h * w
        kk = cin * 1024 + 4 * 256 * classes                                   # multiply-adds per input pixel
        layers = [(2.0 * m * cin * 1024, 2 * (m * cin + m * 1024 + cin * 1024)),          # deconv as the per-layer path books it
                  (2.0 * m * 4 * 256 * classes, 2 * m * 1024 + 4 * m * 4 * classes + 2 * 256 * classes)]
        return (2.0 * m * kk, (m, 4 * classes, kk // (4 * classes)), x.numel() * 2 + y.numel() * 4 + 2 * (1024 + 96) * cin,
                "f16tail", 2.0 * m * kk, {"layers": layers})
    _launch(lib.mrcnn_mask_tail_f16,
            (x.data_ptr(), r, h, w, cin, wde_frags.data_ptr(), bias_de4.data_ptr(), 256, w5_frags.data_ptr(), bias5.data_ptr(),
             classes, y.data_ptr(), _stream()), book)
    return y


@_on_device
def conv_f16_pipelined_heads(x: torch.Tensor, w: torch.Tensor, scale, shift, w_head32: torch.Tensor, pad=(1, 1, 1, 1),
                             relu: bool = True, tile_rows: int = 0, algo_cin: int | None = None) -> HeadSums:
    """RPN conv_shared + both 1x1 heads in one launch on the pipelined fp16 kernel ("f16" mode; model.py:605-607,624-641):
    x fp16 NHWC, w fp16 OHWI with Cout = 512, w_head32 fp16 [32, 512] (rows 0-17: conv_class then conv_bbox). → HeadSums
    (form 4: two planes in pixel order, without the bias)."""
    _need_gpu(x, w, scale, shift, w_head32)
    assert x.dtype == torch.float16 and w.dtype == torch.float16 and x.is_contiguous() and w.is_contiguous()
    b, h, wd, cin = x.shape
    cout, kh, kw, wcin = w.shape
    assert wcin == cin and cout == 512, "the consumer (rpn_scores_deltas form 4) adds exactly two 256-channel planes"
    assert w_head32.dtype == torch.float16 and w_head32.is_contiguous() and tuple(w_head32.shape) == (32, cout)
    (pt, pl, pb, pr), oh, ow = _pad_out_hw(pad, h, wd, kh, kw)
    part = torch.empty(cout // 256, b * oh * ow, 32, dtype=torch.float32, device=x.device)

    def book():
        m, k = b * oh * ow, kh * kw * (algo_cin or cin)
        return 2.0 * m * cout * (k + 18), (m, cout, k), x.numel() * 2 + part.numel() * 4 + 2 * w.numel(), "f16p"
    _launch(lib.mrcnn_conv_f16_pipelined_heads,
            (x.data_ptr(), b, h, wd, cin, w.data_ptr(), cout, kh, kw, pt, pl, pb, pr, _ptr(scale), _ptr(shift),
             1 if relu else 0, w_head32.data_ptr(), part.data_ptr(), int(tile_rows), _stream()), book)
    return HeadSums(part, b, oh, ow, 4)


def _conv_bn_act_op(x, w, scale, shift, stride, pad, relu, residual, res_div):
    return conv_bn_act(x, w, scale, shift, stride, pad, relu, residual, res_div)


_LIB.define("conv_bn_act(Tensor x, Tensor w, Tensor? scale, Tensor? shift, int stride, int[] pad, "
            "bool relu, Tensor? residual, int res_div) -> Tensor")
_LIB.impl("conv_bn_act", _conv_bn_act_op, "CUDA")
_LIB.impl("conv_bn_act", lambda x, *a: _need_gpu(x), "CPU")


def same_pad(size_a: int, size_b: int, kernel: int, stride: int):
    """SamePad2d (model.py:64-87) as (top, left, bottom, right) for a [.., size_a, size_b] (H, W) input.
    The reference computes the LAST-dim pad from size(2) and vice versa (its width/height names are
    swapped); reproduced as written — it only matters when H and W need different pad amounts."""
    out_a = math.ceil(float(size_a) / float(stride))
    out_b = math.ceil(float(size_b) / float(stride))
    pad_a = max((out_a - 1) * stride + kernel - size_a, 0)
    pad_b = max((out_b - 1) * stride + kernel - size_b, 0)
    a_lo, b_lo = pad_a // 2, pad_b // 2
    # F.pad(input, (a_lo, a_hi, b_lo, b_hi)): first pair → last dim (W), second pair → H
    return (b_lo, a_lo, pad_b - b_lo, pad_a - a_lo)


@_on_device
def maxpool(x: torch.Tensor, kernel: int, stride: int, pad=(0, 0, 0, 0), out_kblocked: bool = False) -> torch.Tensor:
    """Zero-padded max-pool on NHWC fp32 (stem pool: kernel 3, stride 2, pad = same_pad(H, W, 3, 2);
    P6: kernel 1, stride 2). out_kblocked=True writes [C/8,B,OH,OW,8] (P6 for the RPN's Winograd conv)."""
    _need_gpu(x)
    assert x.is_contiguous() and x.dtype in (torch.float32, torch.float16) and x.dim() == 4
    b, h, w, c = x.shape
    (pt, pl, pb, pr), oh, ow = _pad_out_hw(pad, h, w, kernel, kernel, stride)
    if x.dtype == torch.float16:
        assert not out_kblocked
        y = torch.empty(b, oh, ow, c, dtype=torch.float16, device=x.device)
        check(lib.mrcnn_maxpool_nhwc_f16(x.data_ptr(), b, h, w, c, int(kernel), int(stride), pt, pl, pb, pr, y.data_ptr(),
                                         _stream()))
        return y
    if out_kblocked:
        assert c % 8 == 0
        y = torch.empty(c // 8, b, oh, ow, 8, dtype=torch.float32, device=x.device)
    else:
        y = torch.empty(b, oh, ow, c, dtype=torch.float32, device=x.device)
    check(lib.mrcnn_maxpool_f32(x.data_ptr(), b, h, w, c, int(kernel), int(stride), pt, pl, pb, pr, y.data_ptr(),
                                1 if out_kblocked else 0, _stream()))
    return y


@_on_device
def nchw_to_nhwc(x: torch.Tensor, channels_padded: int | None = None) -> torch.Tensor:
    _need_gpu(x)
    assert x.is_contiguous() and x.dtype == torch.float32 and x.dim() == 4
    b, c, h, w = x.shape
    cp = int(channels_padded or c)
    y = torch.empty(b, h, w, cp, dtype=torch.float32, device=x.device)
    check(lib.mrcnn_nchw_to_nhwc_f32(x.data_ptr(), b, c, h, w, cp, y.data_ptr(), _stream()))
    return y


@_on_device
def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    _need_gpu(x)
    assert x.is_contiguous() and x.dtype == torch.float32 and x.dim() == 4
    b, h, w, c = x.shape
    y = torch.empty(b, c, h, w, dtype=torch.float32, device=x.device)
    check(lib.mrcnn_nhwc_to_nchw_f32(x.data_ptr(), b, c, h, w, y.data_ptr(), _stream()))
    return y


def bottleneck_fused_supported(h: int, w: int, cin: int, planes: int) -> bool:
    """Shapes the whole-block kernel covers: stride-1 identity blocks with planes = 64, Cin = 256, H and W % 16 == 0."""
    return bool(lib.mrcnn_bottleneck_fused_supported(int(h), int(w), int(cin), int(planes)))


@_on_device
def bottleneck_fused(x, w1, s1, t1, u2, s2, t2, w3, s3, t3) -> torch.Tensor:
    """Bottleneck.forward (model.py:190-211) of a stride-1 identity block in ONE launch (csrc/bottleneck.hip): both
    planes-channel intermediates stay in LDS. x [B,H,W,Cin] NHWC; w1 [P,1,1,Cin]; u2 = winograd_weights(conv2 weight
    [P,3,3,P]); w3 [4P,1,1,P]; (s, t) the folded BN/bias affine of each conv. Returns [B,H,W,4P]. Equals the
    three-launch path bit for bit."""
    _need_gpu(x, w1, s1, t1, u2, s2, t2, w3, s3, t3)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
    b, h, w, cin = x.shape
    planes = w1.size(0)
    assert w1.is_contiguous() and w1.numel() == planes * cin and w3.is_contiguous() and w3.numel() == 4 * planes * planes
    assert u2.is_contiguous() and u2.numel() == 16 * planes * planes
    for t, n in ((s1, planes), (t1, planes), (s2, planes), (t2, planes), (s3, 4 * planes), (t3, 4 * planes)):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n)
    y = torch.empty(b, h, w, 4 * planes, dtype=torch.float32, device=x.device)

    def book():
        m = b * h * w
        algo = 2.0 * m * (cin * planes + 9 * planes * planes + planes * 4 * planes)
        # what the MFMA pipe executes: conv1 on 352 GEMM rows per 256 output pixels (halo + row-tile padding),
        # conv2 as Winograd (1/2.25), conv3 as is
        executed = 2.0 * m * (cin * planes * 352.0 / 256.0 + 9 * planes * planes / 2.25 + planes * 4 * planes)
        return (algo, (m, 4 * planes, cin + 9 * planes + planes),
                4.0 * (2 * x.numel() + y.numel() + w1.numel() + u2.numel() + w3.numel()), "bottleneck", executed)
    _launch(lib.mrcnn_bottleneck_fused_f32,
            (x.data_ptr(), b, h, w, cin, w1.data_ptr(), _ptr(s1), _ptr(t1), u2.data_ptr(), _ptr(s2), _ptr(t2), w3.data_ptr(),
             _ptr(s3), _ptr(t3), planes, y.data_ptr(), _stream()), book)
    return y


# torch.ops.maskrcnn.bottleneck_forward sends eligible blocks to the whole-block kernel (whose conv2 is Winograd F(2x2)) only
# when BOTH switches say so — MRCNN_FUSED_BOTTLENECK=1 and Winograd not disabled (MRCNN_WINOGRAD=0 promises "every conv on the
# direct kernel, bitwise an fmaf chain"); otherwise the op is the exact three/four-launch composite. modules.py keeps this in
# step with its own flags.
BOTTLENECK_OP_FUSED = (os.environ.get("MRCNN_TUNING") == "1" and os.environ.get("MRCNN_FUSED_BOTTLENECK", "0") == "1"
                       and os.environ.get("MRCNN_WINOGRAD", "1") != "0")
_TRANSFORM_CACHE: dict = {}   # transform -> {data_ptr: (weakref to the conv2 weight tensor, its version, its Winograd transform)}


def _cached_transform(transform, w2: torch.Tensor) -> torch.Tensor:
    """transform(w2) — winograd_weights (F(2x2)) or winograd4_weights (F(4x4)) of a conv2 weight — computed once per weight
    tensor, not per call. An entry is valid only for the SAME tensor object at the same version: an address alone is reused by
    the allocator for other weights."""
    cache = _TRANSFORM_CACHE.setdefault(transform, {})
    e = cache.get(w2.data_ptr())
    if e is not None and e[0]() is w2 and e[1] == w2._version:
        return e[2]
    if len(cache) > 256:
        cache.clear()
    u = transform(w2)
    cache[w2.data_ptr()] = (weakref.ref(w2), w2._version, u)
    return u


def bottleneck_plan(batch, h, w, cin, planes, stride, have_u2, have_u4, min_tiles4, fuse_conv3) -> int:
    """Bits of the plan mrcnn_bottleneck_forward_f32 follows: 1 = conv2 on F(4x4), 2 = conv2 on F(2x2), 4 = conv2 + conv3 fused."""
    return int(lib.mrcnn_bottleneck_plan(batch, h, w, cin, planes, int(stride), int(bool(have_u2)), int(bool(have_u4)),
                                         int(min_tiles4), int(bool(fuse_conv3))))


@_on_device
def bottleneck_native(x, w1, s1, t1, w2, u2, u4, s2, t2, w3, s3, t3, wd, sd, td, stride: int, min_tiles4: int = 8,
                      fuse_conv3: bool = True) -> torch.Tensor:
    """Bottleneck.forward (model.py:190-211) as ONE call of the C ABI (mrcnn_bottleneck_forward_f32, csrc/bottleneck_op.hip):
    the library plans the block — conv1 (+ downsample), then conv2 + conv3 + residual in one launch for ResNet C2, or conv2
    (F(4x4) / F(2x2) Winograd when u4 / u2 are given, else the exact direct kernel) and conv3 + residual — and enqueues the
    launches on the current stream. x [B,H,W,Cin] NHWC fp32; w* OHWI; u2 / u4 = winograd_weights / winograd4_weights of w2 or
    None. While ops.CONV_PROFILE is collecting per-launch events, the same plan runs launch by launch from Python
    (identical launches, identical result) so that every launch can be timed."""
    _need_gpu(x, w1, s1, t1, w2, u2, u4, s2, t2, w3, s3, t3, wd, sd, td)
    assert x.dim() == 4 and x.is_contiguous() and x.dtype == torch.float32
    b, h, w, cin = x.shape
    planes, stride = w1.size(0), int(stride)
    assert tuple(w1.shape) == (planes, 1, 1, cin) and tuple(w2.shape) == (planes, 3, 3, planes)
    assert tuple(w3.shape) == (4 * planes, 1, 1, planes) and (wd is None or tuple(wd.shape) == (4 * planes, 1, 1, cin))
    for t in (w1, w2, w3, wd, u2, u4, s1, t1, s2, t2, s3, t3, sd, td):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32)
    if CONV_PROFILE is not None:
        return _bottleneck_launch_by_launch(x, w1, s1, t1, w2, u2, u4, s2, t2, w3, s3, t3, wd, sd, td, stride, min_tiles4,
                                            fuse_conv3)
    oh, ow = -(-h // stride), -(-w // stride)
    y = torch.empty(b, oh, ow, 4 * planes, dtype=torch.float32, device=x.device)
    nbytes = int(lib.mrcnn_bottleneck_workspace_bytes(b, h, w, cin, planes, stride, int(wd is not None)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    assert ws.data_ptr() % 256 == 0
    ptrs = (ctypes.c_void_p * 14)(*[_ptr(t) for t in (w1, s1, t1, w2, u2, u4, s2, t2, w3, s3, t3, wd, sd, td)])
    check(lib.mrcnn_bottleneck_forward_f32(x.data_ptr(), b, h, w, cin, planes, stride, ptrs, int(min_tiles4), int(bool(fuse_conv3)),
                                           ws.data_ptr(), nbytes, y.data_ptr(), _stream()))
    return y


def _bottleneck_launch_by_launch(x, w1, s1, t1, w2, u2, u4, s2, t2, w3, s3, t3, wd, sd, td, stride, min_tiles4, fuse_conv3):
    """The plan of mrcnn_bottleneck_forward_f32 (asked from the library), one binding call per launch."""
    b, h, w, cin = x.shape
    planes = w1.size(0)
    plan = bottleneck_plan(b, h, w, cin, planes, stride, u2 is not None, u4 is not None, min_tiles4, fuse_conv3)
    res = x if wd is None else conv_bn_act(x, wd, sd, td, stride=stride, relu=False)
    hmid = conv_bn_act(x, w1, s1, t1, stride=stride, relu=True, out_kblocked=bool(plan & 3))
    if plan & 4:
        return conv3x3_winograd4_conv3(hmid, u4, s2, t2, w3, s3, t3, res)
    if plan & 1:
        h2 = conv3x3_winograd4(hmid, u4, s2, t2, True)
    elif plan & 2:
        h2 = conv3x3_winograd(hmid, u2, s2, t2, True)
    else:
        h2 = conv_bn_act(hmid, w2, s2, t2, stride=1, pad=(1, 1, 1, 1), relu=True)
    return conv_bn_act(h2, w3, s3, t3, stride=1, relu=True, residual=res)


def bottleneck_forward(x, w1, s1, t1, w2, s2, t2, w3, s3, t3, wd, sd, td, stride: int):
    """torch.ops.maskrcnn.bottleneck_forward — Bottleneck.forward (model.py:190-211) on NHWC: conv1 1x1 (stride) + BN + ReLU,
    SamePad(3,1) + conv2 3x3 + BN + ReLU, conv3 1x1 + BN, + residual (identity or 1x1-stride downsample + BN), ReLU; BN / bias
    are (scale, shift) epilogues. ONE call of the C ABI per block (bottleneck_native): with Winograd enabled (the default) conv2
    runs the F(4x4) / F(2x2) kernels from cached transforms of w2 and the ResNet C2 blocks fuse conv2 + conv3 + residual into
    one launch — exactly what the inference pipeline launches; with MRCNN_WINOGRAD=0 every conv is the exact direct kernel
    (bitwise an fmaf chain). With BOTTLENECK_OP_FUSED (above) the stride-1 identity blocks with planes = 64 run the opt-in
    whole-block kernel instead."""
    from . import modules as _m
    if (BOTTLENECK_OP_FUSED and wd is None and int(stride) == 1 and x.is_cuda and x.dim() == 4
            and tuple(w2.shape[1:3]) == (3, 3)
            and bottleneck_fused_supported(x.size(1), x.size(2), x.size(3), w1.size(0)) and w3.size(0) == x.size(3)):
        return bottleneck_fused(x, w1, s1, t1, _cached_transform(winograd_weights, w2), s2, t2, w3, s3, t3)
    wino = bool(_m.WINOGRAD) and x.is_cuda and tuple(w2.shape[1:3]) == (3, 3) and w2.size(3) % 8 == 0
    u2 = _cached_transform(winograd_weights, w2) if wino else None
    u4 = _cached_transform(winograd4_weights, w2) if (wino and _m.WINOGRAD4 and _m.WINOGRAD4_TRUNK and w2.size(0) % 64 == 0) else None
    return bottleneck_native(x, w1, s1, t1, w2, u2, u4, s2, t2, w3, s3, t3, wd, sd, td, int(stride), _m.WINOGRAD4_MIN_TILES,
                             _m.FUSED_CONV3)


_LIB.define("bottleneck_forward(Tensor x, Tensor w1, Tensor s1, Tensor t1, Tensor w2, Tensor s2, "
            "Tensor t2, Tensor w3, Tensor s3, Tensor t3, Tensor? wd, Tensor? sd, Tensor? td, "
            "int stride) -> Tensor")
_LIB.impl("bottleneck_forward", bottleneck_forward, "CUDA")
_LIB.impl("bottleneck_forward", lambda x, *a: _need_gpu(x), "CPU")

@_on_device
def conv3x3_winograd_heads(x_kblocked: torch.Tensor, u: torch.Tensor, scale, shift, w_head32: torch.Tensor,
                           relu: bool = True, algo_cin=None, tile_mode: int | None = None) -> HeadSums:
    """RPN conv_shared + both 1x1 heads in one launch (model.py:605-607,624-641): relu(conv3x3_same(x)*scale + shift)
    stays on chip and is multiplied by w_head32 [32, Cout] (rows 0-17: conv_class then conv_bbox weights).
    x_kblocked [Cin/8,B,H,W,8]; u from winograd_weights. → HeadSums."""
    _need_gpu(x_kblocked, u, scale, shift, w_head32)
    assert x_kblocked.dim() == 5 and x_kblocked.is_contiguous() and x_kblocked.dtype == torch.float32
    g, b, h, w, _ = x_kblocked.shape
    cin, cout = g * 8, u.size(1)
    assert u.is_contiguous() and u.size(2) == cin and w_head32.is_contiguous() and tuple(w_head32.shape) == (32, cout)
    mode = int(lib.mrcnn_conv3x3_winograd_heads_tile_mode(h, w)) if tile_mode is None else int(tile_mode)
    if mode != 2 and not HAVE_ABLATIONS:
        raise RuntimeError("conv3x3_winograd_heads: maps of at least 16 x 16 pixels (8 x 8 tile positions) and the spatial-tile "
                           "kernel are required; the linear-tile heads variant is an MRCNN_ABLATIONS build")
    rows = int(lib.mrcnn_conv3x3_winograd_heads_rows(b, h, w, mode))
    part = torch.empty(2, rows, 32, dtype=torch.float32, device=x_kblocked.device)

    def book():
        m, k = b * h * w, 9 * (algo_cin or cin)
        algo = 2.0 * m * cout * (k + 18)                      # the 3x3 conv + both 1x1 heads (18 channels)
        executed = 2.0 * m * cout * (k / 2.25 + 32)           # Winograd multiplies + the head MFMAs on 32 padded columns
        return (algo, (m, cout, k), 4.0 * (m * cin + 2 * part.numel() / 2 + cout * k),
                "winograd_spatial" if mode == 2 else "winograd", executed)
    _launch(lib.mrcnn_conv3x3_winograd_heads_f32,
            (x_kblocked.data_ptr(), b, h, w, cin, u.data_ptr(), cout, _ptr(scale), _ptr(shift), 1 if relu else 0,
             w_head32.data_ptr(), mode, part.data_ptr(), _stream()), book)
    return HeadSums(part, b, h, w, mode)


@_on_device
def rpn_scores_deltas(heads, head_bias: torch.Tensor | None = None):
    """heads: 5 per-level entries (P2..P6), each a contiguous fp32 NHWC tensor [B,H_l,W_l,18] (fused RPN head outputs)
    or a HeadSums (conv3x3_winograd_heads; needs head_bias [18]) → (fg scores [B,A], deltas [B,A,4]) in the
    reference's anchor order. One launch."""
    assert len(heads) == 5
    tens = [h.part if isinstance(h, HeadSums) else h for h in heads]
    _need_gpu(*tens, head_bias)
    b = heads[0].batch if isinstance(heads[0], HeadSums) else heads[0].size(0)
    hs, ws, modes = [], [], []
    for h in heads:
        if isinstance(h, HeadSums):
            assert h.batch == b and h.part.is_contiguous() and head_bias is not None and head_bias.numel() == 18
            hs.append(h.height); ws.append(h.width); modes.append(h.tile_mode)
        else:
            assert h.is_contiguous() and h.dtype == torch.float32 and h.size(0) == b and h.size(3) == 18
            hs.append(h.size(1)); ws.append(h.size(2)); modes.append(0)
    a = 3 * sum(hh * ww for hh, ww in zip(hs, ws))
    scores = torch.empty(b, a, dtype=torch.float32, device=tens[0].device)
    deltas = torch.empty(b, a, 4, dtype=torch.float32, device=tens[0].device)
    ptrs = (c_vp * 5)(*[t.data_ptr() for t in tens])
    check(lib.mrcnn_rpn_scores_deltas_v2_f32(ptrs, (c_i32 * 5)(*hs), (c_i32 * 5)(*ws), (c_i32 * 5)(*modes),
                                             _ptr(head_bias), b, scores.data_ptr(), deltas.data_ptr(), _stream()))
    return scores, deltas


@_on_device
def proposal_decode(anchors, deltas, order, top_scores, std_dev, image_height, image_width):
    """anchors [A,4], deltas [B,A,4], order int64 [B,K], top_scores [B,K] → dets [B,K,5]: refined (data.py:124),
    clipped (data.py:86) boxes + score. One launch."""
    _need_gpu(anchors, deltas, order, top_scores)
    assert anchors.is_contiguous() and deltas.is_contiguous() and order.is_contiguous() and top_scores.is_contiguous()
    assert order.dtype == torch.int64 and deltas.dtype == torch.float32
    b, k = order.shape
    dets = torch.empty(b, k, 5, dtype=torch.float32, device=deltas.device)
    check(lib.mrcnn_proposal_decode_f32(anchors.data_ptr(), deltas.data_ptr(), order.data_ptr(),
                                        top_scores.data_ptr(), b, anchors.size(0), k,
                                        (c_f32 * 4)(*[float(v) for v in std_dev]), float(image_height),
                                        float(image_width), dets.data_ptr(), _stream()))
    return dets


@_on_device
def detection_decode(logits, bbox, rois, roi_counts, windows, std_dev, image_height, image_width,
                     min_confidence: float = 0.0):
    """First half of mrn_refine (model.py:1405-1443), one launch. logits [B*P,C] (row-strided view allowed),
    bbox [B*P,C,4] (row-strided view allowed), rois [B,P,4], roi_counts int32 [B], windows [B,4] →
    (dets [B,P,5], nms_class_ids int32 [B,P], class_ids int64 [B,P])."""
    _need_gpu(logits, bbox, rois, roi_counts, windows)
    b, p, _ = rois.shape
    c = logits.size(1)
    assert logits.stride(1) == 1 and bbox.stride(2) == 1 and bbox.stride(1) == 4 and rois.is_contiguous()
    assert roi_counts.dtype == torch.int32 and windows.dtype == torch.float32 and windows.is_contiguous()
    dets = torch.empty(b, p, 5, dtype=torch.float32, device=rois.device)
    nms_cls = torch.empty(b, p, dtype=torch.int32, device=rois.device)
    cls = torch.empty(b, p, dtype=torch.int64, device=rois.device)
    check(lib.mrcnn_detection_decode_f32(logits.data_ptr(), logits.stride(0), bbox.data_ptr(), bbox.stride(0),
                                         rois.data_ptr(), roi_counts.data_ptr(), windows.data_ptr(), b, p, c,
                                         (c_f32 * 4)(*[float(v) for v in std_dev]), float(image_height),
                                         float(image_width), float(min_confidence), dets.data_ptr(),
                                         nms_cls.data_ptr(), cls.data_ptr(), _stream()))
    return dets, nms_cls, cls


@_on_device
def topk_desc(scores: torch.Tensor, k: int):
    """scores fp32 [B,N] → (top [B,k], order int64 [B,k]): descending, ties by ascending index (model.py:1345-1350)."""
    _need_gpu(scores)
    assert scores.dtype == torch.float32 and scores.dim() == 2 and scores.is_contiguous()
    b, n = scores.shape
    top = torch.empty(b, k, dtype=torch.float32, device=scores.device)
    order = torch.empty(b, k, dtype=torch.int64, device=scores.device)
    nbytes = int(lib.mrcnn_topk_workspace_bytes(b))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=scores.device)
    check(lib.mrcnn_topk_desc_f32(scores.data_ptr(), b, n, k, top.data_ptr(), order.data_ptr(), ws.data_ptr(), nbytes,
                                  _stream()))
    return top, order


@_on_device
def proposal_select(dets, keep, keep_counts, proposal_count: int, image_height, image_width):
    """dets [B,K,5], NMS keep int64 [B,K] + counts int32 [B] → (rois [B,P,4] normalised, zero-padded; counts int32 [B])
    — keep[:proposal_count], gather, normalise (model.py:1366-1374) in one launch."""
    _need_gpu(dets, keep, keep_counts)
    assert dets.is_contiguous() and keep.is_contiguous() and keep.dtype == torch.int64
    assert keep_counts.dtype == torch.int32 and keep_counts.is_contiguous()
    b, k, _ = dets.shape
    rois = torch.empty(b, proposal_count, 4, dtype=torch.float32, device=dets.device)
    counts = torch.empty(b, dtype=torch.int32, device=dets.device)
    check(lib.mrcnn_proposal_select_f32(dets.data_ptr(), keep.data_ptr(), keep_counts.data_ptr(), b, k,
                                        proposal_count, float(image_height), float(image_width), rois.data_ptr(),
                                        counts.data_ptr(), _stream()))
    return rois, counts


@_on_device
def detection_select(dets, nms_class_ids, class_ids, keep, keep_counts, max_instances: int, image_height,
                     image_width):
    """Tail of mrn_refine (model.py:1475-1487) in one launch → (class_ids int64 [B,D], scores [B,D], boxes [B,D,4]
    pixels, rois [B,D,4] normalised for the mask head, counts int32 [B]); unused slots are zero."""
    _need_gpu(dets, nms_class_ids, class_ids, keep, keep_counts)
    assert dets.is_contiguous() and nms_class_ids.is_contiguous() and class_ids.is_contiguous()
    assert keep.is_contiguous() and keep.dtype == torch.int64 and class_ids.dtype == torch.int64
    assert nms_class_ids.dtype == torch.int32 and keep_counts.dtype == torch.int32
    b, p, _ = dets.shape
    d, dev = max_instances, dets.device
    ids = torch.empty(b, d, dtype=torch.int64, device=dev)
    scores = torch.empty(b, d, dtype=torch.float32, device=dev)
    boxes = torch.empty(b, d, 4, dtype=torch.float32, device=dev)
    rois = torch.empty(b, d, 4, dtype=torch.float32, device=dev)
    counts = torch.empty(b, dtype=torch.int32, device=dev)
    check(lib.mrcnn_detection_select_f32(dets.data_ptr(), nms_class_ids.data_ptr(), class_ids.data_ptr(),
                                         keep.data_ptr(), keep_counts.data_ptr(), b, p, d, float(image_height),
                                         float(image_width), ids.data_ptr(), scores.data_ptr(), boxes.data_ptr(),
                                         rois.data_ptr(), counts.data_ptr(), _stream()))
    return ids, scores, boxes, rois, counts


@_on_device
def deconv2x2(x: torch.Tensor, w, bias4: torch.Tensor, activation: int = 0, products: int = 0) -> torch.Tensor:
    """2x2 stride-2 transposed conv + bias + activation (Mask.forward's deconv, model.py:864,906-912) as one GEMM
    scattering into [B,2H,2W,Cout]. w: fp32 [4*Cout,1,1,Cin] (products = 0) or the (w_hi, w_lo) fp16 planes of it
    (products = 1 or 3); bias4 [4*Cout]."""
    _need_gpu(x, bias4)
    assert x.is_contiguous() and x.dtype in (torch.float32, torch.float16) and bias4.is_contiguous()
    b, h, wd, cin = x.shape
    w0 = w if products == 0 else w[0]
    cout = w0.size(0) // 4
    assert w0.size(3) == cin and bias4.numel() == 4 * cout
    y = torch.empty(b, 2 * h, 2 * wd, cout, dtype=x.dtype, device=x.device)

    def book():
        m = b * h * wd
        return (2.0 * m * cin * 4 * cout, (m, 4 * cout, cin),
                x.element_size() * (x.numel() + y.numel()) + (4 if products == 0 else 2 * (2 if products == 3 else 1)) * w0.numel(),
                "direct" if products == 0 else "f16")
    if products == 0:
        assert w.dtype == torch.float32 and w.is_contiguous()
        _launch(lib.mrcnn_deconv2x2_bias_act_nhwc_f32,
                (x.data_ptr(), b, h, wd, cin, w.data_ptr(), cout, bias4.data_ptr(), int(activation), y.data_ptr(), _stream()), book)
    elif x.dtype == torch.float16:   # fp16 activations: plain-fp16 mode only
        assert products == 1
        _launch(lib.mrcnn_deconv2x2_bias_act_nhwc_f16io,
                (x.data_ptr(), b, h, wd, cin, w[0].data_ptr(), cout, bias4.data_ptr(), int(activation), y.data_ptr(), _stream()),
                book)
    else:
        w_hi, w_lo = w
        _launch(lib.mrcnn_deconv2x2_bias_act_nhwc_f16mfma,
                (x.data_ptr(), b, h, wd, cin, w_hi.data_ptr(), _ptr(w_lo), cout, bias4.data_ptr(), int(activation), int(products),
                 y.data_ptr(), _stream()), book)
    return y


HAVE_ABLATIONS = hasattr(lib, "mrcnn_rpn_level_fused_f32")   # an MRCNN_ABLATIONS build of the library is loaded


@_on_device
def rpn_level_fused(x, w_shared, b_shared, w_head32, b_head, head_n: int = 18) -> torch.Tensor:
    """RPN.forward on one level (model.py:609-649) with the shared 512-channel activation kept on chip:
    x [B,H,W,Cin] NHWC → [B,H,W,head_n] (class logits then box deltas). fp32 MFMA path, direct kernel. MRCNN_ABLATIONS
    builds only (the default library fuses the heads into the Winograd kernels instead)."""
    if not HAVE_ABLATIONS:
        raise RuntimeError("rpn_level_fused: built only with MRCNN_ABLATIONS=1 python maskrcnn_amd/build.py")
    _need_gpu(x, w_shared, b_shared, w_head32, b_head)
    assert x.is_contiguous() and w_shared.is_contiguous() and w_head32.is_contiguous()
    b, h, wd, cin = x.shape
    cout = w_shared.size(0)
    assert tuple(w_shared.shape[1:]) == (3, 3, cin) and tuple(w_head32.shape) == (32, cout)
    ws_bytes = int(lib.mrcnn_rpn_level_workspace_bytes(b, h, wd, cout, head_n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    y = torch.empty(b, h, wd, head_n, dtype=torch.float32, device=x.device)

    def book():
        m = b * h * wd
        flops = 2.0 * m * (9 * cin * cout + cout * head_n)  # shared 3x3 conv + both 1x1 heads
        return flops, (m, cout, 9 * cin), 4 * (x.numel() + w_shared.numel() + cout * head_n + y.numel()), "rpn_fused"
    _launch(lib.mrcnn_rpn_level_fused_f32,
            (x.data_ptr(), b, h, wd, cin, w_shared.data_ptr(), cout, _ptr(b_shared), w_head32.data_ptr(), _ptr(b_head),
             int(head_n), ws.data_ptr(), ws_bytes, y.data_ptr(), _stream()), book)
    return y


# --------------------------------------------------------------------------------------------------
# image pre-/post-processing (Pillow-exact 8-bit bilinear resample)
# --------------------------------------------------------------------------------------------------
@_on_device
def resize_bilinear_u8(image: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
    """uint8 [H,W], [H,W,C] (C <= 4) or a batch [N,H,W] of single-channel images (rows contiguous; image and row
    strides free, so a cropped view needs no copy) → uint8 of the same rank at out_h x out_w; every image
    == Image.fromarray(a).resize((out_w, out_h), Image.BILINEAR)."""
    _need_gpu(image)
    if image.dtype != torch.uint8 or image.dim() not in (2, 3):
        raise RuntimeError(f"resize_bilinear_u8: expected a uint8 2-d or 3-d tensor, got {image.dtype} {tuple(image.shape)}")
    a = image
    if a.dim() == 3 and a.size(2) <= 4 and a.stride(2) == 1 and a.stride(1) == a.size(2):   # [H,W,C] interleaved
        n, h, w, c = 1, a.size(0), a.size(1), a.size(2)
        image_stride, row_stride = 0, a.stride(0)
        out_shape = (out_h, out_w, c)
    elif a.dim() == 2:
        if a.stride(1) != 1:
            a = a.contiguous()
        n, h, w, c = 1, a.size(0), a.size(1), 1
        image_stride, row_stride = 0, a.stride(0)
        out_shape = (out_h, out_w)
    else:                                                                                     # [N,H,W]
        if a.stride(2) != 1:
            a = a.contiguous()
        n, h, w, c = a.size(0), a.size(1), a.size(2), 1
        image_stride, row_stride = a.stride(0), a.stride(1)
        out_shape = (n, out_h, out_w)
    if out_h < 1 or out_w < 1:
        raise ValueError("height and width must be > 0")       # PIL's message for an empty size
    out = torch.empty(out_shape, dtype=torch.uint8, device=a.device)
    if n == 0:
        return out
    nbytes = int(lib.mrcnn_resize_u8_workspace_bytes(n, h, w, c, out_h, out_w))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=a.device)
    check(lib.mrcnn_resize_bilinear_u8(a.data_ptr(), n, h, w, c, image_stride, row_stride, out.data_ptr(), out_h,
                                       out_w, ws.data_ptr(), nbytes, _stream()))
    return out


@_on_device
def mold_image_u8(image: torch.Tensor, new_h: int, new_w: int, top: int, left: int, out: torch.Tensor,
                  mean_pixel) -> None:
    """uint8 RGB [h,w,3] → out fp32 [3,H,W] (one slot of the batch): resize to new_h x new_w, paste at (top,left) of a
    zero canvas, subtract mean_pixel in double, HWC → CHW. One call replaces utils.py:72-88 + model.py:1754,1108."""
    _need_gpu(image, out)
    if image.dtype != torch.uint8 or image.dim() != 3 or image.size(2) != 3:
        raise RuntimeError(f"mold_image_u8: expected uint8 [h,w,3], got {image.dtype} {tuple(image.shape)}")
    assert out.dtype == torch.float32 and out.dim() == 3 and out.size(0) == 3 and out.is_contiguous()
    a = image.contiguous()
    h, w = a.shape[:2]
    nbytes, ws = 0, None
    if (new_h, new_w) != (h, w):
        nbytes = int(lib.mrcnn_resize_u8_workspace_bytes(1, h, w, 3, new_h, new_w))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=a.device)
    mean = (ctypes.c_double * 3)(*[float(m) for m in mean_pixel])
    check(lib.mrcnn_mold_image_u8(a.data_ptr(), h, w, new_h, new_w, top, left, out.size(1), out.size(2), mean,
                                  out.data_ptr(), _ptr(ws), nbytes, _stream()))


@_on_device
def mold_images_u8(images: torch.Tensor, new_h: int, new_w: int, top: int, left: int, out: torch.Tensor, mean_pixel) -> None:
    """n RGB images of ONE size, uint8 [n,h,w,3] contiguous → out fp32 [n,3,H,W]: mold_image_u8 for a whole batch in one set of
    launches (coefficient tables, horizontal pass, vertical + mold pass)."""
    _need_gpu(images, out)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.size(3) != 3 or not images.is_contiguous():
        raise RuntimeError(f"mold_images_u8: expected contiguous uint8 [n,h,w,3], got {images.dtype} {tuple(images.shape)}")
    n, h, w = images.shape[:3]
    assert out.dtype == torch.float32 and out.dim() == 4 and out.size(0) == n and out.size(1) == 3 and out.is_contiguous()
    nbytes, ws = 0, None
    if (new_h, new_w) != (h, w):
        nbytes = int(lib.mrcnn_resize_u8_workspace_bytes(n, h, w, 3, new_h, new_w))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=images.device)
    mean = (ctypes.c_double * 3)(*[float(m) for m in mean_pixel])
    check(lib.mrcnn_mold_images_u8(images.data_ptr(), n, h * w * 3, h, w, new_h, new_w, top, left, out.size(2), out.size(3), mean,
                                   out.data_ptr(), _ptr(ws), nbytes, _stream()))


@_on_device
def paste_masks(masks: torch.Tensor, class_ids: torch.Tensor, boxes: torch.Tensor, height: int, width: int,
                channels_last: bool, as_l8: bool = False) -> torch.Tensor:
    """datalib.full_masks (data.py:287-314) for N detections in one launch → bool [N,height,width] (as_l8: the same
    mask as a uint8 0/255 'L' image, what decode_masks converts it to before resizing, data.py:271).
    masks fp32 [N,C,mh,mw] (channels_last=False, the reference layout) or [N,mh,mw,C] (True), any strides;
    class_ids int64 [N]; boxes fp32 [N,4] pixel (y1,x1,y2,x2)."""
    _need_gpu(masks, class_ids, boxes)
    if masks.dtype != torch.float32 or masks.dim() != 4:
        raise RuntimeError(f"paste_masks: expected fp32 4-d masks, got {masks.dtype} {tuple(masks.shape)}")
    n = masks.size(0)
    if channels_last:
        mh, mw, c = masks.shape[1:]
        sn, sy, sx, sc = masks.stride()
    else:
        c, mh, mw = masks.shape[1:]
        sn, sc, sy, sx = masks.stride()
    class_ids = class_ids.to(torch.int64).contiguous()
    boxes = boxes.to(torch.float32).contiguous()
    assert class_ids.numel() == n and tuple(boxes.shape) == (n, 4)
    out = torch.empty(n, height, width, dtype=torch.uint8, device=masks.device)
    check(lib.mrcnn_paste_masks_u8(masks.data_ptr(), sn, sy, sx, sc, n, mh, mw, c, class_ids.data_ptr(),
                                   boxes.data_ptr(), height, width, 255 if as_l8 else 1, out.data_ptr(), _stream()))
    return out if as_l8 else out.view(torch.bool)


# --------------------------------------------------------------------------------------------------
# COCO run-length encoding of masks (csrc/rle.hip)
# --------------------------------------------------------------------------------------------------
def rle_default_capacity(height: int, width: int) -> int:
    """Runs per mask rle_encode reserves when the caller names no capacity: four transitions per column (two blobs crossing
    every column) and never less than 1024, never more than a mask can have (H*W + 1)."""
    return min(height * width + 1, max(1024, 4 * width + 2))


@_on_device
def rle_encode(masks: torch.Tensor, threshold: int = 0, capacity: int | None = None):
    """COCO RLE (maskUtils.encode: rleEncode + rleToString + rleArea + rleToBbox of cocoapi/common/maskApi.c) of uint8 or bool
    masks [N,H,W] or [H,W] (N = 1) on the GPU; the last stride must be 1, image and row strides are free (a cropped view needs
    no copy). A pixel is on iff its byte > threshold. → (num_runs int32 [N], counts int32 [N,capacity], strings uint8
    [N,6*capacity], string_bytes int32 [N], areas int32 [N], bboxes int32 [N,4] (x, y, w, h)), all on the device, no host
    synchronisation. A mask with more than `capacity` runs (default rle_default_capacity(H, W)) reports its true num_runs, area
    and bbox, string_bytes 0, and its counts / strings rows are not written (they are uninitialised memory here)."""
    _need_gpu(masks)
    if masks.dtype not in (torch.uint8, torch.bool) or masks.dim() not in (2, 3):
        raise RuntimeError(f"rle_encode: expected a uint8 or bool [N,H,W] or [H,W] tensor, got {masks.dtype} {tuple(masks.shape)}")
    a = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
    if a.dim() == 2:
        a = a.unsqueeze(0)
    n, h, w = a.shape
    if w > 1 and a.stride(2) != 1:
        raise RuntimeError(f"rle_encode: the last stride must be 1, got strides {tuple(masks.stride())}")
    if capacity is None:
        capacity = rle_default_capacity(h, w)
    capacity = int(capacity)
    image_stride = a.stride(0) if n > 1 else 0
    row_stride = a.stride(1) if h > 1 else w
    dev = a.device
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    num_runs, string_bytes, areas, bboxes = i32(n), i32(n), i32(n), i32(n, 4)
    counts = i32(n, max(capacity, 0))
    strings = torch.empty(n, 6 * max(capacity, 0), dtype=torch.uint8, device=dev)
    nbytes = int(lib.mrcnn_rle_workspace_bytes(n, h, w))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _launch(lib.mrcnn_rle_encode_u8,
            (a.data_ptr(), image_stride, row_stride, n, h, w, int(threshold), capacity, num_runs.data_ptr(), counts.data_ptr(),
             strings.data_ptr(), string_bytes.data_ptr(), areas.data_ptr(), bboxes.data_ptr(), ws.data_ptr(), nbytes, _stream()),
            lambda: (0, (n, h, w), n * h * w, "rle_encode"))
    return num_runs, counts, strings, string_bytes, areas, bboxes


_LIB.define("rle_encode(Tensor masks, int threshold=0, int? capacity=None) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
_LIB.impl("rle_encode", rle_encode, "CUDA")
_LIB.impl("rle_encode", lambda masks, *a: _need_gpu(masks), "CPU")


# --------------------------------------------------------------------------------------------------
# COCO evaluation: grouped RLE / box IoU and the matching of evaluateImg (csrc/cocoeval.hip)
# --------------------------------------------------------------------------------------------------
def _rle_table(obj, who: str):
    """(num_runs int32 [N], counts [N,capacity] as int32) of an image.RleMasks or of the two tensors themselves."""
    if hasattr(obj, "num_runs") and hasattr(obj, "counts"):
        obj = (obj.num_runs, obj.counts)
    if not (isinstance(obj, (tuple, list)) and len(obj) == 2 and all(isinstance(t, torch.Tensor) for t in obj)):
        raise RuntimeError(f"{who}: expected an RleMasks or the (num_runs, counts) tensors")
    num_runs, counts = obj
    _need_gpu(num_runs, counts)
    if counts.dtype == getattr(torch, "uint32", None):
        counts = counts.view(torch.int32)
    if num_runs.dtype != torch.int32 or counts.dtype != torch.int32 or num_runs.dim() != 1 or counts.dim() != 2 \
            or counts.size(0) != num_runs.size(0) or counts.size(1) < 1:
        raise RuntimeError(f"{who}: expected num_runs int32 [N] and counts int32 / uint32 [N,capacity >= 1], got "
                           f"{num_runs.dtype} {tuple(num_runs.shape)} and {counts.dtype} {tuple(counts.shape)}")
    return num_runs.contiguous(), counts.contiguous()


def _group_offsets(who, m: int, n: int, dt_off, gt_off, out_off, out_len, dev):
    """The three offset tensors of a grouped call (int32, int32, int64, [K+1] each, on the device) and the output length;
    all None = ONE group of every detection against every ground truth."""
    given = [o is not None for o in (dt_off, gt_off, out_off)]
    if not any(given):
        dt_off = torch.tensor([0, m], dtype=torch.int32, device=dev)
        gt_off = torch.tensor([0, n], dtype=torch.int32, device=dev)
        out_off = torch.tensor([0, m * n], dtype=torch.int64, device=dev)
        return dt_off, gt_off, out_off, m * n, True
    if not all(given):
        raise RuntimeError(f"{who}: dt_off, gt_off and out_off come together")
    _need_gpu(dt_off, gt_off, out_off)
    if dt_off.dtype != torch.int32 or gt_off.dtype != torch.int32 or out_off.dtype != torch.int64 or dt_off.dim() != 1 \
            or dt_off.numel() < 1 or dt_off.shape != gt_off.shape or dt_off.shape != out_off.shape:
        raise RuntimeError(f"{who}: offsets are int32 [K+1], int32 [K+1] and int64 [K+1] device tensors")
    if out_len is None:
        out_len = int(out_off[-1])   # one host read; pass out_len to stay asynchronous
    return dt_off.contiguous(), gt_off.contiguous(), out_off.contiguous(), int(out_len), False


def _crowd(who, iscrowd, n: int):
    if iscrowd is None:
        return None
    _need_gpu(iscrowd)
    if iscrowd.dtype == torch.bool:
        iscrowd = iscrowd.view(torch.uint8)
    if iscrowd.dtype != torch.uint8 or iscrowd.shape != (n,):
        raise RuntimeError(f"{who}: iscrowd is a uint8 / bool [{n}] tensor, got {iscrowd.dtype} {tuple(iscrowd.shape)}")
    return iscrowd.contiguous()


def _iou_out(who, out, out_len: int, dev):
    if out is None:
        return torch.zeros(out_len, dtype=torch.float64, device=dev)
    if out.dtype != torch.float64 or out.dim() != 1 or out.numel() < out_len or not out.is_contiguous() or out.device != dev:
        raise RuntimeError(f"{who}: out must be a contiguous float64 [{out_len}] tensor on {dev}")
    return out


@_on_device
def _rle_iou(dt_num_runs: torch.Tensor, dt_counts: torch.Tensor, gt_num_runs: torch.Tensor, gt_counts: torch.Tensor,
             iscrowd: torch.Tensor | None = None, dt_off: torch.Tensor | None = None, gt_off: torch.Tensor | None = None,
             out_off: torch.Tensor | None = None, out_len: int | None = None, out: torch.Tensor | None = None):
    dnr, dc = _rle_table((dt_num_runs, dt_counts), "rle_iou")
    gnr, gc = _rle_table((gt_num_runs, gt_counts), "rle_iou")
    m, n, dev = dnr.size(0), gnr.size(0), dnr.device
    crowd = _crowd("rle_iou", iscrowd, n)
    dt_off, gt_off, out_off, out_len, single = _group_offsets("rle_iou", m, n, dt_off, gt_off, out_off, out_len, dev)
    res = _iou_out("rle_iou", out, out_len, dev)
    nbytes = int(lib.mrcnn_rle_iou_workspace_bytes(m, dc.size(1), n, gc.size(1)))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _launch(lib.mrcnn_rle_iou_f64,
            (dnr.data_ptr(), dc.data_ptr(), m, dc.size(1), gnr.data_ptr(), gc.data_ptr(), n, gc.size(1), _ptr(crowd),
             dt_off.data_ptr(), gt_off.data_ptr(), out_off.data_ptr(), dt_off.numel() - 1, res.data_ptr(), out_len,
             ws.data_ptr(), nbytes, _stream()),
            lambda: (0, (m, n, out_len), 4 * (dc.numel() + gc.numel()) + 8 * out_len, "rle_iou"))
    return res[:m * n].view(n, m).t() if single else res


def rle_iou(dt, gt, iscrowd: torch.Tensor | None = None, dt_off=None, gt_off=None, out_off=None, out_len=None, out=None):
    """maskUtils.iou on run-length masks (rleIou of cocoapi/common/maskApi.c:77-96, the same bits) on the GPU. dt and gt are
    image.RleMasks or their (num_runs int32 [N], counts [N,capacity]) device tensors — what rle_encode returns, no host trip.
    iscrowd: uint8 [len(gt)]. Without offsets: every detection against every ground truth → float64 [m, n] (a Fortran-order
    view, as _mask.pyx:239 returns). Grouped (include/maskrcnn_hip.h): dt_off / gt_off int32 [K+1] and out_off int64 [K+1]
    device tensors name K groups; → the flat float64 [out_len] buffer with group k's o[g*m + d] matrix at out_off[k] (elements
    of no group stay 0). A pair with a mask that did not fit its capacity is -1."""
    return _rle_iou(*_rle_table(dt, "rle_iou"), *_rle_table(gt, "rle_iou"), iscrowd, dt_off, gt_off, out_off, out_len, out)


@_on_device
def bbox_iou(dt: torch.Tensor, gt: torch.Tensor, iscrowd: torch.Tensor | None = None, dt_off=None, gt_off=None, out_off=None,
             out_len=None, out=None):
    """maskUtils.iou on boxes (bbIou of maskApi.c:109-120, operation by operation in fp64) for float64 (x, y, w, h) boxes
    dt [m,4] and gt [n,4] on the GPU; single-group and grouped forms and the result layout as rle_iou."""
    _need_gpu(dt, gt)
    for name, b in (("dt", dt), ("gt", gt)):
        if b.dtype != torch.float64 or b.dim() != 2 or b.size(1) != 4:
            raise RuntimeError(f"bbox_iou: {name} must be a float64 [N,4] tensor, got {b.dtype} {tuple(b.shape)}")
    dt, gt = dt.contiguous(), gt.contiguous()
    m, n, dev = dt.size(0), gt.size(0), dt.device
    crowd = _crowd("bbox_iou", iscrowd, n)
    dt_off, gt_off, out_off, out_len, single = _group_offsets("bbox_iou", m, n, dt_off, gt_off, out_off, out_len, dev)
    res = _iou_out("bbox_iou", out, out_len, dev)
    _launch(lib.mrcnn_bbox_iou_f64,
            (dt.data_ptr(), m, gt.data_ptr(), n, _ptr(crowd), dt_off.data_ptr(), gt_off.data_ptr(), out_off.data_ptr(),
             dt_off.numel() - 1, res.data_ptr(), out_len, _stream()),
            lambda: (0, (m, n, out_len), 32 * (m + n) + 8 * out_len, "bbox_iou"))
    return res[:m * n].view(n, m).t() if single else res


@_on_device
def coco_match(ious: torch.Tensor, dt_off: torch.Tensor, gt_off: torch.Tensor, out_off: torch.Tensor, dt_area: torch.Tensor,
               gt_area: torch.Tensor, gt_iscrowd: torch.Tensor, area_ranges: torch.Tensor, thresholds: torch.Tensor, out=None):
    """The matching of COCOeval.evaluateImg (cocoeval.py:251-300) for every group x area range x IoU threshold in one launch.
    ious: the flat float64 buffer of a grouped rle_iou / bbox_iou with the same offsets; dt_area float64 [N] (detections of a
    group sorted by descending score, cut at maxDet), gt_area float64 [M], gt_iscrowd uint8 [M], area_ranges float64 [A,2],
    thresholds float64 [T], all on the device. → (dt_match int32 [A,T,N], gt_match int32 [A,T,M], dt_ignore uint8 [A,T,N],
    gt_ignore uint8 [A,M]); matches are 1-based positions within the group in input order, 0 = none. `out` = those four
    tensors, preallocated."""
    _need_gpu(ious, dt_off, gt_off, out_off, dt_area, gt_area, gt_iscrowd, area_ranges, thresholds)
    n_dt, n_gt, dev = dt_area.numel(), gt_area.numel(), dt_area.device
    if gt_iscrowd.dtype == torch.bool:
        gt_iscrowd = gt_iscrowd.view(torch.uint8)
    if ious.dtype != torch.float64 or dt_area.dtype != torch.float64 or gt_area.dtype != torch.float64 \
            or area_ranges.dtype != torch.float64 or thresholds.dtype != torch.float64 or gt_iscrowd.dtype != torch.uint8:
        raise RuntimeError("coco_match: ious, areas, area_ranges and thresholds are float64 tensors, gt_iscrowd uint8")
    if area_ranges.dim() != 2 or area_ranges.size(1) != 2 or thresholds.dim() != 1 or gt_iscrowd.numel() != n_gt \
            or area_ranges.size(0) < 1 or thresholds.numel() < 1:
        raise RuntimeError("coco_match: area_ranges is [A,2], thresholds [T], gt_iscrowd as long as gt_area")
    dt_off, gt_off, out_off, _, _ = _group_offsets("coco_match", n_dt, n_gt, dt_off, gt_off, out_off, 0, dev)
    ious, dt_area, gt_area, gt_iscrowd = ious.contiguous().view(-1), dt_area.contiguous(), gt_area.contiguous(), gt_iscrowd.contiguous()
    area_ranges, thresholds = area_ranges.contiguous(), thresholds.contiguous()
    a, t = area_ranges.size(0), thresholds.numel()
    shapes = ((a, t, n_dt), (a, t, n_gt), (a, t, n_dt), (a, n_gt))
    dtypes = (torch.int32, torch.int32, torch.uint8, torch.uint8)
    if out is None:
        out = tuple(torch.zeros(s, dtype=d, device=dev) for s, d in zip(shapes, dtypes))
    for o, s, d in zip(out, shapes, dtypes):
        if o.dtype != d or tuple(o.shape) != s or not o.is_contiguous() or o.device != dev:
            raise RuntimeError(f"coco_match: out tensors must be contiguous {dtypes} of shapes {shapes} on {dev}")
    dt_match, gt_match, dt_ignore, gt_ignore = out
    _launch(lib.mrcnn_coco_match,
            (ious.data_ptr() if ious.numel() else None, ious.numel(), dt_off.data_ptr(), gt_off.data_ptr(), out_off.data_ptr(),
             dt_off.numel() - 1, _ptr(dt_area) if n_dt else None, n_dt, _ptr(gt_area) if n_gt else None,
             _ptr(gt_iscrowd) if n_gt else None, n_gt, area_ranges.data_ptr(), a, thresholds.data_ptr(), t,
             _ptr(dt_match) if n_dt else None, _ptr(gt_match) if n_gt else None, _ptr(dt_ignore) if n_dt else None,
             _ptr(gt_ignore) if n_gt else None, _stream()),
            lambda: (0, (dt_off.numel() - 1, a, t), 8 * ious.numel(), "coco_match"))
    return dt_match, gt_match, dt_ignore, gt_ignore


_LIB.define("rle_iou(Tensor dt_num_runs, Tensor dt_counts, Tensor gt_num_runs, Tensor gt_counts, Tensor? iscrowd=None, "
            "Tensor? dt_off=None, Tensor? gt_off=None, Tensor? out_off=None, int? out_len=None) -> Tensor")
_LIB.impl("rle_iou", _rle_iou, "CUDA")
_LIB.impl("rle_iou", lambda dt_num_runs, *a: _need_gpu(dt_num_runs), "CPU")
_LIB.define("bbox_iou(Tensor dt, Tensor gt, Tensor? iscrowd=None, Tensor? dt_off=None, Tensor? gt_off=None, "
            "Tensor? out_off=None, int? out_len=None) -> Tensor")
_LIB.impl("bbox_iou", bbox_iou, "CUDA")
_LIB.impl("bbox_iou", lambda dt, *a: _need_gpu(dt), "CPU")


# --------------------------------------------------------------------------------------------------
# COCO polygons to run lengths: rleFrPoly and rleMerge, grouped (csrc/poly.hip)
# --------------------------------------------------------------------------------------------------
POLY_MAX_DIM = 16384
POLY_MAX_PART_POINTS = 1 << 24


def poly_host_bounds(xy, vert_off, heights, widths, who: str = "rle_from_poly", error=RuntimeError):
    """The limits of mrcnn_rle_from_poly_f64 (include/maskrcnn_hip.h) checked on host copies of its arguments — numpy: xy float64
    [V,2], vert_off [n+1], heights / widths [n] — and, per part, a conservative bound on the keys the kernel can keep: the sum over
    the edges of |dX| // 5 + 1 (a crossing falls on a pixel column only where u = 2 mod 5). The bound sizes tables; no value computed
    here reaches an output. Raises `error` at the first value past a limit."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    off = np.asarray(vert_off, dtype=np.int64).reshape(-1)
    hs, ws = np.asarray(heights, dtype=np.int64).reshape(-1), np.asarray(widths, dtype=np.int64).reshape(-1)
    n, v = hs.size, xy.shape[0]
    if off.size != n + 1 or ws.size != n:
        raise error(f"{who}: vert_off has {off.size} entries and widths {ws.size} for {n} parts")
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    if off[0] != 0 or off[-1] != v:
        raise error(f"{who}: vert_off must start at 0 and end at the number of vertices {v}, got {int(off[0])} .. {int(off[-1])}")
    k = np.diff(off)
    if (k < 1).any():
        raise error(f"{who}: part {int(np.argmax(k < 1))} has no vertex (vert_off must increase)")
    for name, a in (("height", hs), ("width", ws)):
        if ((a < 1) | (a > POLY_MAX_DIM)).any():
            i = int(np.argmax((a < 1) | (a > POLY_MAX_DIM)))
            raise error(f"{who}: part {i} has {name} {int(a[i])}, outside [1, {POLY_MAX_DIM}]")
    if not np.isfinite(xy).all():
        raise error(f"{who}: vertex {int(np.argmax(~np.isfinite(xy).all(1)))} is not finite")
    g = np.trunc(5.0 * xy + .5)                       # the grid vertices, as floats: no integer can overflow here
    if (np.abs(5.0 * xy + .5) >= 2.0 ** 31).any():
        raise error(f"{who}: vertex {int(np.argmax((np.abs(5.0 * xy + .5) >= 2.0 ** 31).any(1)))}: |5*v + .5| must stay below 2^31")
    nxt = np.arange(1, v + 1)
    nxt[off[1:] - 1] = off[:-1]                       # the closing edge of every part
    d = np.abs(g[nxt] - g)
    sums = lambda per_edge: np.add.reduceat(per_edge, off[:-1])
    points = sums(d.max(1) + 1)
    if (points > POLY_MAX_PART_POINTS).any():
        i = int(np.argmax(points > POLY_MAX_PART_POINTS))
        raise error(f"{who}: part {i} has {int(points[i])} boundary points, more than {POLY_MAX_PART_POINTS}")
    return sums(np.floor(d[:, 0] / 5.0) + 1).astype(np.int64)


def rle_from_poly_onchip_keys() -> int:
    """Keys of one part that rle_from_poly sorts on chip in one piece; a part with more is sorted range by range."""
    return int(lib.mrcnn_rle_from_poly_onchip_keys())


@_on_device
def rle_from_poly(xy: torch.Tensor, vert_off: torch.Tensor, heights: torch.Tensor, widths: torch.Tensor,
                  capacity: int | None = None):
    """maskUtils.frPyObjects on polygons (rleFrPoly of cocoapi/common/maskApi.c:162-202, the same bits) for n polygon parts in one
    call on the GPU. xy float64 [V,2] (or flat [2V]): all parts' vertices; vert_off int32 [n+1]: part i owns vertices
    [vert_off[i], vert_off[i+1]); heights / widths int32 [n]: every part has its own image size. All device tensors.
    → (num_runs int32 [n], counts int32 [n,capacity], num_keys int32 [n]): the run-list table ops.rle_iou and ops.rle_merge read, and
    the column crossings each part kept before the parity rule. A part with more runs than capacity reports its true num_runs and
    its row is not written (uninitialised memory here). capacity=None: the arguments are read back once, checked against the limits
    of include/maskrcnn_hip.h (RuntimeError at the first value past one) and the capacity is the host's key bound + 1, which no part
    exceeds. With a capacity the call never synchronises; a part past a limit then reports num_runs = num_keys = -1."""
    _need_gpu(xy, vert_off, heights, widths)
    if xy.dtype != torch.float64 or not (xy.dim() == 1 and xy.numel() % 2 == 0 or xy.dim() == 2 and xy.size(1) == 2):
        raise RuntimeError(f"rle_from_poly: xy must be a float64 [V,2] tensor, got {xy.dtype} {tuple(xy.shape)}")
    for name, t in (("vert_off", vert_off), ("heights", heights), ("widths", widths)):
        if t.dtype != torch.int32 or t.dim() != 1:
            raise RuntimeError(f"rle_from_poly: {name} must be an int32 vector, got {t.dtype} {tuple(t.shape)}")
    n, v = heights.numel(), xy.numel() // 2
    if vert_off.numel() != n + 1 or widths.numel() != n:
        raise RuntimeError(f"rle_from_poly: {n} heights need {n} widths and {n + 1} offsets, got {widths.numel()} and {vert_off.numel()}")
    xy, vert_off, heights, widths = xy.contiguous(), vert_off.contiguous(), heights.contiguous(), widths.contiguous()
    if capacity is None:
        ints = torch.cat([vert_off, heights, widths]).cpu().numpy()
        bounds = poly_host_bounds(xy.cpu().numpy(), ints[:n + 1], ints[n + 1:2 * n + 1], ints[2 * n + 1:])
        capacity = int(bounds.max()) + 1 if n else 1
    capacity = int(capacity)
    dev = xy.device
    num_runs = torch.empty(n, dtype=torch.int32, device=dev)
    num_keys = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(n, max(capacity, 0), dtype=torch.int32, device=dev)
    nbytes = int(lib.mrcnn_rle_from_poly_workspace_bytes(n, v))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _launch(lib.mrcnn_rle_from_poly_f64,
            (xy.data_ptr() if v else None, v, vert_off.data_ptr(), _ptr(heights) if n else None, _ptr(widths) if n else None, n,
             capacity, _ptr(num_runs) if n else None, _ptr(counts) if n else None, _ptr(num_keys) if n else None, ws.data_ptr(),
             nbytes, _stream()),
            lambda: (0, (n, v, capacity), 16 * v + 4 * counts.numel(), "rle_from_poly"))
    return num_runs, counts, num_keys


@_on_device
def rle_merge(num_runs: torch.Tensor, counts: torch.Tensor, group_off: torch.Tensor, intersect: bool = False,
              capacity: int | None = None):
    """maskUtils.merge (rleMerge of cocoapi/common/maskApi.c:49-70, the same bits) for G groups in one call on the GPU: group g is
    the union (intersect=False) or the intersection of rows [group_off[g], group_off[g+1]) of the table (num_runs int32 [N],
    counts [N,capacity_in]); group_off int32 [G+1] on the device. → (num_runs int32 [G], counts int32 [G,capacity]). An empty group
    has num_runs 0; a group with more runs than capacity reports its true num_runs and its row is not written; a group holding a
    row that was over its own capacity reports -1. capacity=None: one read of the group sizes, and the capacity is the longest
    group's total run count, which no result exceeds. Contract as for rle_iou: the rows of a group cover the same pixel count and
    only a leading run may be empty."""
    num_runs, counts = _rle_table((num_runs, counts), "rle_merge")
    _need_gpu(group_off)
    if group_off.dtype != torch.int32 or group_off.dim() != 1 or group_off.numel() < 1:
        raise RuntimeError(f"rle_merge: group_off must be an int32 [G+1] tensor, got {group_off.dtype} {tuple(group_off.shape)}")
    group_off = group_off.contiguous()
    n, g, dev = num_runs.size(0), group_off.numel() - 1, num_runs.device
    if capacity is None:
        nr, off = num_runs.cpu().numpy().astype(np.int64), group_off.cpu().numpy().astype(np.int64)
        if (off < 0).any() or (off > n).any() or (np.diff(off) < 0).any():
            raise RuntimeError(f"rle_merge: group_off must be non-decreasing within [0, {n}]")
        csum = np.concatenate([[0], np.cumsum(np.clip(nr, 0, counts.size(1)))])
        capacity = max(1, int((csum[off[1:]] - csum[off[:-1]]).max())) if g else 1
    capacity = int(capacity)
    out_runs = torch.empty(g, dtype=torch.int32, device=dev)
    out_counts = torch.empty(g, max(capacity, 0), dtype=torch.int32, device=dev)
    nbytes = int(lib.mrcnn_rle_merge_workspace_bytes(n, counts.size(1)))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _launch(lib.mrcnn_rle_merge,
            (_ptr(num_runs) if n else None, _ptr(counts) if n else None, n, counts.size(1), group_off.data_ptr(), g,
             1 if intersect else 0, capacity, _ptr(out_runs) if g else None, _ptr(out_counts) if g else None, ws.data_ptr(), nbytes,
             _stream()),
            lambda: (0, (n, g, capacity), 4 * (counts.numel() + out_counts.numel()), "rle_merge"))
    return out_runs, out_counts


_LIB.define("rle_from_poly(Tensor xy, Tensor vert_off, Tensor heights, Tensor widths, int? capacity=None) -> (Tensor, Tensor, Tensor)")
_LIB.impl("rle_from_poly", rle_from_poly, "CUDA")
_LIB.impl("rle_from_poly", lambda xy, *a: _need_gpu(xy), "CPU")
_LIB.define("rle_merge(Tensor num_runs, Tensor counts, Tensor group_off, bool intersect=False, int? capacity=None) -> (Tensor, Tensor)")
_LIB.impl("rle_merge", rle_merge, "CUDA")
_LIB.impl("rle_merge", lambda num_runs, *a: _need_gpu(num_runs), "CPU")


# --------------------------------------------------------------------------------------------------
# The COCO RLE codec on tables: rleFrString, rleToString, rleArea + rleToBbox, rleDecode (csrc/codec.hip)
# --------------------------------------------------------------------------------------------------
# status bits of rle_from_string (include/maskrcnn_hip.h): the first five refuse the row (num_runs = -1), the last two flag it
RLE_BAD_BYTE, RLE_LONG_TOKEN, RLE_OPEN_TOKEN, RLE_BAD_SIZE, RLE_BAD_OFFSETS = 1, 2, 4, 8, 64
RLE_EMPTY_RUN, RLE_PIXEL_SUM = 16, 32


def rle_string_tokens(data, str_off) -> np.ndarray:
    """Tokens (= runs) of every string of a packed HOST buffer — numpy uint8 [total] and offsets [n+1] — as int64 [n]: the
    characters with ((b - 48) & 0x20) == 0, counted with one cumulative sum read at the offsets. No Python loop per character or
    per string; this is how a front end finds the capacity for rle_from_string."""
    data = np.asarray(data, dtype=np.uint8).reshape(-1)
    off = np.asarray(str_off, dtype=np.int64).reshape(-1)
    ends = np.concatenate([[0], np.cumsum(((data.astype(np.int16) - 48) & 0x20) == 0, dtype=np.int64)])
    return ends[off[1:]] - ends[off[:-1]]


def _sizes(who, heights, widths, n: int):
    for name, t in (("heights", heights), ("widths", widths)):
        if t.dtype != torch.int32 or t.dim() != 1 or t.numel() != n:
            raise RuntimeError(f"{who}: {name} must be an int32 [{n}] tensor, got {t.dtype} {tuple(t.shape)}")
    return heights.contiguous(), widths.contiguous()


@_on_device
def rle_from_string(bytes: torch.Tensor, str_off: torch.Tensor, heights: torch.Tensor, widths: torch.Tensor,
                    capacity: int | None = None):
    """maskUtils.frPyObjects on compressed strings (rleFrString of cocoapi/common/maskApi.c:218-231, the same bits) for n strings
    in one call on the GPU. bytes uint8 [total] and str_off int64 [n+1]: string i is bytes[str_off[i]:str_off[i+1]], packed,
    no terminator; heights / widths int32 [n] serve the checks only. All device tensors. → (num_runs int32 [n], counts int32
    [n,capacity], status int32 [n]); the status bits are RLE_* above: a malformed string (a byte outside 48..111, a token of more
    than 6 characters, an end inside a token, a size outside [1, 16384]) reports num_runs = -1 and its row is not written; an
    empty run after the first and a wrong pixel sum are flagged and the row is written; a string with more runs than capacity
    reports its true num_runs and its row is not written (uninitialised memory here). capacity is required: the op never
    synchronises, and the characters it would have to count live on the device — a front end counts them on its host copy
    (rle_string_tokens)."""
    _need_gpu(bytes, str_off, heights, widths)
    if capacity is None:
        raise RuntimeError("rle_from_string: capacity is required (count the tokens on the host copy: ops.rle_string_tokens)")
    if bytes.dtype != torch.uint8 or bytes.dim() != 1:
        raise RuntimeError(f"rle_from_string: bytes must be a uint8 vector, got {bytes.dtype} {tuple(bytes.shape)}")
    if str_off.dtype != torch.int64 or str_off.dim() != 1 or str_off.numel() < 1:
        raise RuntimeError(f"rle_from_string: str_off must be an int64 [n+1] tensor, got {str_off.dtype} {tuple(str_off.shape)}")
    n = str_off.numel() - 1
    heights, widths = _sizes("rle_from_string", heights, widths, n)
    bytes, str_off = bytes.contiguous(), str_off.contiguous()
    capacity = int(capacity)
    dev = str_off.device
    num_runs = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(n, max(capacity, 0), dtype=torch.int32, device=dev)
    total = bytes.numel()
    _launch(lib.mrcnn_rle_from_string,
            (bytes.data_ptr() if total else None, total, str_off.data_ptr(), _ptr(heights) if n else None,
             _ptr(widths) if n else None, n, capacity, _ptr(num_runs) if n else None, _ptr(counts) if n else None,
             _ptr(status) if n else None, _stream()),
            lambda: (0, (n, total, capacity), total + 4 * counts.numel(), "rle_from_string"))
    return num_runs, counts, status


@_on_device
def rle_area_bbox(num_runs: torch.Tensor, counts: torch.Tensor, heights: torch.Tensor, widths: torch.Tensor):
    """maskUtils.area and maskUtils.toBbox (rleArea, rleToBbox of maskApi.c:72-75, :133-147, the same values) of every row of a
    table (num_runs int32 [N], counts [N,capacity]) with per-row heights / widths int32 [N] → (areas int32 [N], bboxes int32
    [N,4] as (x, y, w, h)): what rle_encode returns for dense masks. A row that was refused or is over its capacity gets -1s."""
    num_runs, counts = _rle_table((num_runs, counts), "rle_area_bbox")
    _need_gpu(heights, widths)
    n, dev = num_runs.size(0), num_runs.device
    heights, widths = _sizes("rle_area_bbox", heights, widths, n)
    areas = torch.empty(n, dtype=torch.int32, device=dev)
    bboxes = torch.empty(n, 4, dtype=torch.int32, device=dev)
    if n:
        _launch(lib.mrcnn_rle_area_bbox,
                (num_runs.data_ptr(), counts.data_ptr(), n, counts.size(1), heights.data_ptr(), widths.data_ptr(), areas.data_ptr(),
                 bboxes.data_ptr(), _stream()),
                lambda: (0, (n, counts.size(1), 1), 4 * counts.numel(), "rle_area_bbox"))
    return areas, bboxes


@_on_device
def rle_to_string(num_runs: torch.Tensor, counts: torch.Tensor, total_bytes: int | None = None):
    """rleToString (maskApi.c:204-216, the same characters) of every row of a table → (bytes uint8 [total_bytes], str_off int64
    [N+1]) on the device, packed: string i is bytes[str_off[i]:str_off[i+1]]. str_off always holds the true offsets. With
    total_bytes given the call never synchronises; rows that would cross the end of the buffer are not written (str_off[N] >
    total_bytes tells). total_bytes=None costs one host read of the scanned total and allocates exactly. A row that was refused
    or is over its capacity has an empty string."""
    num_runs, counts = _rle_table((num_runs, counts), "rle_to_string")
    n, dev = num_runs.size(0), num_runs.device
    str_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    nbytes = int(lib.mrcnn_rle_to_string_workspace_bytes(n))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    have = 0
    if total_bytes is None:
        _to_string_launch(num_runs, counts, None, 0, have, str_off, ws, nbytes)      # offsets only
        total_bytes, have = int(str_off[n]), 1                                     # the one host read; the write pass alone follows
    out = torch.empty(max(int(total_bytes), 0), dtype=torch.uint8, device=dev)
    _to_string_launch(num_runs, counts, out, 0, have, str_off, ws, nbytes)
    return out, str_off


def _to_string_launch(num_runs, counts, buf, row_stride, have_offsets, str_off, ws, nbytes):
    n = num_runs.size(0)
    _launch(lib.mrcnn_rle_to_string,
            (_ptr(num_runs) if n else None, _ptr(counts) if n else None, n, counts.size(1),
             buf.data_ptr() if buf is not None and buf.numel() else None, buf.numel() if buf is not None else 0, int(row_stride),
             int(have_offsets), str_off.data_ptr(), ws.data_ptr(), nbytes, _stream()),
            lambda: (0, (n, counts.size(1), 1), 4 * counts.numel(), "rle_to_string"))


@_on_device
def rle_to_string_rows(num_runs: torch.Tensor, counts: torch.Tensor, row_stride: int | None = None):
    """rle_to_string into the ENCODER's layout: → (strings uint8 [N,row_stride], string_bytes int32 [N]), row i holding its
    characters from column 0 (the rest zero) — what rle_encode returns, written by the kernel itself, no packed intermediate and
    no host synchronisation. row_stride defaults to 6*capacity (6 characters a run cover masks of up to 2^28 pixels). A row whose
    string is longer than row_stride, or that was refused or is over its capacity, has string_bytes 0 and an all-zero row."""
    num_runs, counts = _rle_table((num_runs, counts), "rle_to_string_rows")
    n, dev = num_runs.size(0), num_runs.device
    stride = 6 * counts.size(1) if row_stride is None else int(row_stride)
    if stride < 1:
        raise RuntimeError(f"rle_to_string_rows: row_stride={stride} must be >= 1")
    strings = torch.zeros(n, stride, dtype=torch.uint8, device=dev)
    str_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    nbytes = int(lib.mrcnn_rle_to_string_workspace_bytes(n))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _to_string_launch(num_runs, counts, strings, stride, 0, str_off, ws, nbytes)
    lengths = str_off[1:] - str_off[:-1]
    return strings, torch.where(lengths <= stride, lengths, torch.zeros_like(lengths)).to(torch.int32)


@_on_device
def rle_decode(num_runs: torch.Tensor, counts: torch.Tensor, height: int, width: int, out: torch.Tensor | None = None):
    """maskUtils.decode (rleDecode of maskApi.c:43-47) of every row of a table of H x W masks → uint8 [N,H,W] on the device,
    row-major, 0 / 1 — what rle_encode reads. `out`: a uint8 [N,H,W] tensor to fill (unit last stride, free image and row
    strides); every byte of it is written. Runs past H*W are clipped, pixels the runs do not reach are 0, and a row that was
    refused or is over its capacity decodes to zeros."""
    num_runs, counts = _rle_table((num_runs, counts), "rle_decode")
    n, dev = num_runs.size(0), num_runs.device
    h, w = int(height), int(width)
    if out is None:
        out = torch.empty(n, h, w, dtype=torch.uint8, device=dev)
    _need_gpu(out)
    if out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w) or (w > 1 and out.stride(2) != 1):
        raise RuntimeError(f"rle_decode: out must be a uint8 [{n},{h},{w}] tensor with unit last stride, got {out.dtype} "
                           f"{tuple(out.shape)} strides {tuple(out.stride())}")
    if n == 0:
        return out
    image_stride = out.stride(0) if n > 1 else 0
    row_stride = out.stride(1) if h > 1 else w
    nbytes = int(lib.mrcnn_rle_decode_workspace_bytes(n, counts.size(1)))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _launch(lib.mrcnn_rle_decode_u8,
            (num_runs.data_ptr(), counts.data_ptr(), n, counts.size(1), h, w, out.data_ptr(), image_stride, row_stride,
             ws.data_ptr(), nbytes, _stream()),
            lambda: (0, (n, h, w), n * h * w + 4 * counts.numel(), "rle_decode"))
    return out


_LIB.define("rle_from_string(Tensor bytes, Tensor str_off, Tensor heights, Tensor widths, int? capacity=None) -> (Tensor, Tensor, Tensor)")
_LIB.impl("rle_from_string", rle_from_string, "CUDA")
_LIB.impl("rle_from_string", lambda bytes, *a: _need_gpu(bytes), "CPU")
_LIB.define("rle_area_bbox(Tensor num_runs, Tensor counts, Tensor heights, Tensor widths) -> (Tensor, Tensor)")
_LIB.impl("rle_area_bbox", rle_area_bbox, "CUDA")
_LIB.impl("rle_area_bbox", lambda num_runs, *a: _need_gpu(num_runs), "CPU")
_LIB.define("rle_to_string(Tensor num_runs, Tensor counts, int? total_bytes=None) -> (Tensor, Tensor)")
_LIB.impl("rle_to_string", rle_to_string, "CUDA")
_LIB.impl("rle_to_string", lambda num_runs, *a: _need_gpu(num_runs), "CPU")
_LIB.define("rle_decode(Tensor num_runs, Tensor counts, int height, int width) -> Tensor")   # `out` is the Python binding's
_LIB.impl("rle_decode", lambda num_runs, counts, height, width: rle_decode(num_runs, counts, height, width), "CUDA")
_LIB.impl("rle_decode", lambda num_runs, *a: _need_gpu(num_runs), "CPU")


# --------------------------------------------------------------------------------------------------
# Rendering detections onto the image: data.blend_image without the labels (csrc/overlay.hip)
# --------------------------------------------------------------------------------------------------
@_on_device
def blend_instances(image: torch.Tensor, masks: torch.Tensor, colors: torch.Tensor, boxes: torch.Tensor | None = None,
                    threshold: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """data.blend_image (data.py:383-403: blend_mask per instance, then the rectangles) without the labels, the bits Pillow gives,
    in one launch (mrcnn_blend_instances_u8 in include/maskrcnn_hip.h states the rule). image uint8 [H,W,3] with unit strides
    inside a row (the row stride is free); masks uint8 or bool [N,H,W] with unit pixel stride (image and row strides free: a
    cropped or expanded view needs no copy), a pixel on where its byte > threshold; colors uint8 [N,3]; boxes int32 [N,4]
    (y1, x1, y2, x2) or None: no rectangles. → out, uint8 [H,W,3] on the device (a new tensor when none is given; `out is image`
    renders in place). N == 0 copies the image. No host synchronisation."""
    _need_gpu(image, masks, colors, boxes, out)
    if image.dtype != torch.uint8 or image.dim() != 3 or image.size(2) != 3:
        raise RuntimeError(f"blend_instances: expected an RGB uint8 [H,W,3] image, got {image.dtype} {tuple(image.shape)}")
    h, w = int(image.size(0)), int(image.size(1))
    if masks.dtype not in (torch.uint8, torch.bool) or masks.dim() != 3 or tuple(masks.shape[1:]) != (h, w):
        raise RuntimeError(f"blend_instances: expected uint8 or bool masks [N,{h},{w}], got {masks.dtype} {tuple(masks.shape)}")
    m = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
    n = int(m.size(0))
    if n > 0 and w > 1 and m.stride(2) != 1:
        raise RuntimeError(f"blend_instances: the masks' last stride must be 1, got strides {tuple(masks.stride())}")
    if out is None:
        out = torch.empty(h, w, 3, dtype=torch.uint8, device=image.device)
    for name, t in (("image", image), ("out", out)):
        if t.dtype != torch.uint8 or tuple(t.shape) != (h, w, 3) or t.stride(2) != 1 or (w > 1 and t.stride(1) != 3):
            raise RuntimeError(f"blend_instances: {name} must be a uint8 [{h},{w},3] tensor with unit strides inside a row, got "
                               f"{t.dtype} {tuple(t.shape)} strides {tuple(t.stride())}")
    if colors.dtype != torch.uint8 or tuple(colors.shape) != (n, 3):
        raise RuntimeError(f"blend_instances: colors must be uint8 [{n},3], got {colors.dtype} {tuple(colors.shape)}")
    colors = colors.contiguous()
    if boxes is not None:
        if boxes.dtype != torch.int32 or tuple(boxes.shape) != (n, 4):
            raise RuntimeError(f"blend_instances: boxes must be int32 [{n},4] or None, got {boxes.dtype} {tuple(boxes.shape)}")
        boxes = boxes.contiguous()
    row = lambda t: t.stride(0) if h > 1 else 3 * w
    _launch(lib.mrcnn_blend_instances_u8,
            (image.data_ptr(), row(image), m.data_ptr(), m.stride(0) if n > 1 else 0, m.stride(1) if n > 0 and h > 1 else w,
             colors.data_ptr(), _ptr(boxes), n, h, w, int(threshold), out.data_ptr(), row(out), _stream()),
            lambda: (0, (n, h, w), n * h * w + 6 * h * w, "blend_instances"))
    return out


_LIB.define("blend_instances(Tensor image, Tensor masks, Tensor colors, Tensor? boxes=None, int threshold=0) -> Tensor")   # `out` is the Python binding's
_LIB.impl("blend_instances", lambda image, masks, colors, boxes=None, threshold=0: blend_instances(image, masks, colors, boxes, threshold), "CUDA")
_LIB.impl("blend_instances", lambda image, *a: _need_gpu(image), "CPU")


# --------------------------------------------------------------------------------------------------
# RPN training targets: data.rpn_samples for a batch (csrc/targets.hip)
# --------------------------------------------------------------------------------------------------
def _target_anchors(who, anchors):
    _need_gpu(anchors)
    if anchors.dtype != torch.float64 or anchors.dim() != 2 or anchors.size(1) != 4 or anchors.size(0) < 1:
        raise RuntimeError(f"{who}: anchors must be float64 [A,4] with A >= 1 (anchors.pyramid_anchors(cfg, dtype=torch.float64)), "
                           f"got {anchors.dtype} {tuple(anchors.shape)}")
    return anchors.contiguous()


def _target_rows(who, gt_boxes, gt_off):
    _need_gpu(gt_boxes, gt_off)
    if gt_boxes.dtype != torch.float32 or gt_boxes.dim() != 2 or gt_boxes.size(1) != 4:
        raise RuntimeError(f"{who}: gt_boxes must be float32 [M,4], got {gt_boxes.dtype} {tuple(gt_boxes.shape)}")
    if gt_off.dtype != torch.int32 or gt_off.dim() != 1 or gt_off.numel() < 2:
        raise RuntimeError(f"{who}: gt_off must be int32 [B+1] with B >= 1, got {gt_off.dtype} {tuple(gt_off.shape)}")
    return gt_boxes.contiguous(), gt_off.contiguous()


def _target_ids(who, gt_class_ids, m: int):
    _need_gpu(gt_class_ids)
    if gt_class_ids.dtype != torch.int32 or tuple(gt_class_ids.shape) != (m,):
        raise RuntimeError(f"{who}: gt_class_ids must be int32 [{m}], got {gt_class_ids.dtype} {tuple(gt_class_ids.shape)}")
    return gt_class_ids.contiguous()


def _target_std(who, std_dev):
    std = [float(v) for v in std_dev]
    if len(std) != 4:
        raise RuntimeError(f"{who}: std_dev must hold 4 numbers, got {len(std)}")
    return std


def _ptr_if(m: int, t):
    """The pointer of a tensor of the m packed rows: none where there is no row (a null pointer is what the library expects then)."""
    return t.data_ptr() if m else None


def _target_map(who, name, t, dtype, b: int, a: int):
    _need_gpu(t)
    if t.dtype != dtype or tuple(t.shape) != (b, a):
        raise RuntimeError(f"{who}: {name} must be {dtype} [{b},{a}], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def _workspace(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


@_on_device
def anchor_match(anchors: torch.Tensor, gt_boxes: torch.Tensor, gt_class_ids: torch.Tensor, gt_off: torch.Tensor,
                 neg_iou: float = 0.3, pos_iou: float = 0.7, crowd_iou: float = 0.001):
    """Steps 1-6 of data.rpn_samples (data.py:485-540; the rule is stated at mrcnn_anchor_match in include/maskrcnn_hip.h) for B
    images: anchors float64 [A,4], ground truth packed as gt_boxes float32 [M,4], gt_class_ids int32 [M], gt_off int32 [B+1] →
    (match int32 [B,A] of -1 / 0 / 1, iou_argmax int32 [B,A] (row position within the image), iou_max float32 [B,A], gt_argmax
    int32 [M] (-1: crowd or dropped row), status int32 [B] (bit 0: no kept row in the image)). The thresholds are narrowed to
    fp32. No host synchronisation."""
    who = "anchor_match"
    anchors = _target_anchors(who, anchors)
    gt_boxes, gt_off = _target_rows(who, gt_boxes, gt_off)
    m, a, b, dev = gt_boxes.size(0), anchors.size(0), gt_off.numel() - 1, anchors.device
    gt_class_ids = _target_ids(who, gt_class_ids, m)
    match = torch.empty(b, a, dtype=torch.int32, device=dev)
    iou_argmax = torch.empty(b, a, dtype=torch.int32, device=dev)
    iou_max = torch.empty(b, a, dtype=torch.float32, device=dev)
    gt_argmax = torch.empty(m, dtype=torch.int32, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    nbytes = int(lib.mrcnn_anchor_match_workspace_bytes(m))
    ws = _workspace(nbytes, dev)
    _launch(lib.mrcnn_anchor_match,
            (anchors.data_ptr(), a, _ptr_if(m, gt_boxes), _ptr_if(m, gt_class_ids), gt_off.data_ptr(), m, b,
             float(neg_iou), float(pos_iou), float(crowd_iou), match.data_ptr(), iou_argmax.data_ptr(), iou_max.data_ptr(),
             _ptr_if(m, gt_argmax), status.data_ptr(), ws.data_ptr(), nbytes, _stream()),
            lambda: (0, (b, a, m), 32 * a + 12 * b * a, "anchor_match"))
    return match, iou_argmax, iou_max, gt_argmax, status


@_on_device
def sample_by_key(match: torch.Tensor, keys: torch.Tensor, count: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """Steps 7-8 of data.rpn_samples (data.py:542-557) for match int32 [B,A]: of an image's positives the count // 2 with the
    smallest (key, anchor index) stay positive, then of its negatives the count - (positives left) with the smallest stay
    negative; the others become 0. keys int32 [B,A], non-negative (the caller's stand-in for np.random.choice: independent
    uniform keys draw from the same distribution). → out int32 [B,A] (a new tensor when none is given; `out is match` works in
    place). No host synchronisation."""
    who = "sample_by_key"
    _need_gpu(match, keys, out)
    if match.dtype != torch.int32 or match.dim() != 2 or match.size(0) < 1 or match.size(1) < 1:
        raise RuntimeError(f"{who}: match must be int32 [B,A] with B, A >= 1, got {match.dtype} {tuple(match.shape)}")
    b, a = match.shape
    same = out is match
    match = _target_map(who, "match", match, torch.int32, b, a)
    keys = _target_map(who, "keys", keys, torch.int32, b, a)
    if out is None:
        out = torch.empty(b, a, dtype=torch.int32, device=match.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (b, a) or not out.is_contiguous():
        raise RuntimeError(f"{who}: out must be a contiguous int32 [{b},{a}] tensor, got {out.dtype} {tuple(out.shape)} strides "
                           f"{tuple(out.stride())}")
    if same:
        match = out
    nbytes = int(lib.mrcnn_sample_by_key_workspace_bytes(b))
    ws = _workspace(nbytes, match.device)
    _launch(lib.mrcnn_sample_by_key,
            (match.data_ptr(), keys.data_ptr(), b, a, int(count), out.data_ptr(), ws.data_ptr(), nbytes, _stream()),
            lambda: (0, (b, a, int(count)), 8 * 8 * b * a, "sample_by_key"))
    return out


@_on_device
def rpn_deltas(anchors: torch.Tensor, gt_boxes: torch.Tensor, gt_off: torch.Tensor, match: torch.Tensor, iou_argmax: torch.Tensor,
               count: int, std_dev=(0.1, 0.1, 0.2, 0.2)):
    """Step 9 of data.rpn_samples (data.py:559-589): the regression deltas of an image's positives (match == 1) in ascending
    anchor index against row iou_argmax of the image, divided by std_dev (four host numbers, used as fp64) and narrowed to fp32,
    with the reference's NumPy >= 2 promotion (mrcnn_rpn_deltas in include/maskrcnn_hip.h) → (rpn_bbox float32 [B,count,4], rows
    past the positives 0; num_pos int32 [B]). Positives beyond `count` are counted, not written. No host synchronisation."""
    who = "rpn_deltas"
    anchors = _target_anchors(who, anchors)
    gt_boxes, gt_off = _target_rows(who, gt_boxes, gt_off)
    m, a, b, dev = gt_boxes.size(0), anchors.size(0), gt_off.numel() - 1, anchors.device
    match = _target_map(who, "match", match, torch.int32, b, a)
    iou_argmax = _target_map(who, "iou_argmax", iou_argmax, torch.int32, b, a)
    count = int(count)
    std = _target_std(who, std_dev)
    rpn_bbox = torch.empty(b, max(count, 0), 4, dtype=torch.float32, device=dev)
    num_pos = torch.empty(b, dtype=torch.int32, device=dev)
    nbytes = int(lib.mrcnn_rpn_deltas_workspace_bytes(b, a))
    ws = _workspace(nbytes, dev)
    _launch(lib.mrcnn_rpn_deltas,
            (anchors.data_ptr(), a, _ptr_if(m, gt_boxes), gt_off.data_ptr(), m, b, match.data_ptr(), iou_argmax.data_ptr(),
             count, (ctypes.c_double * 4)(*std), rpn_bbox.data_ptr() if count > 0 else None, num_pos.data_ptr(), ws.data_ptr(),
             nbytes, _stream()),
            lambda: (0, (b, a, count), 2 * 4 * b * a + 16 * b * count, "rpn_deltas"))
    return rpn_bbox, num_pos


_LIB.define("anchor_match(Tensor anchors, Tensor gt_boxes, Tensor gt_class_ids, Tensor gt_off, float neg_iou=0.3, float pos_iou=0.7, "
            "float crowd_iou=0.001) -> (Tensor, Tensor, Tensor, Tensor, Tensor)")
_LIB.impl("anchor_match", anchor_match, "CUDA")
_LIB.impl("anchor_match", lambda anchors, *a: _need_gpu(anchors), "CPU")
_LIB.define("sample_by_key(Tensor match, Tensor keys, int count) -> Tensor")   # `out` is the Python binding's
_LIB.impl("sample_by_key", lambda match, keys, count: sample_by_key(match, keys, count), "CUDA")
_LIB.impl("sample_by_key", lambda match, *a: _need_gpu(match), "CPU")
_LIB.define("rpn_deltas(Tensor anchors, Tensor gt_boxes, Tensor gt_off, Tensor match, Tensor iou_argmax, int count, "
            "float[] std_dev) -> (Tensor, Tensor)")
_LIB.impl("rpn_deltas", rpn_deltas, "CUDA")
_LIB.impl("rpn_deltas", lambda anchors, *a: _need_gpu(anchors), "CPU")


# --------------------------------------------------------------------------------------------------
# Detection training targets: model.mrn_samples for a batch (csrc/detection_targets.hip)
# --------------------------------------------------------------------------------------------------
def _target_out(who, name, t, dtype, shape, dev):
    """A caller's output tensor, checked — or a new one."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    _need_gpu(t)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != dev:
        raise RuntimeError(f"{who}: out tensor {name} must be a contiguous {dtype} {list(shape)} tensor on {dev}, got {t.dtype} "
                           f"{tuple(t.shape)} strides {tuple(t.stride())} on {t.device}")
    return t


@_on_device
def detection_targets(rois: torch.Tensor, gt_boxes: torch.Tensor, gt_class_ids: torch.Tensor, gt_off: torch.Tensor,
                      keys: torch.Tensor, count: int = 100, positive_ratio: float = 0.33, std_dev=(0.1, 0.1, 0.2, 0.2),
                      pos_iou: float = 0.5, crowd_iou: float = 0.001, out=None):
    """Steps 1-6 of model.mrn_samples (model.py:396-576; the rule is stated at mrcnn_detection_targets in include/maskrcnn_hip.h)
    for B images: rois float32 [B,N,4], ground truth packed as gt_boxes float32 [M,4], gt_class_ids int32 [M], gt_off int32 [B+1],
    keys int32 [B,N] (non-negative: the stand-in for torch.randperm, as in sample_by_key) →
    (rois_out float32 [B,count,4], target_class_ids int32 [B,count], target_deltas float32 [B,count,4], roi_index int32 [B,count],
    gt_index int32 [B,count], num_pos int32 [B], num_neg int32 [B], status int32 [B] (bit 0: no kept row in the image)).
    The positives come first, then the negatives, each by ascending (key, roi index); rows past num_pos + num_neg are 0 / -1.
    std_dev: four host numbers, narrowed to fp32, as are the thresholds. out: the eight tensors to write into. One launch, no
    host synchronisation."""
    who = "detection_targets"
    _need_gpu(rois, gt_class_ids, keys)
    if rois.dtype != torch.float32 or rois.dim() != 3 or rois.size(2) != 4 or rois.size(0) < 1 or rois.size(1) < 1:
        raise RuntimeError(f"{who}: rois must be float32 [B,N,4] with B, N >= 1, got {rois.dtype} {tuple(rois.shape)}")
    gt_boxes, gt_off = _target_rows(who, gt_boxes, gt_off)
    b, n, m, dev = rois.size(0), rois.size(1), gt_boxes.size(0), rois.device
    if gt_off.numel() != b + 1:
        raise RuntimeError(f"{who}: gt_off must be int32 [{b + 1}] for {b} images of rois, got {tuple(gt_off.shape)}")
    rois, gt_class_ids = rois.contiguous(), _target_ids(who, gt_class_ids, m)
    keys = _target_map(who, "keys", keys, torch.int32, b, n)
    count = int(count)
    std = _target_std(who, std_dev)
    c = max(count, 0)
    spec = (("rois_out", torch.float32, (b, c, 4)), ("target_class_ids", torch.int32, (b, c)), ("target_deltas", torch.float32, (b, c, 4)),
            ("roi_index", torch.int32, (b, c)), ("gt_index", torch.int32, (b, c)), ("num_pos", torch.int32, (b,)),
            ("num_neg", torch.int32, (b,)), ("status", torch.int32, (b,)))
    if out is not None and len(out) != len(spec):
        raise RuntimeError(f"{who}: out must hold {len(spec)} tensors ({', '.join(s[0] for s in spec)}), got {len(out)}")
    outs = tuple(_target_out(who, name, None if out is None else out[i], dtype, shape, dev) for i, (name, dtype, shape) in enumerate(spec))
    _launch(lib.mrcnn_detection_targets,
            (rois.data_ptr(), _ptr_if(m, gt_boxes), _ptr_if(m, gt_class_ids), gt_off.data_ptr(), keys.data_ptr(),
             b, n, m, count, float(positive_ratio), float(pos_iou), float(crowd_iou), (ctypes.c_float * 4)(*std),
             *[t.data_ptr() if t.numel() else None for t in outs], _stream()),
            lambda: (0, (b, n, m), 20 * b * n + 20 * m + 44 * b * c, "detection_targets"))
    return outs


@_on_device
def mask_targets(gt_masks: torch.Tensor, gt_off: torch.Tensor, rois_out: torch.Tensor, gt_index: torch.Tensor,
                 num_pos: torch.Tensor, mask_shape=(28, 28), out: torch.Tensor | None = None) -> torch.Tensor:
    """Step 7 of model.mrn_samples (model.py:491-507): for slot s < num_pos[b] of image b, CropFunction(mh, mw, 0) of mask row
    gt_off[b] + gt_index[b,s] with box rois_out[b,s], then torch.round; zeros for every other slot → target_mask float32
    [B,count,mh,mw]. gt_masks [M,H,W] uint8 / bool (the byte's value as a float) or float32, read in place through the index.
    rois_out float32 [B,count,4], gt_index int32 [B,count], num_pos int32 [B] as detection_targets returns them. One launch, no
    host synchronisation."""
    who = "mask_targets"
    _need_gpu(gt_masks, gt_off, rois_out, gt_index, num_pos)
    if gt_masks.dtype not in (torch.uint8, torch.bool, torch.float32) or gt_masks.dim() != 3:
        raise RuntimeError(f"{who}: gt_masks must be uint8, bool or float32 [M,H,W], got {gt_masks.dtype} {tuple(gt_masks.shape)}")
    if rois_out.dtype != torch.float32 or rois_out.dim() != 3 or rois_out.size(2) != 4 or rois_out.size(0) < 1:
        raise RuntimeError(f"{who}: rois_out must be float32 [B,count,4], got {rois_out.dtype} {tuple(rois_out.shape)}")
    b, count, dev = rois_out.size(0), rois_out.size(1), rois_out.device
    if gt_off.dtype != torch.int32 or tuple(gt_off.shape) != (b + 1,):
        raise RuntimeError(f"{who}: gt_off must be int32 [{b + 1}], got {gt_off.dtype} {tuple(gt_off.shape)}")
    gt_index = _target_map(who, "gt_index", gt_index, torch.int32, b, count)
    if num_pos.dtype != torch.int32 or tuple(num_pos.shape) != (b,):
        raise RuntimeError(f"{who}: num_pos must be int32 [{b}], got {num_pos.dtype} {tuple(num_pos.shape)}")
    if len(mask_shape) != 2:
        raise RuntimeError(f"{who}: mask_shape must be (height, width), got {tuple(mask_shape)}")
    mh, mw = int(mask_shape[0]), int(mask_shape[1])
    gt_masks, gt_off, rois_out, num_pos = gt_masks.contiguous(), gt_off.contiguous(), rois_out.contiguous(), num_pos.contiguous()
    m, h, w = gt_masks.shape
    out = _target_out(who, "target_mask", out, torch.float32, (b, count, max(mh, 0), max(mw, 0)), dev)
    fn = lib.mrcnn_mask_targets_f32 if gt_masks.dtype == torch.float32 else lib.mrcnn_mask_targets_u8
    _launch(fn, (gt_masks.data_ptr() if gt_masks.numel() else None, m, h, w, gt_off.data_ptr(), b, count, _ptr(rois_out) if count else None,
                 _ptr(gt_index) if count else None, num_pos.data_ptr(), mh, mw, out.data_ptr() if out.numel() else None, _stream()),
            lambda: (0, (b, count, mh * mw), 4 * b * count * mh * mw, "mask_targets"))
    return out


_LIB.define("detection_targets(Tensor rois, Tensor gt_boxes, Tensor gt_class_ids, Tensor gt_off, Tensor keys, int count=100, "
            "float positive_ratio=0.33, float[] std_dev=[0.1, 0.1, 0.2, 0.2], float pos_iou=0.5, float crowd_iou=0.001) -> "
            "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")   # `out` is the Python binding's
_LIB.impl("detection_targets", lambda *a, **k: detection_targets(*a, **k), "CUDA")
_LIB.impl("detection_targets", lambda rois, *a, **k: _need_gpu(rois), "CPU")
_LIB.define("mask_targets(Tensor gt_masks, Tensor gt_off, Tensor rois_out, Tensor gt_index, Tensor num_pos, "
            "int[] mask_shape=[28, 28]) -> Tensor")
_LIB.impl("mask_targets", lambda *a, **k: mask_targets(*a, **k), "CUDA")
_LIB.impl("mask_targets", lambda gt_masks, *a, **k: _need_gpu(gt_masks), "CPU")


# --------------------------------------------------------------------------------------------------
# Training losses: the reference's five loss functions for a batch, forward and backward (csrc/losses.hip)
# --------------------------------------------------------------------------------------------------
def _loss_input(who, name, t, dtype, shape):
    """A contiguous tensor of this dtype and shape whose first byte is 16-byte aligned (the kernels read float4 rows)."""
    _need_gpu(t)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{who}: {name} must be {dtype} {list(shape)}, got {t.dtype} {tuple(t.shape)}")
    t = t.detach().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _rpn_loss_inputs(who, match, logits, pred_bbox, target_bbox):
    _need_gpu(match, logits, pred_bbox, target_bbox)
    if match.dtype != torch.int32 or match.dim() != 2 or match.size(0) < 1 or match.size(1) < 1:
        raise RuntimeError(f"{who}: match must be int32 [B,A] with B, A >= 1, got {match.dtype} {tuple(match.shape)}")
    b, a = match.shape
    if target_bbox.dim() != 3 or target_bbox.size(1) < 1:
        raise RuntimeError(f"{who}: target_bbox must be float32 [{b},count,4] with count >= 1, got {tuple(target_bbox.shape)}")
    count = target_bbox.size(1)
    return (_loss_input(who, "match", match, torch.int32, (b, a)), _loss_input(who, "logits", logits, torch.float32, (b, a, 2)),
            _loss_input(who, "pred_bbox", pred_bbox, torch.float32, (b, a, 4)),
            _loss_input(who, "target_bbox", target_bbox, torch.float32, (b, count, 4)), b, a, count)


def _loss_grad_out(who, grad_out, counts, losses: int):
    """grad_out float32 [losses] (the batch's mean) or [B,losses] (per image) → (grad_out, counts, per_image)."""
    b = counts.size(0)
    _need_gpu(grad_out, counts)
    if counts.dtype != torch.int32 or tuple(counts.shape) != (b, losses):
        raise RuntimeError(f"{who}: counts must be int32 [B,{losses}] as the forward returned them, got {counts.dtype} {tuple(counts.shape)}")
    if grad_out.dtype != torch.float32 or tuple(grad_out.shape) not in ((losses,), (b, losses)):
        raise RuntimeError(f"{who}: grad_out must be float32 [{losses}] or [{b},{losses}], got {grad_out.dtype} {tuple(grad_out.shape)}")
    return grad_out.contiguous(), counts.contiguous(), grad_out.dim() == 2


@_on_device
def rpn_loss(match: torch.Tensor, logits: torch.Tensor, pred_bbox: torch.Tensor, target_bbox: torch.Tensor):
    """RPN.class_loss and RPN.boxes_loss (model.py:652-718) for B images; the rule is stated at mrcnn_rpn_loss_forward in
    include/maskrcnn_hip.h. match int32 [B,A] of -1 / 0 / 1, logits float32 [B,A,2], pred_bbox float32 [B,A,4], target_bbox float32
    [B,count,4] as rpn_deltas wrote it → (sums float64 [B,2]: the class and box terms of each image, counts int32 [B,2]: the
    anchors with match != 0 and 4 x the positives that have a target row, status int32 [B]: bit 0 = more than count positives,
    chunk_pos int32 [B,chunks]: what rpn_loss_backward ranks the positives by). A loss is sums / counts, over the batch or per
    image. Two launches, no host synchronisation."""
    who = "rpn_loss"
    match, logits, pred_bbox, target_bbox, b, a, count = _rpn_loss_inputs(who, match, logits, pred_bbox, target_bbox)
    dev = match.device
    sums = torch.empty(b, 2, dtype=torch.float64, device=dev)
    counts = torch.empty(b, 2, dtype=torch.int32, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    chunk_pos = torch.empty(b, max(int(lib.mrcnn_rpn_loss_chunks(a)), 1), dtype=torch.int32, device=dev)
    nbytes = int(lib.mrcnn_rpn_loss_workspace_bytes(b, a, count))
    ws = _workspace(nbytes, dev)
    _launch(lib.mrcnn_rpn_loss_forward,
            (match.data_ptr(), logits.data_ptr(), pred_bbox.data_ptr(), target_bbox.data_ptr(), b, a, count, sums.data_ptr(),
             counts.data_ptr(), status.data_ptr(), chunk_pos.data_ptr(), ws.data_ptr(), nbytes, _stream()),
            lambda: (0, (b, a, count), 4 * b * a + 56 * b * count, "rpn_loss"))
    return sums, counts, status, chunk_pos


@_on_device
def rpn_loss_backward(match: torch.Tensor, logits: torch.Tensor, pred_bbox: torch.Tensor, target_bbox: torch.Tensor,
                      chunk_pos: torch.Tensor, counts: torch.Tensor, grad_out: torch.Tensor):
    """The gradients of rpn_loss's two losses → (grad_logits float32 [B,A,2], grad_bbox float32 [B,A,4]), every element written,
    +0 where an anchor does not contribute. counts and chunk_pos as rpn_loss returned them; grad_out float32 [2]: the upstream
    gradients of (class loss, box loss) = batch sums / batch counts, or [B,2]: of each image's own sums / counts. One launch, no
    host synchronisation."""
    who = "rpn_loss_backward"
    match, logits, pred_bbox, target_bbox, b, a, count = _rpn_loss_inputs(who, match, logits, pred_bbox, target_bbox)
    chunk_pos = _loss_input(who, "chunk_pos", chunk_pos, torch.int32, (b, max(int(lib.mrcnn_rpn_loss_chunks(a)), 1)))
    grad_out, counts, per_image = _loss_grad_out(who, grad_out, counts, 2)
    grad_logits, grad_bbox = torch.empty_like(logits), torch.empty_like(pred_bbox)
    _launch(lib.mrcnn_rpn_loss_backward,
            (match.data_ptr(), logits.data_ptr(), pred_bbox.data_ptr(), target_bbox.data_ptr(), chunk_pos.data_ptr(),
             counts.data_ptr(), grad_out.data_ptr(), int(per_image), b, a, count, grad_logits.data_ptr(), grad_bbox.data_ptr(),
             _stream()),
            lambda: (0, (b, a, count), 28 * b * a, "rpn_loss_backward"))
    return grad_logits, grad_bbox


def _head_loss_inputs(who, target_class_ids, num_rois, target_deltas, target_mask, logits, pred_bbox, pred_masks):
    _need_gpu(target_class_ids, num_rois, target_deltas, target_mask, logits, pred_bbox, pred_masks)
    if target_class_ids.dtype != torch.int32 or target_class_ids.dim() != 2 or target_class_ids.size(0) < 1 or target_class_ids.size(1) < 1:
        raise RuntimeError(f"{who}: target_class_ids must be int32 [B,count] with B, count >= 1, got {target_class_ids.dtype} "
                           f"{tuple(target_class_ids.shape)}")
    b, count = target_class_ids.shape
    if target_mask.dim() != 4 or logits.dim() != 3 or logits.size(2) < 1:
        raise RuntimeError(f"{who}: target_mask must be float32 [{b},{count},mh,mw] and logits float32 [{b},{count},C], got "
                           f"{tuple(target_mask.shape)} and {tuple(logits.shape)}")
    c, mh, mw = logits.size(2), target_mask.size(2), target_mask.size(3)
    return (_loss_input(who, "target_class_ids", target_class_ids, torch.int32, (b, count)),
            _loss_input(who, "num_rois", num_rois, torch.int32, (b,)),
            _loss_input(who, "target_deltas", target_deltas, torch.float32, (b, count, 4)),
            _loss_input(who, "target_mask", target_mask, torch.float32, (b, count, mh, mw)),
            _loss_input(who, "logits", logits, torch.float32, (b, count, c)),
            _loss_input(who, "pred_bbox", pred_bbox, torch.float32, (b, count, c, 4)),
            _loss_input(who, "pred_masks", pred_masks, torch.float32, (b, count, c, mh, mw)), b, count, c, mh, mw)


@_on_device
def head_loss(target_class_ids: torch.Tensor, num_rois: torch.Tensor, target_deltas: torch.Tensor, target_mask: torch.Tensor,
              logits: torch.Tensor, pred_bbox: torch.Tensor, pred_masks: torch.Tensor):
    """Classifier.class_loss, Classifier.boxes_loss and Mask.mask_loss (model.py:802-845, 922-953) for B images on the padded outputs
    of detection_targets; the rule is stated at mrcnn_rpn_loss_forward in include/maskrcnn_hip.h. target_class_ids int32 [B,count],
    num_rois int32 [B] (num_pos + num_neg: the slots past it never contribute), target_deltas float32 [B,count,4], target_mask
    float32 [B,count,mh,mw], logits float32 [B,count,C], pred_bbox float32 [B,count,C,4], pred_masks float32 [B,count,C,mh,mw] →
    (sums float64 [B,3]: class, box, mask; counts int32 [B,3]: the slots, 4 x the positive slots, mh x mw x the positive slots;
    status int32 [B]: bit 1 = a class id outside 0 .. C-1, whose slot is skipped). Two launches, no host synchronisation."""
    who = "head_loss"
    ids, num_rois, deltas, mask, logits, pred_bbox, pred_masks, b, count, c, mh, mw = _head_loss_inputs(
        who, target_class_ids, num_rois, target_deltas, target_mask, logits, pred_bbox, pred_masks)
    dev = ids.device
    sums = torch.empty(b, 3, dtype=torch.float64, device=dev)
    counts = torch.empty(b, 3, dtype=torch.int32, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    nbytes = int(lib.mrcnn_head_loss_workspace_bytes(b, count))
    ws = _workspace(nbytes, dev)
    _launch(lib.mrcnn_head_loss_forward,
            (ids.data_ptr(), num_rois.data_ptr(), deltas.data_ptr(), mask.data_ptr(), logits.data_ptr(), pred_bbox.data_ptr(),
             pred_masks.data_ptr(), b, count, c, mh, mw, sums.data_ptr(), counts.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes,
             _stream()),
            lambda: (0, (b, count, c), 4 * b * count * (c + 2 * mh * mw + 10), "head_loss"))
    return sums, counts, status


@_on_device
def head_loss_backward(target_class_ids: torch.Tensor, num_rois: torch.Tensor, target_deltas: torch.Tensor, target_mask: torch.Tensor,
                       logits: torch.Tensor, pred_bbox: torch.Tensor, pred_masks: torch.Tensor, counts: torch.Tensor,
                       grad_out: torch.Tensor):
    """The gradients of head_loss's three losses → (grad_logits, grad_bbox, grad_masks) in the predictions' shapes, every element
    written: zeros but the contributing slots' logits rows, their class's box row and their class's mask plane. counts as
    head_loss returned them; grad_out float32 [3] (batch mean) or [B,3] (per image), as for rpn_loss_backward. One launch, no host
    synchronisation."""
    who = "head_loss_backward"
    ids, num_rois, deltas, mask, logits, pred_bbox, pred_masks, b, count, c, mh, mw = _head_loss_inputs(
        who, target_class_ids, num_rois, target_deltas, target_mask, logits, pred_bbox, pred_masks)
    grad_out, counts, per_image = _loss_grad_out(who, grad_out, counts, 3)
    grad_logits, grad_bbox, grad_masks = torch.empty_like(logits), torch.empty_like(pred_bbox), torch.empty_like(pred_masks)
    _launch(lib.mrcnn_head_loss_backward,
            (ids.data_ptr(), num_rois.data_ptr(), deltas.data_ptr(), mask.data_ptr(), logits.data_ptr(), pred_bbox.data_ptr(),
             pred_masks.data_ptr(), counts.data_ptr(), grad_out.data_ptr(), int(per_image), b, count, c, mh, mw,
             grad_logits.data_ptr(), grad_bbox.data_ptr(), grad_masks.data_ptr(), _stream()),
            lambda: (0, (b, count, c), 4 * b * count * c * (mh * mw + 5), "head_loss_backward"))
    return grad_logits, grad_bbox, grad_masks


_LIB.define("rpn_loss(Tensor match, Tensor logits, Tensor pred_bbox, Tensor target_bbox) -> (Tensor, Tensor, Tensor, Tensor)")
_LIB.impl("rpn_loss", rpn_loss, "CUDA")
_LIB.impl("rpn_loss", lambda match, *a: _need_gpu(match), "CPU")
_LIB.define("rpn_loss_backward(Tensor match, Tensor logits, Tensor pred_bbox, Tensor target_bbox, Tensor chunk_pos, Tensor counts, "
            "Tensor grad_out) -> (Tensor, Tensor)")
_LIB.impl("rpn_loss_backward", rpn_loss_backward, "CUDA")
_LIB.impl("rpn_loss_backward", lambda match, *a: _need_gpu(match), "CPU")
_LIB.define("head_loss(Tensor target_class_ids, Tensor num_rois, Tensor target_deltas, Tensor target_mask, Tensor logits, "
            "Tensor pred_bbox, Tensor pred_masks) -> (Tensor, Tensor, Tensor)")
_LIB.impl("head_loss", head_loss, "CUDA")
_LIB.impl("head_loss", lambda ids, *a: _need_gpu(ids), "CPU")
_LIB.define("head_loss_backward(Tensor target_class_ids, Tensor num_rois, Tensor target_deltas, Tensor target_mask, Tensor logits, "
            "Tensor pred_bbox, Tensor pred_masks, Tensor counts, Tensor grad_out) -> (Tensor, Tensor, Tensor)")
_LIB.impl("head_loss_backward", head_loss_backward, "CUDA")
_LIB.impl("head_loss_backward", lambda ids, *a: _need_gpu(ids), "CPU")


# --------------------------------------------------------------------------------------------------
# Winograd F(2x2,3x3) 3x3 stride-1 SAME conv (csrc/conv_wino.hip)
# --------------------------------------------------------------------------------------------------
def winograd_set_spatial(on: int) -> None:
    """Process-wide tuning switch: 1 = spatial-tile Winograd kernel on large maps (default), 0 = linear-tile kernel
    everywhere, -1 = default / MRCNN_WINO_SPATIAL. Results are bit-identical either way."""
    check(lib.mrcnn_winograd_set_spatial(int(on)))


@_on_device
def winograd_weights(w_ohwi: torch.Tensor) -> torch.Tensor:
    """[Cout,3,3,Cin] fp32 → the transformed filter G g G^T (evaluated in double), 16*Cout*Cin floats in the
    kernel's k-blocked order [Cin/8][16][Cout][8] (returned with the logical shape [16,Cout,Cin])."""
    _need_gpu(w_ohwi)
    assert w_ohwi.dtype == torch.float32 and w_ohwi.is_contiguous() and tuple(w_ohwi.shape[1:3]) == (3, 3)
    cout, cin = w_ohwi.size(0), w_ohwi.size(3)
    u = torch.empty(16, cout, cin, dtype=torch.float32, device=w_ohwi.device)
    check(lib.mrcnn_winograd_weights_f32(w_ohwi.data_ptr(), cout, cin, u.data_ptr(), _stream()))
    return u


@_on_device
def nhwc_to_kblocked(x: torch.Tensor) -> torch.Tensor:
    """[B,H,W,C] → [C/8,B,H,W,8]."""
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.size(3) % 8 == 0
    b, h, w, c = x.shape
    y = torch.empty(c // 8, b, h, w, 8, dtype=torch.float32, device=x.device)
    check(lib.mrcnn_nhwc_to_kblocked_f32(x.data_ptr(), b * h * w, c, y.data_ptr(), _stream()))
    return y


@_on_device
def conv3x3_winograd(x: torch.Tensor, u: torch.Tensor, scale, shift, relu: bool = False, algo_cin=None,
                     out: str = "nhwc"):
    """relu(conv3x3_same(x) * scale + shift) with u from winograd_weights.
    x: NHWC fp32 [B,H,W,Cin] or k-blocked [Cin/8,B,H,W,8] (H, W even; Cin % 8 == 0).
    out: "nhwc" → [B,H,W,Cout]; "kblocked" → [Cout/8,B,H,W,8] (feeds the next Winograd conv without a transposition
    pass); "both" → (nhwc, kblocked)."""
    _need_gpu(x, u, scale, shift)
    assert x.dtype == torch.float32 and x.is_contiguous() and u.is_contiguous() and out in ("nhwc", "kblocked", "both")
    if x.dim() == 5:
        layout = 1
        g, b, h, w, _ = x.shape
        cin = g * 8
    else:
        layout = 0
        b, h, w, cin = x.shape
    cout = u.size(1)
    assert u.size(2) == cin
    y = torch.empty(b, h, w, cout, dtype=torch.float32, device=x.device) if out != "kblocked" else None
    yk = torch.empty(cout // 8, b, h, w, 8, dtype=torch.float32, device=x.device) if out != "nhwc" else None
    nbytes, ws = 0, None
    if layout == 0:
        nbytes = int(lib.mrcnn_conv3x3_winograd_workspace_bytes(b, h, w, cin))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)

    def book():
        m, k = b * h * w, 9 * (algo_cin or cin)
        # FLOPs are the algorithmic ones of the convolution (2*M*N*K), as for the direct kernel — not the reduced
        # multiply count Winograd actually executes
        return (2.0 * m * cout * k, (m, cout, k), 4.0 * (m * cin + m * cout * (2 if out == "both" else 1) + cout * k),
                "winograd_spatial" if int(lib.mrcnn_conv3x3_winograd_heads_tile_mode(h, w)) == 2 else "winograd")
    _launch(lib.mrcnn_conv3x3_winograd_f32,
            (x.data_ptr(), layout, b, h, w, cin, u.data_ptr(), cout, _ptr(scale), _ptr(shift), 1 if relu else 0, _ptr(y), _ptr(yk),
             _ptr(ws), nbytes, _stream()), book)
    return y if out == "nhwc" else yk if out == "kblocked" else (y, yk)


# --------------------------------------------------------------------------------------------------
# Winograd F(4x4,3x3) 3x3 stride-1 SAME conv (csrc/conv_wino4.hip): maps with H % 4 == W % 4 == 0, Cout % 64 == 0
# --------------------------------------------------------------------------------------------------
def conv3x3_winograd4_supported(h: int, w: int, cin: int, cout: int, batch: int = 1) -> bool:
    """Shapes the F(4x4) kernel takes — its 32-bit offset limits (4 * batch * h * w * channels <= 0xFFFFFFF0 bytes) included."""
    return bool(lib.mrcnn_conv3x3_winograd4_supported(int(batch), int(h), int(w), int(cin), int(cout)))


@_on_device
def winograd4_weights(w_ohwi: torch.Tensor) -> torch.Tensor:
    """[Cout,3,3,Cin] fp32 → G g G^T (6 x 6, evaluated in double) in the kernel's order [Cin/4,36,2,Cout,2]."""
    _need_gpu(w_ohwi)
    assert w_ohwi.dtype == torch.float32 and w_ohwi.is_contiguous() and tuple(w_ohwi.shape[1:3]) == (3, 3)
    cout, cin = w_ohwi.size(0), w_ohwi.size(3)
    assert cin % 4 == 0
    u = torch.empty(cin // 4, 36, 2, cout, 2, dtype=torch.float32, device=w_ohwi.device)
    check(lib.mrcnn_winograd4_weights_f32(w_ohwi.data_ptr(), cout, cin, u.data_ptr(), _stream()))
    return u


@_on_device
def conv3x3_winograd4(x_kblocked: torch.Tensor, u4: torch.Tensor, scale, shift, relu: bool = False, algo_cin=None,
                      out: str = "nhwc"):
    """relu(conv3x3_same(x) * scale + shift) with u4 from winograd4_weights; x k-blocked [Cin/8,B,H,W,8].
    out: "nhwc" → [B,H,W,Cout]; "kblocked" → [Cout/8,B,H,W,8]; "both" → (nhwc, kblocked)."""
    _need_gpu(x_kblocked, u4, scale, shift)
    assert x_kblocked.dim() == 5 and x_kblocked.dtype == torch.float32 and x_kblocked.is_contiguous()
    assert u4.is_contiguous() and out in ("nhwc", "kblocked", "both")
    g, b, h, w, _ = x_kblocked.shape
    cin, cout = g * 8, u4.size(3)
    assert u4.size(0) * 4 == cin and conv3x3_winograd4_supported(h, w, cin, cout, b), (b, h, w, cin, cout)
    y = torch.empty(b, h, w, cout, dtype=torch.float32, device=x_kblocked.device) if out != "kblocked" else None
    yk = torch.empty(cout // 8, b, h, w, 8, dtype=torch.float32, device=x_kblocked.device) if out != "nhwc" else None

    def book():
        m, k = b * h * w, 9 * (algo_cin or cin)
        return (2.0 * m * cout * k, (m, cout, k), 4.0 * (m * cin + m * cout * (2 if out == "both" else 1) + 4 * cout * k),
                "winograd4", 2.0 * m * cout * k / 4.0)
    _launch(lib.mrcnn_conv3x3_winograd4_f32,
            (x_kblocked.data_ptr(), b, h, w, cin, u4.data_ptr(), cout, _ptr(scale), _ptr(shift), 1 if relu else 0, _ptr(y),
             _ptr(yk), _stream()), book)
    return y if out == "nhwc" else yk if out == "kblocked" else (y, yk)


@_on_device
def conv3x3_winograd4_conv3(x_kblocked: torch.Tensor, u4: torch.Tensor, scale, shift, w3: torch.Tensor, scale3, shift3,
                            residual: torch.Tensor, algo_cin=None) -> torch.Tensor:
    """conv2 + conv3 of a Bottleneck in one launch (model.py:197-209): relu(conv3x3_same(x) * scale + shift) — 64 channels,
    never written — times the 1x1 expansion w3 [C3,1,1,64], affine (scale3, shift3), + residual [B,H,W,C3], ReLU.
    x k-blocked [Cin/8,B,H,W,8]; u4 = winograd4_weights of the [64,3,3,Cin] conv2 weight. Equals conv3x3_winograd4 followed
    by conv_bn_act(..., residual=...) bit for bit."""
    _need_gpu(x_kblocked, u4, scale, shift, w3, scale3, shift3, residual)
    assert x_kblocked.dim() == 5 and x_kblocked.is_contiguous() and x_kblocked.dtype == torch.float32
    g, b, h, w, _ = x_kblocked.shape
    cin, c3 = g * 8, w3.size(0)
    assert u4.is_contiguous() and u4.size(0) * 4 == cin and u4.size(3) == 64 and conv3x3_winograd4_supported(h, w, cin, 64, b)
    assert w3.is_contiguous() and w3.numel() == c3 * 64 and c3 % 32 == 0
    assert residual.is_contiguous() and tuple(residual.shape) == (b, h, w, c3) and residual.dtype == torch.float32
    y = torch.empty(b, h, w, c3, dtype=torch.float32, device=x_kblocked.device)

    def book():
        m, k = b * h * w, 9 * (algo_cin or cin)
        algo = 2.0 * m * (64 * k + 64 * c3)
        return (algo, (m, c3, k + 64), 4.0 * (m * cin + 2 * m * c3 + 4 * 64 * k + 64 * c3), "winograd4",
                2.0 * m * (64 * k / 4.0 + 64 * c3))
    _launch(lib.mrcnn_conv3x3_winograd4_conv3_f32,
            (x_kblocked.data_ptr(), b, h, w, cin, u4.data_ptr(), _ptr(scale), _ptr(shift), w3.data_ptr(), c3, _ptr(scale3),
             _ptr(shift3), residual.data_ptr(), y.data_ptr(), _stream()), book)
    return y


@_on_device
def conv3x3_winograd4_heads(x_kblocked: torch.Tensor, u4: torch.Tensor, scale, shift, w_head32: torch.Tensor,
                            relu: bool = True, algo_cin=None) -> HeadSums:
    """The RPN level in one launch on the F(4x4) kernel: relu(conv3x3_same(x)*scale+shift) and its two 1x1 heads
    (w_head32 [32, Cout]: rows 0..17 = conv_class then conv_bbox) → HeadSums with tile_mode 3."""
    _need_gpu(x_kblocked, u4, scale, shift, w_head32)
    assert x_kblocked.dim() == 5 and x_kblocked.is_contiguous() and x_kblocked.dtype == torch.float32
    g, b, h, w, _ = x_kblocked.shape
    cin, cout = g * 8, u4.size(3)
    assert u4.is_contiguous() and u4.size(0) * 4 == cin and conv3x3_winograd4_supported(h, w, cin, cout, b)
    assert w_head32.is_contiguous() and tuple(w_head32.shape) == (32, cout)
    rows = int(lib.mrcnn_conv3x3_winograd4_heads_rows(b, h, w))
    part = torch.empty(rows, 32, dtype=torch.float32, device=x_kblocked.device)

    def book():
        m, k = b * h * w, 9 * (algo_cin or cin)
        return (2.0 * m * cout * (k + 18), (m, cout, k), 4.0 * (m * cin + part.numel() + 4 * cout * k), "winograd4",
                2.0 * m * cout * (k / 4.0 + 32))
    _launch(lib.mrcnn_conv3x3_winograd4_heads_f32,
            (x_kblocked.data_ptr(), b, h, w, cin, u4.data_ptr(), cout, _ptr(scale), _ptr(shift), 1 if relu else 0,
             w_head32.data_ptr(), part.data_ptr(), _stream()), book)
    return HeadSums(part, b, h, w, 3)


@_on_device
def stem_conv(x: torch.Tensor, w: torch.Tensor, scale, shift, relu: bool = True, algo_cin: int | None = None,
              nchw: bool = False, out_f16: bool = False):
    """The ResNet stem: conv 7x7 stride 2 pad 3 + affine + ReLU. x NHWC [B,H,W,4] (RGB + zero channel) — or, with nchw=True,
    the molded image itself [B,3,H,W] (no layout pass beforehand; same result bit for bit) —, w OHWI [64,7,7,4] → [B,H/2,W/2,64]."""
    _need_gpu(x, w, scale, shift)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.size(1 if nchw else 3) == (3 if nchw else 4)
    assert w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (64, 7, 7, 4)
    if nchw:
        b, _, h, wd = x.shape
    else:
        b, h, wd, _ = x.shape
    assert nchw or not out_f16, "the fp16-output form reads the NCHW image"
    y = torch.empty(b, h // 2, wd // 2, 64, dtype=torch.float16 if out_f16 else torch.float32, device=x.device)
    fn = lib.mrcnn_stem_conv7x7_s2_nchw_f16out if out_f16 else \
        lib.mrcnn_stem_conv7x7_s2_nchw_f32 if nchw else lib.mrcnn_stem_conv7x7_s2_nhwc_f32

    def book():
        m, k = y.numel() // 64, 49 * (algo_cin or 4)
        return 2.0 * m * 64 * k, (m, 64, k), 4.0 * (x.numel() + w.numel()) + y.numel() * y.element_size(), "stem"
    _launch(fn, (x.data_ptr(), b, h, wd, w.data_ptr(), _ptr(scale), _ptr(shift), 1 if relu else 0, y.data_ptr(), _stream()), book)
    return y


def _check_stem_pool(x, w, scale, shift):
    """What both stem + max-pool forms take: x the molded NCHW image [B,3,H,W] fp32 with H and W multiples of 4, w OHWI
    [64,7,7,4] fp32. → (B, H, W)."""
    _need_gpu(x, w, scale, shift)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.size(1) == 3
    assert w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (64, 7, 7, 4)
    b, _, h, wd = x.shape
    assert h % 4 == 0 and wd % 4 == 0
    return b, h, wd


@_on_device
def stem_pool_f16(x: torch.Tensor, w: torch.Tensor, scale, shift, algo_cin: int | None = None) -> torch.Tensor:
    """The "f16" mode's stem + max-pool in one launch on the fp16 MFMA (model.py:223-229): x the molded NCHW image [B,3,H,W]
    fp32, w OHWI [64,7,7,4] fp32 → fp16 NHWC [B, ceil(H/4), ceil(W/4), 64]."""
    b, h, wd = _check_stem_pool(x, w, scale, shift)
    y = torch.empty(b, h // 4, wd // 4, 64, dtype=torch.float16, device=x.device)

    def book():
        m, k = b * (h // 2) * (wd // 2), 49 * (algo_cin or 4)
        return 2.0 * m * 64 * k, (m, 64, k), 4.0 * (x.numel() + w.numel()) + y.numel() * 2, "stem"
    _launch(lib.mrcnn_stem_conv7x7_s2_pool_f16,
            (x.data_ptr(), b, h, wd, w.data_ptr(), _ptr(scale), _ptr(shift), y.data_ptr(), _stream()), book)
    return y


@_on_device
def stem_pool_f32(x: torch.Tensor, w: torch.Tensor, scale, shift, algo_cin: int | None = None) -> torch.Tensor:
    """The exact-fp32 stem + max-pool in one launch (model.py:223-229; csrc/stem.hip: stem7x7_s2_pool_f32): x the molded NCHW
    image [B,3,H,W] fp32 (H, W multiples of 4), w OHWI [64,7,7,4] fp32 (channel 3 zero) → fp32 NHWC [B, H/4, W/4, 64]."""
    b, h, wd = _check_stem_pool(x, w, scale, shift)
    assert b * h * wd < (1 << 27), "stem_pool_f32: B*H*W < 2^27 pixels (32-bit byte offsets of the fp32 output)"
    y = torch.empty(b, h // 4, wd // 4, 64, dtype=torch.float32, device=x.device)

    def book():
        m, k = b * (h // 2) * (wd // 2), 49 * (algo_cin or 3)
        # executed: 77 MFMAs of K = 2 per 32 x 32 block (k = 22 per filter row) on 15 x 33 conv pixels per 7 x 16 pooled ones,
        # padded to 512 GEMM rows
        tiles = b * -(-(h // 4) // 7) * -(-(wd // 4) // 16)
        return 2.0 * m * 64 * k, (m, 64, k), 4.0 * (x.numel() + 64 * 147 + y.numel()), "stem", 2.0 * tiles * 512 * 64 * 154
    _launch(lib.mrcnn_stem_conv7x7_s2_pool_f32,
            (x.data_ptr(), b, h, wd, w.data_ptr(), _ptr(scale), _ptr(shift), y.data_ptr(), _stream()), book)
    return y
