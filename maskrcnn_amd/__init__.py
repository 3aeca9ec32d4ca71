"""maskrcnn_amd — MI355X-native (gfx950) Mask R-CNN inference hot path.

Importing the package loads libmaskrcnn_hip.so and registers torch.ops.maskrcnn.*; there is no CPU or
PyTorch fallback for the ops (a missing library is an ImportError).
"""
import torch as _torch

from . import _lib  # noqa: F401  (fails loudly if the HIP library is missing)
from . import ops  # noqa: F401  (registers torch.ops.maskrcnn.*)
from . import losses  # noqa: F401  (the training losses on the targets' padded outputs)
from . import layers  # noqa: F401  (the head layers' conv / transposed conv with a grad_fn)
from . import optim  # noqa: F401  (ClippedSGD: gradient norm, clip and momentum step in three launches)
from . import rpn_train  # noqa: F401  (TrainableRPN: a dense pass without a graph, forward and backward on the sampled anchors)
from . import head_train  # noqa: F401  (TrainableClassifier / TrainableMask / TrainableHeads: the mask branch on the positives' class planes)


class _RoiAlignNCHW(_torch.autograd.Function):
    """roi_align below as ONE function of the four NCHW maps: the backward turns the incoming gradient channels-last, calls
    ops.roi_align_pyramid_backward (fixed summation order: the reference's CPU bits) and turns the four results back. The layout
    passes are exact copies. No gradient for the boxes (model.py:358)."""

    @staticmethod
    def forward(ctx, boxes, pool_size, area, p2, p3, p4, p5):
        maps = [p2, p3, p4, p5]
        fms = [ops.nchw_to_nhwc(m.unsqueeze(0).contiguous()) for m in maps]
        pooled = ops.roi_align_pyramid(fms, boxes.contiguous(), pool_size, area, rois_per_image=boxes.size(0))
        ctx.save_for_backward(boxes)
        ctx.call = (pool_size, area, [(m.size(1), m.size(2)) for m in maps])
        return ops.nhwc_to_nchw(pooled)

    @staticmethod
    @_torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        (boxes,) = ctx.saved_tensors
        pool_size, area, sizes = ctx.call
        grads = ops.roi_align_pyramid_backward(ops.nchw_to_nhwc(grad.contiguous()), boxes.contiguous(), pool_size, area, 1, sizes,
                                               rois_per_image=boxes.size(0))
        return (None, None, None) + tuple(ops.nhwc_to_nchw(g).squeeze(0) if need else None
                                          for g, need in zip(grads, ctx.needs_input_grad[3:]))


def roi_align(inputs, pool_size, image_shape):
    """Drop-in for the reference's `roi_align(inputs, pool_size, image_shape)` (model.py:276-393), same arguments and result:
    inputs = [boxes [1, N, 4] or [N, 4] normalised (y1, x1, y2, x2)] + [P2, P3, P4, P5], each [1, C, H_l, W_l] NCHW fp32 on the
    GPU; image_shape = (height, width[, channels]) of the padded image → pooled [N, C, pool_size, pool_size] in RoI order.
    The reference loops over the four levels with a `nonzero()` / `any()` host synchronisation per level, one `CropFunction`
    call each, a `cat` and an inverse permutation (:340-387); here the level of every box (:331-338, same fp32 operations) is
    decided inside ONE launch of the pyramid kernel (mrcnn_roi_align_pyramid_nhwc_f32) and nothing touches the host. Like the
    reference (:312-313) the batch dimension of every entry of `inputs` is squeezed IN PLACE in the caller's list. The maps are
    converted to channels-last on the way in and the crops back on the way out (the pipeline, which keeps NHWC maps, calls
    ops.roi_align_pyramid directly). Differentiable with respect to the maps (not the boxes, model.py:358): where a map requires
    grad the result carries a grad_fn whose backward is ops.roi_align_pyramid_backward between two exact layout passes."""
    for i in range(len(inputs)):
        inputs[i] = inputs[i].squeeze(0)
    boxes, maps = inputs[0], inputs[1:]
    if len(maps) != 4:
        raise RuntimeError(f"roi_align: four pyramid levels expected, got {len(maps)}")
    area = float(image_shape[0] * image_shape[1])
    if _torch.is_grad_enabled() and any(m.requires_grad for m in maps):   # the same launches, with a grad_fn on the result
        return _RoiAlignNCHW.apply(boxes, int(pool_size), area, *maps)
    fms = [ops.nchw_to_nhwc(m.unsqueeze(0).contiguous()) for m in maps]
    pooled = ops.roi_align_pyramid(fms, boxes.contiguous(), int(pool_size), area, rois_per_image=boxes.size(0))
    return ops.nhwc_to_nchw(pooled)


__all__ = ["ops", "roi_align", "losses", "layers", "optim", "rpn_train", "head_train"]   # reference-signature refine stages: maskrcnn_amd.refine (imports the pipeline)
