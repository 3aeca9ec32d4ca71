"""The five training losses of Mask R-CNN for a batch of images, forward and backward, on the device.

The reference's train_epoch (model.py:1622-1629) adds RPN.class_loss, RPN.boxes_loss (model.py:652-718), Classifier.class_loss,
Classifier.boxes_loss (model.py:802-845) and Mask.mask_loss (model.py:922-953). Each of them is a torch.nonzero (a host read-back),
two or three gathers and a stock loss, per image. Here they read the padded outputs of targets.rpn_targets and
targets.detection_targets in place (csrc/losses.hip; the rule is stated at mrcnn_rpn_loss_forward in include/maskrcnn_hip.h):

    rpn_match, rpn_bbox = targets.rpn_targets(anchors, gt_boxes, gt_class_ids)
    t = targets.detection_targets(rois, gt_boxes, gt_class_ids, gt_masks)
    rpn = losses.rpn_losses(rpn_match, rpn_class_logits, rpn_pred_bbox, rpn_bbox)
    head = losses.head_losses(t, class_logits, pred_bbox, pred_masks)
    (sum(rpn[:2]) + sum(head[:3])).backward()          # gradients arrive in the five prediction tensors

Nothing in that path synchronises with the host. reduction="mean" divides the batch's sum by the batch's count (the reference's
functions on the concatenation of the images; the reference itself at B = 1), reduction="per_image" returns float32 [B], each entry
the reference's value for that image alone. One deviation by design: a loss without a contributing element is 0 with zero
gradients, where the reference's stock losses return NaN, the mean of nothing.

device="cpu" runs the same rule in numpy float64 without the library (rpn_terms_numpy / head_terms_numpy and the two *_losses_numpy
below, gradients included): the fixture's generator, the host tests and a user without a GPU read it.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from .targets import DetectionTargets

__all__ = ["rpn_losses", "head_losses", "classifier_losses", "RpnLosses", "HeadLosses", "rpn_terms_numpy", "head_terms_numpy",
           "classifier_terms_numpy", "rpn_losses_numpy", "head_losses_numpy", "reduce_numpy", "MAX_CLASSES"]

MAX_CLASSES = 4096
REDUCTIONS = ("mean", "per_image")


class RpnLosses(NamedTuple):
    rpn_class_loss: torch.Tensor     # float32, 0-dim ("mean") or [B] ("per_image")
    rpn_bbox_loss: torch.Tensor
    status: torch.Tensor             # int32 [B]; bit 0: the image has more positives than target rows


class HeadLosses(NamedTuple):
    class_loss: torch.Tensor
    bbox_loss: torch.Tensor
    mask_loss: torch.Tensor
    status: torch.Tensor             # int32 [B]; bit 1: a class id outside 0 .. C-1 (the slot is skipped)


# ----------------------------------------------------------------------------------------------------------------------
# The rule in numpy float64, one image at a time: sums, counts and the derivative of every element's term
# ----------------------------------------------------------------------------------------------------------------------
def _cross_entropy(x: np.ndarray, c: np.ndarray):
    """x float64 [n,C], c int [n] → (terms [n], derivatives [n,C]): log(sum exp(x - max)) - (x[c] - max); softmax - onehot."""
    rows = np.arange(x.shape[0])
    mx = x.max(axis=1) if x.shape[0] else np.zeros(0)
    e = np.exp(x - mx[:, None])
    s = e.sum(axis=1)
    d = e / s[:, None]
    d[rows, c] -= 1.0
    return np.log(s) - (x[rows, c] - mx), d


def _smooth_l1(d: np.ndarray):
    a = np.abs(d)
    return np.where(a < 1.0, 0.5 * d * d, a - 0.5), np.where(a < 1.0, d, np.sign(d))


def _binary_cross_entropy(p: np.ndarray, y: np.ndarray):
    with np.errstate(divide="ignore", invalid="ignore"):
        term = -(y * np.maximum(np.log(p), -100.0) + (1.0 - y) * np.maximum(np.log1p(-p), -100.0))
        return term, (p - y) / np.maximum((1.0 - p) * p, 1e-12)


def rpn_terms_numpy(match, logits, pred_bbox, target_bbox):
    """One image: match [A] of -1 / 0 / 1, logits [A,2], pred_bbox [A,4], target_bbox [count,4] → (sums float64 [2], counts int64 [2],
    status, d_logits float64 [A,2], d_bbox float64 [A,4]): the sums of the class and box terms, the numbers of elements, and each
    element's derivative (0 where it does not contribute; not yet divided by a count)."""
    m = np.asarray(match).reshape(-1)
    x, p, t = np.asarray(logits, np.float32), np.asarray(pred_bbox, np.float32), np.asarray(target_bbox, np.float32)
    d_logits, d_bbox = np.zeros(x.shape), np.zeros(p.shape)
    nz = np.where(m != 0)[0]
    terms, d_logits[nz] = _cross_entropy(x[nz].astype(np.float64), (m[nz] == 1).astype(np.int64))
    pos = np.where(m == 1)[0]
    used = pos[:t.shape[0]]
    box, d_bbox[used] = _smooth_l1(p[used].astype(np.float64) - t[:len(used)].astype(np.float64))
    return (np.array([terms.sum(), box.sum()]), np.array([len(nz), 4 * len(used)], np.int64), int(len(pos) > t.shape[0]), d_logits, d_bbox)


def head_terms_numpy(target_class_ids, num_rois, target_deltas, target_mask, logits, pred_bbox, pred_masks):
    """One image: target_class_ids [count], num_rois (an int), target_deltas [count,4], target_mask [count,mh,mw], logits [count,C],
    pred_bbox [count,C,4], pred_masks [count,C,mh,mw] → (sums float64 [3], counts int64 [3], status, d_logits, d_bbox, d_masks)."""
    ids = np.asarray(target_class_ids).reshape(-1).astype(np.int64)
    x, pb, pm = np.asarray(logits, np.float32), np.asarray(pred_bbox, np.float32), np.asarray(pred_masks, np.float32)
    td, tm = np.asarray(target_deltas, np.float32), np.asarray(target_mask, np.float32)
    count, classes = x.shape
    d_logits, d_bbox, d_masks = np.zeros(x.shape), np.zeros(pb.shape), np.zeros(pm.shape)
    valid = np.arange(count) < min(max(int(num_rois), 0), count)
    bad = valid & ((ids < 0) | (ids >= classes))
    use = np.where(valid & ~bad)[0]
    ce, d_logits[use] = _cross_entropy(x[use].astype(np.float64), ids[use])
    pos = use[ids[use] > 0]
    box, d_bbox[pos, ids[pos]] = _smooth_l1(pb[pos, ids[pos]].astype(np.float64) - td[pos].astype(np.float64))
    mask, d_masks[pos, ids[pos]] = _binary_cross_entropy(pm[pos, ids[pos]].astype(np.float64), tm[pos].astype(np.float64))
    # a slot's mask terms are added up first, then the slots: the order of the device's partial sums
    sums = np.array([ce.sum(), box.sum(), mask.reshape(len(pos), tm.shape[1] * tm.shape[2]).sum(axis=1).sum()])
    counts = np.array([len(use), 4 * len(pos), len(pos) * tm.shape[1] * tm.shape[2]], np.int64)
    return sums, counts, 2 * int(bad.any()), d_logits, d_bbox, d_masks


def classifier_terms_numpy(target_class_ids, num_rois, target_deltas, logits, pred_bbox):
    """head_terms_numpy without the mask tensors → (sums float64 [2], counts int64 [2], status, d_logits, d_bbox): its class and box
    columns, computed by the same statements."""
    count, classes = np.asarray(logits).shape
    sums, counts, status, d_logits, d_bbox, _ = head_terms_numpy(target_class_ids, num_rois, target_deltas, np.zeros((count, 1, 1), np.float32),
                                                                 logits, pred_bbox, np.full((count, classes, 1, 1), 0.5, np.float32))
    return sums[:2], counts[:2], status, d_logits, d_bbox


def reduce_numpy(sums, counts, reduction: str = "mean"):
    """sums float64 [B,k], counts [B,k] → (losses float32 [k] or [B,k], denominators int64 [B,k]): the quotient narrowed last, 0 where
    nothing contributes; an element's gradient is its derivative times (upstream gradient / denominator)."""
    sums, counts = np.asarray(sums, np.float64), np.asarray(counts, np.int64)
    shape = sums.shape
    if reduction == "mean":
        sums, counts = sums.sum(axis=0, keepdims=True), counts.sum(axis=0, keepdims=True)
    losses = np.where(counts > 0, sums / np.maximum(counts, 1), 0.0).astype(np.float32)
    return (losses[0] if reduction == "mean" else losses), np.broadcast_to(counts, shape)


def _batch_terms(fn, arrays):
    """fn over the images of a batch → (sums [B,k], counts [B,k], status int32 [B], [derivatives stacked over the batch])."""
    rows = [fn(*[a[i] for a in arrays]) for i in range(arrays[0].shape[0])]
    n = len(rows[0])
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.array([r[2] for r in rows], np.int32),
            [np.stack([r[k] for r in rows]) for k in range(3, n)])


def _scaled(derivs, denominators, grad_out):
    """The derivative arrays [B,...] of losses 0, 1, ... times grad_out (float64 [k] or [B,k]) / denominators [B,k] (0 where that is
    0), narrowed to float32."""
    go = np.broadcast_to(np.asarray(grad_out, np.float64), denominators.shape)
    scale = np.where(denominators > 0, go / np.maximum(denominators, 1), 0.0)
    return [(d * scale[:, k].reshape((-1,) + (1,) * (d.ndim - 1))).astype(np.float32) for k, d in enumerate(derivs)]


def rpn_losses_numpy(match, logits, pred_bbox, target_bbox, reduction: str = "mean"):
    """The batch in numpy: match [B,A], logits [B,A,2], pred_bbox [B,A,4], target_bbox [B,count,4] → (losses float32 [2] or [B,2]:
    class, box; counts int32 [B,2]; status int32 [B]; grad_logits float32 [B,A,2]; grad_bbox float32 [B,A,4]), the gradients for an
    upstream gradient of 1 on each loss (each image's loss under "per_image")."""
    sums, counts, status, derivs = _batch_terms(rpn_terms_numpy, [np.asarray(v) for v in (match, logits, pred_bbox, target_bbox)])
    losses, denominators = reduce_numpy(sums, counts, reduction)
    grads = _scaled(derivs, denominators, np.ones(2))
    return losses, counts.astype(np.int32), status, grads[0], grads[1]


def head_losses_numpy(target_class_ids, num_rois, target_deltas, target_mask, logits, pred_bbox, pred_masks, reduction: str = "mean"):
    """The batch in numpy, shapes as ops.head_loss → (losses float32 [3] or [B,3]: class, box, mask; counts int32 [B,3]; status int32
    [B]; grad_logits, grad_bbox, grad_masks float32 in the predictions' shapes)."""
    arrays = [np.asarray(v) for v in (target_class_ids, num_rois, target_deltas, target_mask, logits, pred_bbox, pred_masks)]
    sums, counts, status, derivs = _batch_terms(head_terms_numpy, arrays)
    losses, denominators = reduce_numpy(sums, counts, reduction)
    grads = _scaled(derivs, denominators, np.ones(3))
    return losses, counts.astype(np.int32), status, grads[0], grads[1], grads[2]


# ----------------------------------------------------------------------------------------------------------------------
# autograd: the op pairs on the device, the numpy rule on the host
# ----------------------------------------------------------------------------------------------------------------------
def _reduce_device(sums: torch.Tensor, counts: torch.Tensor, per_image: bool) -> torch.Tensor:
    """float32 [k] or [B,k]: the fp64 quotient narrowed last, 0 where nothing contributes. No host read."""
    if not per_image:
        sums, counts = sums.sum(dim=0), counts.sum(dim=0)
    q = sums / counts.clamp(min=1).to(torch.float64)
    return torch.where(counts > 0, q, torch.zeros_like(q)).to(torch.float32)


class _RpnLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, pred_bbox, match, target_bbox, per_image):
        from . import ops
        sums, counts, status, chunk_pos = ops.rpn_loss(match, logits, pred_bbox, target_bbox)
        ctx.save_for_backward(match, logits, pred_bbox, target_bbox, chunk_pos, counts)
        ctx.mark_non_differentiable(status)
        return _reduce_device(sums, counts, per_image), status

    @staticmethod
    def backward(ctx, grad_losses, _):
        from . import ops
        grad_logits, grad_bbox = ops.rpn_loss_backward(*ctx.saved_tensors, grad_losses.to(torch.float32).contiguous())
        return grad_logits, grad_bbox, None, None, None


class _HeadLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, pred_bbox, pred_masks, ids, num_rois, deltas, mask, per_image):
        from . import ops
        sums, counts, status = ops.head_loss(ids, num_rois, deltas, mask, logits, pred_bbox, pred_masks)
        ctx.save_for_backward(ids, num_rois, deltas, mask, logits, pred_bbox, pred_masks, counts)
        ctx.mark_non_differentiable(status)
        return _reduce_device(sums, counts, per_image), status

    @staticmethod
    def backward(ctx, grad_losses, _):
        from . import ops
        return (*ops.head_loss_backward(*ctx.saved_tensors, grad_losses.to(torch.float32).contiguous()), None, None, None, None, None)


class _NumpyLoss(torch.autograd.Function):
    """Either family on the host: forward(ctx, terms_fn, per_image, n_pred, *predictions, *targets)."""

    @staticmethod
    def forward(ctx, terms_fn, per_image, n_pred, *tensors):
        arrays = [t.detach().cpu().numpy() for t in tensors]
        preds, targets = arrays[:n_pred], arrays[n_pred:]
        order = [*targets[:1], *preds, *targets[1:]] if terms_fn is rpn_terms_numpy else [*targets, *preds]
        sums, counts, status, derivs = _batch_terms(terms_fn, order)
        losses, denominators = reduce_numpy(sums, counts, "per_image" if per_image else "mean")
        ctx.derivs, ctx.denominators, ctx.extra = derivs, denominators, len(tensors) - n_pred
        status = torch.from_numpy(status)
        ctx.mark_non_differentiable(status)
        return torch.from_numpy(np.ascontiguousarray(losses)), status

    @staticmethod
    def backward(ctx, grad_losses, _):
        grads = _scaled(ctx.derivs, ctx.denominators, grad_losses.detach().cpu().numpy().astype(np.float64))
        return (None, None, None, *[torch.from_numpy(g) for g in grads], *[None] * ctx.extra)


# ----------------------------------------------------------------------------------------------------------------------
# Front end
# ----------------------------------------------------------------------------------------------------------------------
def _device_of(device, *tensors) -> torch.device:
    if device is not None:
        return torch.device(device)
    return next((t.device for t in tensors if isinstance(t, torch.Tensor) and t.is_cuda), torch.device("cpu"))


def _tensor(x, dev, dtype=None) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.array(x))
    return x.to(dev, dtype) if dtype is not None else x.to(dev)


def _check_reduction(who: str, reduction: str) -> bool:
    if reduction not in REDUCTIONS:
        raise ValueError(f"{who}: reduction={reduction!r} must be one of {REDUCTIONS}")
    return reduction == "per_image"


def rpn_losses(rpn_match, rpn_class_logits, rpn_pred_bbox, target_bbox, reduction: str = "mean", device=None) -> RpnLosses:
    """RPN.class_loss and RPN.boxes_loss for a batch → RpnLosses(rpn_class_loss, rpn_bbox_loss, status).

    rpn_match: [B,A,1] or [B,A], int32 or int64, of -1 / 0 / 1, and target_bbox float32 [B,count,4], as targets.rpn_targets returns
    them. rpn_class_logits float32 [B,A,2], rpn_pred_bbox float32 [B,A,4]: the predictions; gradients flow into them. The k-th
    positive of an image in ascending anchor index is paired with target_bbox[b,k]; status bit 0 tells an image with more positives
    than rows (the extra ones are left out). device: where to compute — by default where the predictions are; "cpu" is the numpy
    route. No call synchronises with the host."""
    who = "rpn_losses"
    per_image = _check_reduction(who, reduction)
    dev = _device_of(device, rpn_class_logits, rpn_pred_bbox)
    match = _tensor(rpn_match, dev)
    if match.dim() == 3 and match.size(2) == 1:
        match = match.squeeze(2)
    logits, pred, target = _tensor(rpn_class_logits, dev, torch.float32), _tensor(rpn_pred_bbox, dev, torch.float32), _tensor(target_bbox, dev, torch.float32)
    if match.dim() != 2 or match.dtype not in (torch.int32, torch.int64) or match.size(0) < 1 or match.size(1) < 1:
        raise ValueError(f"{who}: rpn_match must be int32 or int64 [B,A,1] or [B,A], got {match.dtype} {tuple(match.shape)}")
    b, a = match.shape
    if tuple(logits.shape) != (b, a, 2) or tuple(pred.shape) != (b, a, 4):
        raise ValueError(f"{who}: rpn_class_logits must be [{b},{a},2] and rpn_pred_bbox [{b},{a},4], got {tuple(logits.shape)} and "
                         f"{tuple(pred.shape)}")
    if target.dim() != 3 or target.size(0) != b or target.size(2) != 4 or not 1 <= target.size(1) <= 1024:
        raise ValueError(f"{who}: target_bbox must be [{b},count,4] with count in [1, 1024], got {tuple(target.shape)}")
    match = match.to(torch.int32)
    if dev.type == "cpu":
        losses, status = _NumpyLoss.apply(rpn_terms_numpy, per_image, 2, logits, pred, match, target)
    else:
        losses, status = _RpnLoss.apply(logits, pred, match, target, per_image)
    return RpnLosses(losses[..., 0], losses[..., 1], status)


def head_losses(target_class_ids, num_rois, target_deltas, target_mask, class_logits=None, pred_bbox=None, pred_masks=None,
                reduction: str = "mean", device=None) -> HeadLosses:
    """Classifier.class_loss, Classifier.boxes_loss and Mask.mask_loss for a batch → HeadLosses(class_loss, bbox_loss, mask_loss,
    status). Also head_losses(t, class_logits, pred_bbox, pred_masks, ...) with t a targets.DetectionTargets.

    target_class_ids int [B,count], num_rois int [B] (num_pos + num_neg: the slots past it are padding and never contribute),
    target_deltas float32 [B,count,4], target_mask float32 [B,count,mh,mw]: as targets.detection_targets returns them.
    class_logits [B,count,C], pred_bbox [B,count,C,4], pred_masks [B,count,C,mh,mw], or flat over the slots ([B*count,...], the
    reference's [R,C,...]): the predictions; gradients flow into them. A positive slot (class id > 0) reads its class's box row and
    mask plane only. status bit 1 tells a class id outside 0 .. C-1, whose slot is skipped. device as for rpn_losses."""
    who = "head_losses"
    if isinstance(target_class_ids, DetectionTargets):
        if pred_bbox is not None or pred_masks is not None:
            raise ValueError(f"{who}: with a DetectionTargets pass class_logits, pred_bbox, pred_masks right after it")
        t, class_logits, pred_bbox, pred_masks = target_class_ids, num_rois, target_deltas, target_mask
        target_class_ids, num_rois, target_deltas, target_mask = t.target_class_ids, t.num_pos + t.num_neg, t.target_deltas, t.target_mask
    if class_logits is None or pred_bbox is None or pred_masks is None:
        raise ValueError(f"{who}: class_logits, pred_bbox and pred_masks are required")
    per_image = _check_reduction(who, reduction)
    dev = _device_of(device, class_logits, pred_bbox, pred_masks)
    ids, num_rois = _tensor(target_class_ids, dev), _tensor(num_rois, dev)
    deltas, mask = _tensor(target_deltas, dev, torch.float32), _tensor(target_mask, dev, torch.float32)
    logits, pbox, pmask = (_tensor(v, dev, torch.float32) for v in (class_logits, pred_bbox, pred_masks))
    if ids.dim() != 2 or ids.dtype not in (torch.int32, torch.int64) or ids.size(0) < 1 or not 1 <= ids.size(1) <= 1024:
        raise ValueError(f"{who}: target_class_ids must be int32 or int64 [B,count] with count in [1, 1024], got {ids.dtype} {tuple(ids.shape)}")
    b, count = ids.shape
    if mask.dim() != 4 or tuple(mask.shape[:2]) != (b, count) or not (1 <= mask.size(2) <= 64 and 1 <= mask.size(3) <= 64):
        raise ValueError(f"{who}: target_mask must be [{b},{count},mh,mw] with mh, mw in [1, 64], got {tuple(mask.shape)}")
    mh, mw = mask.shape[2:]
    if tuple(num_rois.shape) != (b,) or tuple(deltas.shape) != (b, count, 4):
        raise ValueError(f"{who}: num_rois must be [{b}] and target_deltas [{b},{count},4], got {tuple(num_rois.shape)} and {tuple(deltas.shape)}")
    if logits.dim() < 2 or logits.numel() % (b * count) or not 2 <= logits.size(-1) <= MAX_CLASSES:
        raise ValueError(f"{who}: class_logits must be [{b},{count},C] or [{b * count},C] with C in [2, {MAX_CLASSES}], got {tuple(logits.shape)}")
    c = logits.size(-1)
    want = ((b, count, c), (b, count, c, 4), (b, count, c, mh, mw))
    for name, v, shape in zip(("class_logits", "pred_bbox", "pred_masks"), (logits, pbox, pmask), want):
        if tuple(v.shape) not in (shape, (b * count, *shape[2:])):
            raise ValueError(f"{who}: {name} must be {list(shape)} or {[b * count, *shape[2:]]}, got {tuple(v.shape)}")
    logits, pbox, pmask = (v.reshape(shape) for v, shape in zip((logits, pbox, pmask), want))
    ids, num_rois = ids.to(torch.int32), num_rois.to(torch.int32)
    if dev.type == "cpu":
        losses, status = _NumpyLoss.apply(head_terms_numpy, per_image, 3, logits, pbox, pmask, ids, num_rois, deltas, mask)
    else:
        losses, status = _HeadLoss.apply(logits, pbox, pmask, ids, num_rois, deltas, mask, per_image)
    return HeadLosses(losses[..., 0], losses[..., 1], losses[..., 2], status)


def classifier_losses(target_class_ids, num_rois, target_deltas=None, class_logits=None, pred_bbox=None, reduction: str = "mean",
                      device=None):
    """Classifier.class_loss and Classifier.boxes_loss for a batch, without a mask tensor → (class_loss, bbox_loss, status): the
    first two losses of head_losses and its status, bit for bit, gradients included (on the device the same two launches with null
    mask pointers, on the CPU the same numpy statements). Also classifier_losses(t, class_logits, pred_bbox, ...) with t a
    targets.DetectionTargets. Shapes, reduction and device as for head_losses; the predictions may be flat over the slots."""
    who = "classifier_losses"
    if isinstance(target_class_ids, DetectionTargets):
        if class_logits is not None or pred_bbox is not None:
            raise ValueError(f"{who}: with a DetectionTargets pass class_logits and pred_bbox right after it")
        t, class_logits, pred_bbox = target_class_ids, num_rois, target_deltas
        target_class_ids, num_rois, target_deltas = t.target_class_ids, t.num_pos + t.num_neg, t.target_deltas
    if target_deltas is None or class_logits is None or pred_bbox is None:
        raise ValueError(f"{who}: target_deltas, class_logits and pred_bbox are required")
    per_image = _check_reduction(who, reduction)
    dev = _device_of(device, class_logits, pred_bbox)
    ids, num_rois = _tensor(target_class_ids, dev), _tensor(num_rois, dev)
    deltas, logits, pbox = (_tensor(v, dev, torch.float32) for v in (target_deltas, class_logits, pred_bbox))
    if ids.dim() != 2 or ids.dtype not in (torch.int32, torch.int64) or ids.size(0) < 1 or not 1 <= ids.size(1) <= 1024:
        raise ValueError(f"{who}: target_class_ids must be int32 or int64 [B,count] with count in [1, 1024], got {ids.dtype} {tuple(ids.shape)}")
    b, count = ids.shape
    if tuple(num_rois.shape) != (b,) or tuple(deltas.shape) != (b, count, 4):
        raise ValueError(f"{who}: num_rois must be [{b}] and target_deltas [{b},{count},4], got {tuple(num_rois.shape)} and {tuple(deltas.shape)}")
    if logits.dim() < 2 or logits.numel() % (b * count) or not 2 <= logits.size(-1) <= MAX_CLASSES:
        raise ValueError(f"{who}: class_logits must be [{b},{count},C] or [{b * count},C] with C in [2, {MAX_CLASSES}], got {tuple(logits.shape)}")
    c = logits.size(-1)
    want = ((b, count, c), (b, count, c, 4))
    for name, v, shape in zip(("class_logits", "pred_bbox"), (logits, pbox), want):
        if tuple(v.shape) not in (shape, (b * count, *shape[2:])):
            raise ValueError(f"{who}: {name} must be {list(shape)} or {[b * count, *shape[2:]]}, got {tuple(v.shape)}")
    logits, pbox = (v.reshape(shape) for v, shape in zip((logits, pbox), want))
    ids, num_rois = ids.to(torch.int32), num_rois.to(torch.int32)
    if dev.type == "cpu":
        losses, status = _NumpyLoss.apply(classifier_terms_numpy, per_image, 2, logits, pbox, ids, num_rois, deltas)
    else:
        losses, status = _HeadLoss.apply(logits, pbox, None, ids, num_rois, deltas, None, per_image)
    return losses[..., 0], losses[..., 1], status
