"""Bindings of the training side: RPN targets (csrc/targets.hip), detection targets (csrc/detection_targets.hip), the five
losses, forward and backward (csrc/losses.hip), the backward of the pyramid RoIAlign (csrc/roi_align_backward.hip), the backward
of the conv + frozen affine + activation at stride 1 or 2 (csrc/conv_backward.hip) and the backbone's two other gradients, the
dilation of a compact stride-2 gradient and the max-pool backward (csrc/pool_backward.hip), clipped SGD (csrc/optim.hip) and the
RPN's training branch on the sampled anchors: compaction, patch gather and patch scatter (csrc/rpn_train.hip), and the mask head's
class-plane branch: the 1x1 conv to each slot's own class and the mask loss on those planes (csrc/mask_train.hip). ops.py re-exports every name here;
argument checks and registration are _binding.py's."""
from __future__ import annotations

import collections
import ctypes

import torch

from ._binding import _launch, _on_device, _ptr, _ptr0, _stream, checked, checked_out, refuse, register, workspace
from ._lib import c_i32, c_vp, lib

_I32, _F32 = torch.int32, torch.float32
_ANCHORS_HINT = " (anchors.pyramid_anchors(cfg, dtype=torch.float64))"


# --------------------------------------------------------------------------------------------------
# RPN training targets: data.rpn_samples for a batch (csrc/targets.hip)
# --------------------------------------------------------------------------------------------------
def _target_std(who, std_dev):
    std = [float(v) for v in std_dev]
    if len(std) != 4:
        raise RuntimeError(f"{who}: std_dev must hold 4 numbers, got {len(std)}")
    return std


@_on_device
def anchor_match(anchors: torch.Tensor, gt_boxes: torch.Tensor, gt_class_ids: torch.Tensor, gt_off: torch.Tensor,
                 neg_iou: float = 0.3, pos_iou: float = 0.7, crowd_iou: float = 0.001):
    """Steps 1-6 of data.rpn_samples (data.py:485-540; the rule is stated at mrcnn_anchor_match in include/maskrcnn_hip.h) for B
    images: anchors float64 [A,4], ground truth packed as gt_boxes float32 [M,4], gt_class_ids int32 [M], gt_off int32 [B+1] →
    (match int32 [B,A] of -1 / 0 / 1, iou_argmax int32 [B,A] (row position within the image), iou_max float32 [B,A], gt_argmax
    int32 [M] (-1: crowd or dropped row), status int32 [B] (bit 0: no kept row in the image)). The thresholds are narrowed to
    fp32. No host synchronisation."""
    who = "anchor_match"
    anchors = checked(who, "anchors", anchors, torch.float64, (("A", 1), 4), hint=_ANCHORS_HINT)
    gt_boxes = checked(who, "gt_boxes", gt_boxes, _F32, ("M", 4))
    gt_off = checked(who, "gt_off", gt_off, _I32, (("B+1", 2),))
    m, a, b, dev = gt_boxes.size(0), anchors.size(0), gt_off.numel() - 1, anchors.device
    gt_class_ids = checked(who, "gt_class_ids", gt_class_ids, _I32, (m,))
    match = torch.empty(b, a, dtype=torch.int32, device=dev)
    iou_argmax = torch.empty(b, a, dtype=torch.int32, device=dev)
    iou_max = torch.empty(b, a, dtype=torch.float32, device=dev)
    gt_argmax = torch.empty(m, dtype=torch.int32, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    nbytes = int(lib.mrcnn_anchor_match_workspace_bytes(m))
    ws = workspace(nbytes, dev)
    _launch(lib.mrcnn_anchor_match,
            (anchors.data_ptr(), a, _ptr0(gt_boxes), _ptr0(gt_class_ids), gt_off.data_ptr(), m, b,
             float(neg_iou), float(pos_iou), float(crowd_iou), match.data_ptr(), iou_argmax.data_ptr(), iou_max.data_ptr(),
             _ptr0(gt_argmax), status.data_ptr(), ws.data_ptr(), nbytes, _stream()),
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
    match = checked(who, "match", match, _I32, (("B", 1), ("A", 1)))    # `out is match`: contiguous then, and passed on as it is
    b, a = match.shape
    keys = checked(who, "keys", keys, _I32, (b, a))
    out = checked_out(who, "out", out, _I32, (b, a), match.device)
    nbytes = int(lib.mrcnn_sample_by_key_workspace_bytes(b))
    ws = workspace(nbytes, match.device)
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
    anchors = checked(who, "anchors", anchors, torch.float64, (("A", 1), 4), hint=_ANCHORS_HINT)
    gt_boxes = checked(who, "gt_boxes", gt_boxes, _F32, ("M", 4))
    gt_off = checked(who, "gt_off", gt_off, _I32, (("B+1", 2),))
    m, a, b, dev = gt_boxes.size(0), anchors.size(0), gt_off.numel() - 1, anchors.device
    match = checked(who, "match", match, _I32, (b, a))
    iou_argmax = checked(who, "iou_argmax", iou_argmax, _I32, (b, a))
    count = int(count)
    std = _target_std(who, std_dev)
    rpn_bbox = torch.empty(b, max(count, 0), 4, dtype=torch.float32, device=dev)
    num_pos = torch.empty(b, dtype=torch.int32, device=dev)
    nbytes = int(lib.mrcnn_rpn_deltas_workspace_bytes(b, a))
    ws = workspace(nbytes, dev)
    _launch(lib.mrcnn_rpn_deltas,
            (anchors.data_ptr(), a, _ptr0(gt_boxes), gt_off.data_ptr(), m, b, match.data_ptr(), iou_argmax.data_ptr(),
             count, (ctypes.c_double * 4)(*std), _ptr0(rpn_bbox), num_pos.data_ptr(), ws.data_ptr(), nbytes, _stream()),
            lambda: (0, (b, a, count), 2 * 4 * b * a + 16 * b * count, "rpn_deltas"))
    return rpn_bbox, num_pos


register("anchor_match(Tensor anchors, Tensor gt_boxes, Tensor gt_class_ids, Tensor gt_off, float neg_iou=0.3, float pos_iou=0.7, "
         "float crowd_iou=0.001) -> (Tensor, Tensor, Tensor, Tensor, Tensor)", anchor_match)
register("sample_by_key(Tensor match, Tensor keys, int count) -> Tensor", sample_by_key)   # `out` is the Python binding's
register("rpn_deltas(Tensor anchors, Tensor gt_boxes, Tensor gt_off, Tensor match, Tensor iou_argmax, int count, "
         "float[] std_dev) -> (Tensor, Tensor)", rpn_deltas)


# --------------------------------------------------------------------------------------------------
# Detection training targets: model.mrn_samples for a batch (csrc/detection_targets.hip)
# --------------------------------------------------------------------------------------------------
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
    rois = checked(who, "rois", rois, _F32, (("B", 1), ("N", 1), 4))
    b, n, dev = rois.size(0), rois.size(1), rois.device
    gt_boxes = checked(who, "gt_boxes", gt_boxes, _F32, ("M", 4))
    gt_off = checked(who, "gt_off", gt_off, _I32, (b + 1,), hint=f" for {b} images of rois")
    m = gt_boxes.size(0)
    gt_class_ids = checked(who, "gt_class_ids", gt_class_ids, _I32, (m,))
    keys = checked(who, "keys", keys, _I32, (b, n))
    count = int(count)
    std = _target_std(who, std_dev)
    c = max(count, 0)
    spec = (("rois_out", _F32, (b, c, 4)), ("target_class_ids", _I32, (b, c)), ("target_deltas", _F32, (b, c, 4)),
            ("roi_index", _I32, (b, c)), ("gt_index", _I32, (b, c)), ("num_pos", _I32, (b,)), ("num_neg", _I32, (b,)),
            ("status", _I32, (b,)))
    if out is not None and len(out) != len(spec):
        raise RuntimeError(f"{who}: out must hold {len(spec)} tensors ({', '.join(s[0] for s in spec)}), got {len(out)}")
    outs = tuple(checked_out(who, name, None if out is None else o, dtype, shape, dev) for (name, dtype, shape), o in zip(spec, out or spec))
    _launch(lib.mrcnn_detection_targets,
            (rois.data_ptr(), _ptr0(gt_boxes), _ptr0(gt_class_ids), gt_off.data_ptr(), keys.data_ptr(),
             b, n, m, count, float(positive_ratio), float(pos_iou), float(crowd_iou), (ctypes.c_float * 4)(*std),
             *[_ptr0(t) for t in outs], _stream()),
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
    gt_masks = checked(who, "gt_masks", gt_masks, (torch.uint8, torch.bool, _F32), ("M", "H", "W"))
    rois_out = checked(who, "rois_out", rois_out, _F32, (("B", 1), "count", 4))
    b, count, dev = rois_out.size(0), rois_out.size(1), rois_out.device
    gt_off = checked(who, "gt_off", gt_off, _I32, (b + 1,))
    gt_index = checked(who, "gt_index", gt_index, _I32, (b, count))
    num_pos = checked(who, "num_pos", num_pos, _I32, (b,))
    if len(mask_shape) != 2:
        raise RuntimeError(f"{who}: mask_shape must be (height, width), got {tuple(mask_shape)}")
    mh, mw = int(mask_shape[0]), int(mask_shape[1])
    m, h, w = gt_masks.shape
    out = checked_out(who, "target_mask", out, _F32, (b, count, max(mh, 0), max(mw, 0)), dev)
    fn = lib.mrcnn_mask_targets_f32 if gt_masks.dtype == _F32 else lib.mrcnn_mask_targets_u8
    _launch(fn, (_ptr0(gt_masks), m, h, w, gt_off.data_ptr(), b, count, _ptr0(rois_out), _ptr0(gt_index), num_pos.data_ptr(), mh, mw,
                 _ptr0(out), _stream()),
            lambda: (0, (b, count, mh * mw), 4 * b * count * mh * mw, "mask_targets"))
    return out


register("detection_targets(Tensor rois, Tensor gt_boxes, Tensor gt_class_ids, Tensor gt_off, Tensor keys, int count=100, "
         "float positive_ratio=0.33, float[] std_dev=[0.1, 0.1, 0.2, 0.2], float pos_iou=0.5, float crowd_iou=0.001) -> "
         "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)", detection_targets)   # `out` is the Python binding's
register("mask_targets(Tensor gt_masks, Tensor gt_off, Tensor rois_out, Tensor gt_index, Tensor num_pos, "
         "int[] mask_shape=[28, 28]) -> Tensor", mask_targets)


# --------------------------------------------------------------------------------------------------
# Training losses: the reference's five loss functions for a batch, forward and backward (csrc/losses.hip)
# --------------------------------------------------------------------------------------------------
def _rpn_loss_inputs(who, match, logits, pred_bbox, target_bbox):
    """The four tensors both RPN loss ops read, on 16-byte boundaries (the kernels read float4 rows), and B, A, count."""
    match = checked(who, "match", match, _I32, (("B", 1), ("A", 1)), align16=True)
    b, a = match.shape
    target_bbox = checked(who, "target_bbox", target_bbox, _F32, (b, ("count", 1), 4), align16=True)
    return (match, checked(who, "logits", logits, _F32, (b, a, 2), align16=True),
            checked(who, "pred_bbox", pred_bbox, _F32, (b, a, 4), align16=True), target_bbox, b, a, target_bbox.size(1))


def _loss_grad_out(who, grad_out, counts, losses: int):
    """grad_out float32 [losses] (the batch's mean) or [B,losses] (per image) → (grad_out, counts, per_image)."""
    counts = checked(who, "counts", counts, _I32, ("B", losses), hint=" as the forward returned them")
    per_image = isinstance(grad_out, torch.Tensor) and grad_out.dim() == 2
    shape = (counts.size(0), losses) if per_image else (losses,)
    return checked(who, "grad_out", grad_out, _F32, shape, hint=f" (or [{losses}]: the batch's mean)"), counts, per_image


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
    ws = workspace(nbytes, dev)
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
    chunk_pos = checked(who, "chunk_pos", chunk_pos, _I32, (b, max(int(lib.mrcnn_rpn_loss_chunks(a)), 1)), align16=True)
    grad_out, counts, per_image = _loss_grad_out(who, grad_out, counts, 2)
    grad_logits, grad_bbox = torch.empty_like(logits), torch.empty_like(pred_bbox)
    _launch(lib.mrcnn_rpn_loss_backward,
            (match.data_ptr(), logits.data_ptr(), pred_bbox.data_ptr(), target_bbox.data_ptr(), chunk_pos.data_ptr(),
             counts.data_ptr(), grad_out.data_ptr(), int(per_image), b, a, count, grad_logits.data_ptr(), grad_bbox.data_ptr(),
             _stream()),
            lambda: (0, (b, a, count), 28 * b * a, "rpn_loss_backward"))
    return grad_logits, grad_bbox


def _head_loss_inputs(who, target_class_ids, num_rois, target_deltas, target_mask, logits, pred_bbox, pred_masks):
    """The seven tensors both head loss ops read, on 16-byte boundaries, and B, count, C, mh, mw. target_mask and pred_masks both
    None: the classifier alone (the library takes null pointers for them; mh = mw = 1 stand in)."""
    ids = checked(who, "target_class_ids", target_class_ids, _I32, (("B", 1), ("count", 1)), align16=True)
    b, count = ids.shape
    no_masks = target_mask is None and pred_masks is None
    if not no_masks:
        target_mask = checked(who, "target_mask", target_mask, _F32, (b, count, "mh", "mw"), align16=True)
    logits = checked(who, "logits", logits, _F32, (b, count, ("C", 1)), align16=True)
    c, mh, mw = logits.size(2), (1 if no_masks else target_mask.size(2)), (1 if no_masks else target_mask.size(3))
    return (ids, checked(who, "num_rois", num_rois, _I32, (b,), align16=True),
            checked(who, "target_deltas", target_deltas, _F32, (b, count, 4), align16=True), target_mask, logits,
            checked(who, "pred_bbox", pred_bbox, _F32, (b, count, c, 4), align16=True),
            None if no_masks else checked(who, "pred_masks", pred_masks, _F32, (b, count, c, mh, mw), align16=True), b, count, c, mh, mw)


@_on_device
def head_loss(target_class_ids: torch.Tensor, num_rois: torch.Tensor, target_deltas: torch.Tensor, target_mask: torch.Tensor,
              logits: torch.Tensor, pred_bbox: torch.Tensor, pred_masks: torch.Tensor):
    """Classifier.class_loss, Classifier.boxes_loss and Mask.mask_loss (model.py:802-845, 922-953) for B images on the padded outputs
    of detection_targets; the rule is stated at mrcnn_rpn_loss_forward in include/maskrcnn_hip.h. target_class_ids int32 [B,count],
    num_rois int32 [B] (num_pos + num_neg: the slots past it never contribute), target_deltas float32 [B,count,4], target_mask
    float32 [B,count,mh,mw], logits float32 [B,count,C], pred_bbox float32 [B,count,C,4], pred_masks float32 [B,count,C,mh,mw] →
    (sums float64 [B,3]: class, box, mask; counts int32 [B,3]: the slots, 4 x the positive slots, mh x mw x the positive slots;
    status int32 [B]: bit 1 = a class id outside 0 .. C-1, whose slot is skipped). target_mask and pred_masks both None: the classifier
    alone — the mask sum and count are 0, the other columns and their bits unchanged. Two launches, no host synchronisation."""
    who = "head_loss"
    ids, num_rois, deltas, mask, logits, pred_bbox, pred_masks, b, count, c, mh, mw = _head_loss_inputs(
        who, target_class_ids, num_rois, target_deltas, target_mask, logits, pred_bbox, pred_masks)
    dev = ids.device
    sums = torch.empty(b, 3, dtype=torch.float64, device=dev)
    counts = torch.empty(b, 3, dtype=torch.int32, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    nbytes = int(lib.mrcnn_head_loss_workspace_bytes(b, count))
    ws = workspace(nbytes, dev)
    _launch(lib.mrcnn_head_loss_forward,
            (ids.data_ptr(), num_rois.data_ptr(), deltas.data_ptr(), _ptr(mask), logits.data_ptr(), pred_bbox.data_ptr(),
             _ptr(pred_masks), b, count, c, mh, mw, sums.data_ptr(), counts.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes,
             _stream()),
            lambda: (0, (b, count, c), 4 * b * count * (c + 2 * mh * mw + 10), "head_loss"))
    return sums, counts, status


@_on_device
def head_loss_backward(target_class_ids: torch.Tensor, num_rois: torch.Tensor, target_deltas: torch.Tensor, target_mask: torch.Tensor,
                       logits: torch.Tensor, pred_bbox: torch.Tensor, pred_masks: torch.Tensor, counts: torch.Tensor,
                       grad_out: torch.Tensor):
    """The gradients of head_loss's three losses → (grad_logits, grad_bbox, grad_masks) in the predictions' shapes, every element
    written: zeros but the contributing slots' logits rows, their class's box row and their class's mask plane. counts as
    head_loss returned them; grad_out float32 [3] (batch mean) or [B,3] (per image), as for rpn_loss_backward. Without the mask
    tensors (both None) grad_masks is None. One launch, no host synchronisation."""
    who = "head_loss_backward"
    ids, num_rois, deltas, mask, logits, pred_bbox, pred_masks, b, count, c, mh, mw = _head_loss_inputs(
        who, target_class_ids, num_rois, target_deltas, target_mask, logits, pred_bbox, pred_masks)
    grad_out, counts, per_image = _loss_grad_out(who, grad_out, counts, 3)
    grad_logits, grad_bbox = torch.empty_like(logits), torch.empty_like(pred_bbox)
    grad_masks = None if pred_masks is None else torch.empty_like(pred_masks)
    _launch(lib.mrcnn_head_loss_backward,
            (ids.data_ptr(), num_rois.data_ptr(), deltas.data_ptr(), _ptr(mask), logits.data_ptr(), pred_bbox.data_ptr(),
             _ptr(pred_masks), counts.data_ptr(), grad_out.data_ptr(), int(per_image), b, count, c, mh, mw,
             grad_logits.data_ptr(), grad_bbox.data_ptr(), _ptr(grad_masks), _stream()),
            lambda: (0, (b, count, c), 4 * b * count * c * (mh * mw + 5), "head_loss_backward"))
    return grad_logits, grad_bbox, grad_masks


register("rpn_loss(Tensor match, Tensor logits, Tensor pred_bbox, Tensor target_bbox) -> (Tensor, Tensor, Tensor, Tensor)", rpn_loss)
register("rpn_loss_backward(Tensor match, Tensor logits, Tensor pred_bbox, Tensor target_bbox, Tensor chunk_pos, Tensor counts, "
         "Tensor grad_out) -> (Tensor, Tensor)", rpn_loss_backward)
register("head_loss(Tensor target_class_ids, Tensor num_rois, Tensor target_deltas, Tensor target_mask, Tensor logits, "
         "Tensor pred_bbox, Tensor pred_masks) -> (Tensor, Tensor, Tensor)", head_loss)
register("head_loss_backward(Tensor target_class_ids, Tensor num_rois, Tensor target_deltas, Tensor target_mask, Tensor logits, "
         "Tensor pred_bbox, Tensor pred_masks, Tensor counts, Tensor grad_out) -> (Tensor, Tensor, Tensor)", head_loss_backward)



# --------------------------------------------------------------------------------------------------
# Backward of the pyramid RoIAlign to the four FPN maps (csrc/roi_align_backward.hip)
# --------------------------------------------------------------------------------------------------
def _map_sizes(who, map_sizes):
    """Four (H, W) pairs, or the same eight numbers in a row → [(H, W)] * 4."""
    try:
        flat = [int(v) for s in map_sizes for v in (s if isinstance(s, (list, tuple, torch.Size)) else (s,))]
    except TypeError:
        flat = []
    if len(flat) != 8 or min(flat) < 1:
        refuse(who, "map_sizes", "the (H, W) of the 4 levels P2..P5, each >= 1", map_sizes)
    return list(zip(flat[0::2], flat[1::2]))


@_on_device
def roi_align_pyramid_backward(grad_out: torch.Tensor, rois: torch.Tensor, pool: int, image_area: float, batch: int, map_sizes,
                               rois_per_image: int | None = None, roi_batch: torch.Tensor | None = None,
                               roi_counts: torch.Tensor | None = None, out=None):
    """The gradient of roi_align_pyramid's default output with respect to the four maps; the rule is stated at
    mrcnn_roi_align_pyramid_backward_f32 in include/maskrcnn_hip.h: per element the reference's crop_backward terms in a fixed
    order (RoI index, bin row, bin column, tap), so the bits equal the reference's CPU backward and two calls agree.
    grad_out float32 [R,pool,pool,C] (NHWC), rois float32 [R,4]; pool, image_area, rois_per_image, roi_batch int32 [R] and
    roi_counts int32 [R / rois_per_image] as the forward took them; batch and map_sizes = [(H_l, W_l)] * 4: the maps' shape →
    [grad_P2, .., grad_P5], each float32 [batch,H_l,W_l,C] with every element written (+0 where nothing lands). out: the four
    tensors to write into. Two launches, no floating-point atomic, no host synchronisation."""
    who = "roi_align_pyramid_backward"
    sizes = _map_sizes(who, map_sizes)
    pool, batch = int(pool), int(batch)
    if not 1 <= pool <= 1024:
        refuse(who, "pool", "in 1 .. 1024", pool)
    if batch < 1:
        refuse(who, "batch", ">= 1", batch)
    grad_out = checked(who, "grad_out", grad_out, _F32, ("R", pool, pool, "C"), align16=True)
    r, c, dev = grad_out.size(0), grad_out.size(3), grad_out.device
    if c < 4 or c % 4:
        refuse(who, "grad_out", f"float32 [R,{pool},{pool},C] with C a multiple of 4", grad_out)
    rois = checked(who, "rois", rois, _F32, (r, 4))
    roi_batch = checked(who, "roi_batch", roi_batch, _I32, (r,), optional=True)
    rpi = int(rois_per_image or 0)
    if roi_batch is None and rpi < 1:
        refuse(who, "rois_per_image", ">= 1 without roi_batch", rois_per_image)
    if roi_counts is not None:
        if roi_batch is not None or rpi < 1 or r % rpi:
            refuse(who, "roi_counts", f"None with roi_batch, or with R ({r}) no multiple of rois_per_image ({rois_per_image})", roi_counts)
        roi_counts = checked(who, "roi_counts", roi_counts, _I32, (r // rpi,))
    if out is not None and len(out) != 4:
        raise RuntimeError(f"{who}: out must hold 4 tensors (the gradients of P2..P5), got {len(out)}")
    grads = [checked_out(who, f"grad_P{l + 2}", None if out is None else out[l], _F32, (batch, h, w, c), dev)
             for l, (h, w) in enumerate(sizes)]
    nbytes = int(lib.mrcnn_roi_align_pyramid_backward_workspace_bytes(r))
    ws = workspace(nbytes, dev)
    _launch(lib.mrcnn_roi_align_pyramid_backward_f32,
            (_ptr0(grad_out), (c_i32 * 4)(*[h for h, _ in sizes]), (c_i32 * 4)(*[w for _, w in sizes]), batch, c, _ptr0(rois),
             _ptr(roi_batch), r, rpi, _ptr(roi_counts), pool, float(image_area), (c_vp * 4)(*[g.data_ptr() for g in grads]),
             ws.data_ptr(), nbytes, _stream()),
            lambda: (0, (r, pool * pool, c), 4 * c * (r * pool * pool + batch * sum(h * w for h, w in sizes)), "roi_align_pyramid_backward"))
    return grads


# roi_align_pyramid_backward has no torch.ops.maskrcnn schema and is not in ops.__all__, as rle_resample: tests/test_binding_host.py
# pins both lists to what was registered before it. It is reached as ops.roi_align_pyramid_backward.


# --------------------------------------------------------------------------------------------------
# Backward of the conv + frozen affine + activation, stride 1 or 2 (csrc/conv_backward.hip)
# --------------------------------------------------------------------------------------------------
ConvBackward = collections.namedtuple("ConvBackward", "dx dw dshift dresidual z")


def _backward_stride(who, stride) -> int:
    if type(stride) is not int or stride not in (1, 2):
        refuse(who, "stride", "1 or 2", stride)
    return stride


def conv_backward_chunk(b: int, h: int, w: int, cin: int, cout: int, kh: int, kw: int, pad=(0, 0, 0, 0), stride: int = 1) -> int:
    """The chunk length L of the weight gradient of this layer (mrcnn_conv_backward_weights_chunk): its pixel axis M = B*OH*OW is
    summed in ceil(M / L) fp32 chains that a second launch adds in fp64. A function of the shape only (the stride enters through OH
    and OW); host arithmetic."""
    pt, pl, pb, pr = [int(v) for v in pad]
    stride = _backward_stride("conv_backward_chunk", stride)
    got = int(lib.mrcnn_conv_backward_weights_chunk(int(b), int(h), int(w), int(cin), int(cout), int(kh), int(kw), stride, pt, pl, pb, pr))
    if got < 1:
        raise RuntimeError(f"conv_backward_chunk: the conv backward refuses these arguments ({lib.mrcnn_last_error().decode()})")
    return got


@_on_device
def conv_bn_act_backward(grad_out: torch.Tensor, x: torch.Tensor, w: torch.Tensor, y: torch.Tensor | None,
                         scale: torch.Tensor | None = None, pad=(0, 0, 0, 0), act: int = 0, res_div: int = 0, scatter: bool = False,
                         row_counts: torch.Tensor | None = None, rows_per_group: int = 0, needs=(True, True, True, False),
                         stride: int = 1):
    """The gradients of y = act(scale * conv(x, w) + shift (+ residual)) — conv_bn_act, or deconv2x2 with scatter=True
    (w [4*C,1,1,Cin], grad_out and y [B,2H,2W,C]) — for a FROZEN scale; the rule is stated at mrcnn_conv_act_backward_f32 in
    include/maskrcnn_hip.h. grad_out and y float32 in the output's shape (y is read only with an activation and may be None without),
    x float32 [B,H,W,Cin], w float32 [Cout,KH,KW,Cin], scale float32 [Cout] or None; pad, act (0 none, 1 ReLU, 2 sigmoid), row_counts
    and rows_per_group as the forward took them; res_div 0 (no residual), 1 or 2. needs = (dx, dw, dshift, dresidual) →
    ConvBackward(dx [B,H,W,Cin], dw as w, dshift [Cout], dresidual [B,OH/res_div,OW/res_div,Cout], z [B,OH,OW,roundup(Cout,4)]);
    entries not asked for are None (z: when neither dx nor dw is). No gradient of scale: BatchNorm is frozen. dx is the forward
    kernel on z bit for bit; dw is summed in chunks of conv_backward_chunk(...) pixels, then in fp64; dshift in fp64. Two calls give
    the same bits. Two launches per gradient, no floating-point atomic, no host synchronisation.
    stride 1 or 2 as the forward took it (the same entry points and the same rule, which the header states for both). At stride 2
    OH = (H + top + bottom - KH) // 2 + 1; dw and dshift are as above for any kernel size; dx is returned only for a 1x1 kernel
    without padding and is then the COMPACT gradient [B,OH,OW,Cin] — the values at the even positions of the full one, which
    ops.dilate2_sum writes out (adding a second compact gradient on the way). No row_counts and no scatter at stride 2."""
    who = "conv_bn_act_backward"
    stride = _backward_stride(who, stride)
    act, res_div, scatter, rpg = int(act), int(res_div), bool(scatter), int(rows_per_group)
    if len(needs) != 4:
        raise RuntimeError(f"{who}: needs must hold 4 flags (dx, dw, dshift, dresidual), got {len(needs)}")
    need_dx, need_dw, need_dshift, need_dres = [bool(v) for v in needs]
    if act not in (0, 1, 2):
        refuse(who, "act", "0 (none), 1 (ReLU) or 2 (sigmoid)", act)
    if res_div not in (0, 1, 2):
        refuse(who, "res_div", "0 (no residual), 1 or 2", res_div)
    if (res_div or scatter) and act == 2 or res_div and scatter:
        refuse(who, "act", "0 or 1 with a residual or the scatter, which do not combine either", act)
    if need_dres and not res_div:
        refuse(who, "needs", "without dresidual where res_div is 0", tuple(needs))
    x = checked(who, "x", x, _F32, (("B", 1), ("H", 1), ("W", 1), ("Cin", 4)), align16=True)
    b, h, wd, cin = x.shape
    if cin % 4:
        refuse(who, "x", "float32 [B,H,W,Cin] with Cin a multiple of 4", x)
    w = checked(who, "w", w, _F32, (("Cout", 1), ("KH", 1), ("KW", 1), cin), align16=True)
    cout, kh, kw, _ = w.shape
    pt, pl, pb, pr = [int(v) for v in pad]
    if scatter and (kh != 1 or kw != 1 or cout % 4 or (pt, pl, pb, pr) != (0, 0, 0, 0)):
        refuse(who, "w", f"float32 [4*C,1,1,{cin}] without padding for the scatter", w)
    if min(pt, pl, pb, pr) < 0 or max(pt, pb) > kh - 1 or max(pl, pr) > kw - 1:
        refuse(who, "pad", f"(top, left, bottom, right) in 0 .. kernel size - 1 = ({kh - 1}, {kw - 1})", (pt, pl, pb, pr))
    if h + pt + pb < kh or wd + pl + pr < kw:
        refuse(who, "x", f"float32 [B,H,W,Cin] no smaller than the {kh} x {kw} kernel with its padding", x)
    oh, ow = (h + pt + pb - kh) // stride + 1, (wd + pl + pr - kw) // stride + 1
    if stride == 2:
        if need_dx and (kh != 1 or kw != 1 or (pt, pl, pb, pr) != (0, 0, 0, 0)):
            refuse(who, "w", f"float32 [Cout,1,1,{cin}] without padding for a data gradient at stride 2 (needs[0])", w)
        if row_counts is not None:
            refuse(who, "row_counts", "None at stride 2", row_counts)
        if scatter:
            refuse(who, "scatter", "False at stride 2", scatter)
    out_shape = (b, 2 * h, 2 * wd, cout // 4) if scatter else (b, oh, ow, cout)
    grad_out = checked(who, "grad_out", grad_out, _F32, out_shape, align16=True)
    y = checked(who, "y", y, _F32, out_shape, optional=act == 0, align16=True)
    scale = checked(who, "scale", scale, _F32, (cout,), optional=True)
    m = b * oh * ow
    if row_counts is not None:
        if res_div or scatter or rpg < 1 or m % rpg:
            refuse(who, "row_counts", f"None with a residual or the scatter, or with rows_per_group ({rows_per_group}) not dividing the "
                   f"{m} output rows", row_counts)
        row_counts = checked(who, "row_counts", row_counts, _I32, (m // rpg,))
    if res_div == 2 and (oh % 2 or ow % 2):
        refuse(who, "res_div", f"1 for an odd output size ({oh} x {ow})", res_div)
    shape_args = (b, h, wd, cin, cout, kh, kw, stride, pt, pl, pb, pr)
    nbytes = int(lib.mrcnn_conv_backward_workspace_bytes(*shape_args))
    if nbytes < 1:
        raise RuntimeError(f"{who}: {lib.mrcnn_last_error().decode()}")
    dev, cout4, n = x.device, -(-cout // 4) * 4, kh * kw * cin
    ws = workspace(nbytes, dev)
    need_z = need_dx or need_dw
    alias = act == 0 and scale is None and row_counts is None and not scatter and cout % 4 == 0     # z is grad_out itself
    g_is_dy = act == 0 and row_counts is None
    z = g = dres2 = dshift = None
    if need_z:
        z = grad_out if alias else torch.empty(b, oh, ow, cout4, dtype=_F32, device=dev)
    if need_dres and res_div == 1:
        g = grad_out if g_is_dy else torch.empty(b, oh, ow, cout, dtype=_F32, device=dev)
    if need_dres and res_div == 2:
        dres2 = torch.empty(b, oh // 2, ow // 2, cout, dtype=_F32, device=dev)
    if need_dshift:
        dshift = torch.empty(cout, dtype=_F32, device=dev)
    z_out, g_out = (None if alias else z), (None if g_is_dy else g)
    if z_out is not None or g_out is not None or dres2 is not None or dshift is not None:
        _launch(lib.mrcnn_conv_act_backward_f32,
                (grad_out.data_ptr(), _ptr(y), b, oh, ow, cout, _ptr(scale), act, 2 if dres2 is not None else min(res_div, 1),
                 int(scatter), _ptr(row_counts), rpg, _ptr(z_out), _ptr(g_out), _ptr(dres2), _ptr(dshift), ws.data_ptr(), nbytes,
                 _stream()),
                lambda: (0, (m, cout, 1), 4 * m * (2 * cout + cout4), "conv_act_backward"))
    dx = dw = None
    if need_dx:
        dx = torch.empty((b, oh, ow, cin) if stride == 2 else (b, h, wd, cin), dtype=_F32, device=dev)   # stride 2: the compact one
        _launch(lib.mrcnn_conv_backward_data_f32,
                (z.data_ptr(), *shape_args[:4], w.data_ptr(), *shape_args[4:], dx.data_ptr(), ws.data_ptr(), nbytes, _stream()),
                lambda: (2.0 * m * n * cout, (dx.numel() // cin, cin, kh * kw * cout4), 4 * (m * cout4 + 2 * n * cout4 + dx.numel()),
                         "conv_backward_data"))
    if need_dw:
        dw = torch.empty(cout, kh, kw, cin, dtype=_F32, device=dev)
        chunks = -(-m // int(lib.mrcnn_conv_backward_weights_chunk(*shape_args)))
        _launch(lib.mrcnn_conv_backward_weights_f32,
                (x.data_ptr(), *shape_args[:4], z.data_ptr(), *shape_args[4:], _ptr(row_counts), rpg, dw.data_ptr(), ws.data_ptr(),
                 nbytes, _stream()),
                lambda: (2.0 * m * n * cout, (cout, n, m), 4 * (x.numel() + m * cout4 + (2 * chunks + 1) * n * cout),
                         "conv_backward_weights"))
    return ConvBackward(dx, dw, dshift, dres2 if res_div == 2 else g, z)


# conv_bn_act_backward has no torch.ops.maskrcnn schema and is not in ops.__all__ either, for the same reason. The differentiable
# front end is maskrcnn_amd.layers.


# --------------------------------------------------------------------------------------------------
# The backbone's other two gradients (csrc/pool_backward.hip)
# --------------------------------------------------------------------------------------------------
@_on_device
def dilate2_sum(a: torch.Tensor, b: torch.Tensor | None = None, height: int | None = None, width: int | None = None,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """The full gradient of a stride-2 1x1 conv (or of MaxPool2d(1, 2): P6) from the compact one; the rule is stated at
    mrcnn_dilate2_sum_f32 in include/maskrcnn_hip.h. a float32 [B,OH,OW,C] (C % 4 == 0), b the same shape or None, height and width
    of the full map with OH = ceil(height / 2), OW = ceil(width / 2) → out float32 [B,height,width,C]:
    out[:, 2i, 2j] = a[:, i, j] (+ b[:, i, j], one fp32 add), +0 everywhere else. Every byte of out is written once: no memset, no
    atomic. One launch, no host synchronisation."""
    who = "dilate2_sum"
    a = checked(who, "a", a, _F32, (("B", 1), ("OH", 1), ("OW", 1), ("C", 4)), align16=True)
    bb, oh, ow, c = a.shape
    if c % 4:
        refuse(who, "a", "float32 [B,OH,OW,C] with C a multiple of 4", a)
    b = checked(who, "b", b, _F32, (bb, oh, ow, c), optional=True, align16=True)
    if type(height) is not int or type(width) is not int or (height + 1) // 2 != oh or (width + 1) // 2 != ow:
        refuse(who, "(height, width)", f"two ints with ceil(height / 2) = {oh} and ceil(width / 2) = {ow}", (height, width))
    out = checked_out(who, "out", out, _F32, (bb, height, width, c), a.device)
    if out.data_ptr() % 16:
        refuse(who, "out", "on a 16-byte boundary", out)
    _launch(lib.mrcnn_dilate2_sum_f32, (a.data_ptr(), _ptr(b), bb, height, width, c, out.data_ptr(), _stream()),
            lambda: (0, (bb * height * width, c, 1), 4 * (out.numel() + a.numel() * (1 if b is None else 2)), "dilate2_sum"))
    return out


@_on_device
def maxpool_backward(grad_out: torch.Tensor, x: torch.Tensor, kernel: int, stride: int, pad=(0, 0, 0, 0),
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """The backward of ops.maxpool (zero padding, then the max) from the saved input; the rule is stated at mrcnn_maxpool_backward_f32
    in include/maskrcnn_hip.h: a window's gradient goes to its first maximum in (ky, kx) order, padding taps reading 0 — and is
    dropped where a padding tap is that maximum —, and an input element adds the gradients of its windows in ascending (oy, ox) order
    in fp32. x float32 [B,H,W,C] (C % 4 == 0), grad_out float32 [B,OH,OW,C], kernel 1 .. 3, stride 1 .. 2, pad = (top, left, bottom,
    right) each in 0 .. kernel - 1 → out float32 [B,H,W,C], every element written. One launch, no atomic, no host synchronisation."""
    who = "maxpool_backward"
    if type(kernel) is not int or not 1 <= kernel <= 3:
        refuse(who, "kernel", "an int in 1 .. 3", kernel)
    if type(stride) is not int or not 1 <= stride <= 2:
        refuse(who, "stride", "1 or 2", stride)
    try:
        pt, pl, pb, pr = pads = tuple(int(v) for v in pad)
    except (TypeError, ValueError):
        pads = None
    if pads is None or min(pads) < 0 or max(pads) > kernel - 1:
        refuse(who, "pad", f"(top, left, bottom, right) in 0 .. kernel - 1 = {kernel - 1}", pad)
    x = checked(who, "x", x, _F32, (("B", 1), ("H", 1), ("W", 1), ("C", 4)), align16=True)
    b, h, w, c = x.shape
    if c % 4:
        refuse(who, "x", "float32 [B,H,W,C] with C a multiple of 4", x)
    if h + pt + pb < kernel or w + pl + pr < kernel:
        refuse(who, "x", f"float32 [B,H,W,C] no smaller than the {kernel} x {kernel} window with its padding", x)
    oh, ow = (h + pt + pb - kernel) // stride + 1, (w + pl + pr - kernel) // stride + 1
    grad_out = checked(who, "grad_out", grad_out, _F32, (b, oh, ow, c), align16=True)
    out = checked_out(who, "out", out, _F32, (b, h, w, c), x.device)
    if out.data_ptr() % 16:
        refuse(who, "out", "on a 16-byte boundary", out)
    _launch(lib.mrcnn_maxpool_backward_f32,
            (grad_out.data_ptr(), x.data_ptr(), b, h, w, c, kernel, stride, pt, pl, pb, pr, out.data_ptr(), _stream()),
            lambda: (0, (b * h * w, c, kernel * kernel), 4 * (2 * x.numel() + grad_out.numel()), "maxpool_backward"))
    return out


# dilate2_sum and maxpool_backward have no torch.ops.maskrcnn schema and are not in ops.__all__ either, for the same reason. The
# differentiable front ends are maskrcnn_amd.layers.conv_bn_act(stride=2), .maxpool and .bottleneck.


# --------------------------------------------------------------------------------------------------
# Clipped SGD on a table of tensors (csrc/optim.hip)
# --------------------------------------------------------------------------------------------------
SGD_MODES = ("clip", "step", "step_zero")
_MAX_TENSORS, _MAX_TILES = 65535, 1 << 24


def _optim_table(who, table, tile_off, tiles):
    """table int64 [T,4] and tile_off int64 [T+1] of one call, T and the tile count. tiles=None reads tile_off[T] back from the
    device (a host synchronisation: the front end passes the number it built the table with)."""
    table = checked(who, "table", table, torch.int64, (("T", 1), 4), strides="refuse")
    t = table.size(0)
    if t > _MAX_TENSORS:
        refuse(who, "table", f"int64 [T,4] with T in 1 .. {_MAX_TENSORS}", table)
    tile_off = checked(who, "tile_off", tile_off, torch.int64, (t + 1,), strides="refuse", hint=f" for the {t} tensors of table")
    tiles = int(tile_off[-1]) if tiles is None else int(tiles)
    if not 0 <= tiles <= _MAX_TILES:
        refuse(who, "tiles", f"in 0 .. 2^24 (tile_off[T], {int(lib.mrcnn_optim_tile())} elements a tile)", tiles)
    return table, tile_off, t, tiles


def _finite(who, name, value, want="a finite number", ok=lambda v: True):
    try:
        v = float(value)
    except (TypeError, ValueError):
        refuse(who, name, want, value)
    if v != v or v in (float("inf"), float("-inf")) or not ok(v):
        refuse(who, name, want, value)
    return v


@_on_device
def grad_clip_coef(table: torch.Tensor, tile_off: torch.Tensor, max_norm: float, tiles: int | None = None):
    """Steps 1-3 of the clipped-SGD rule (stated at mrcnn_optim_clip_coef in include/maskrcnn_hip.h) on a device-resident tensor
    table: table int64 [T,4] = (address of p, address of g or 0, address of b, numel), tile_off int64 [T+1] = the prefix sum of
    ceil(numel / optim.TILE) → (info float64 [3] = (S, norm, c) with S the fp64 sum of g*g in a fixed order, norm = sqrt(S),
    c = min(1, max_norm / (norm + 1e-6)); status int32 [1], bit 0: S is not finite). tiles: tile_off[T] as the table's builder knows
    it (None reads it back from the device). The addresses must be live fp32 tensors of numel elements on this device: nothing here
    can check that (maskrcnn_amd.optim.ClippedSGD does, before every call). Two launches, no host synchronisation."""
    who = "grad_clip_coef"
    table, tile_off, t, tiles = _optim_table(who, table, tile_off, tiles)
    if not (isinstance(max_norm, (int, float)) and max_norm > 0):
        refuse(who, "max_norm", "a number above 0", max_norm)
    dev = table.device
    info = torch.empty(3, dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = workspace(8 * tiles, dev)
    _launch(lib.mrcnn_optim_clip_coef,
            (table.data_ptr(), tile_off.data_ptr(), t, tiles, float(max_norm), ws.data_ptr(), info.data_ptr(), status.data_ptr(),
             _stream()),
            lambda: (0, (t, tiles, 1), 4 * tiles * int(lib.mrcnn_optim_tile()), "optim_clip_coef"))
    return info, status


@_on_device
def sgd_apply(table: torch.Tensor, wd: torch.Tensor, tile_off: torch.Tensor, info: torch.Tensor | None, status: torch.Tensor | None,
              lr: float, momentum: float, mode, tiles: int | None = None) -> None:
    """Step 4 of the clipped-SGD rule in place on the table's tensors: per element in fp64 d = c g + wd p, B = momentum b + d,
    b' = fp32(B), p' = fp32(p - lr B), g' = fp32(c g). table and tile_off as for grad_clip_coef, wd float64 [T]; info and status as
    grad_clip_coef returned them (c and the non-finite flag are read on the device), or both None: c = 1 and no check. mode: "clip"
    (writes g'), "step" (p', b', g') or "step_zero" (p', b' and +0 into g), or 0 / 1 / 2. With status bit 0 set nothing is written
    but step_zero's zeros. The table lives on the device, so what it holds is the caller's to guarantee, as the addresses are:
    numel below 2^31 per tensor, every wd finite, tile_off the prefix sum of ceil(numel / optim.TILE) — optim.build_table checks all
    three on the host. One launch, no host synchronisation."""
    who = "sgd_apply"
    table, tile_off, t, tiles = _optim_table(who, table, tile_off, tiles)
    wd = checked(who, "wd", wd, torch.float64, (t,), strides="refuse")
    info = checked(who, "info", info, torch.float64, (3,), optional=True, strides="refuse")
    status = checked(who, "status", status, _I32, (1,), optional=True, strides="refuse")
    if (info is None) != (status is None):
        refuse(who, "status", "None exactly when info is None", status)
    lr = _finite(who, "lr", lr)
    momentum = _finite(who, "momentum", momentum, "a number in [0, 1)", lambda v: 0.0 <= v < 1.0)
    if mode in SGD_MODES:
        mode = SGD_MODES.index(mode)
    if type(mode) is not int or not 0 <= mode < len(SGD_MODES):
        refuse(who, "mode", 'one of "clip", "step", "step_zero" (0, 1, 2)', mode)
    per_element = (8, 24, 24)[mode]      # bytes read + written per element, worst case: step's store of g' is left out when c == 1
    _launch(lib.mrcnn_optim_sgd_apply,
            (table.data_ptr(), wd.data_ptr(), tile_off.data_ptr(), t, tiles, _ptr(info), _ptr(status), lr, momentum, mode, _stream()),
            lambda: (0, (t, tiles, 1), per_element * tiles * int(lib.mrcnn_optim_tile()), "optim_sgd_apply"))


# grad_clip_coef and sgd_apply have no torch.ops.maskrcnn schema and are not in ops.__all__ either, for the same reason. The front
# end, which builds the table and keeps its pointers current, is maskrcnn_amd.optim.ClippedSGD.


# --------------------------------------------------------------------------------------------------
# The RPN's training branch on the sampled anchors: compaction, patch gather, patch scatter (csrc/rpn_train.hip)
# --------------------------------------------------------------------------------------------------
_MAX_LEVELS, _MAX_SIDE, _MAX_APL, _MAX_CAPACITY, _MAX_IMAGES, _MAX_ELEMENTS = 8, 16384, 16, 1024, 65535, 1 << 30


def _int_in(who, name, value, lo, hi) -> int:
    if type(value) is not int or not lo <= value <= hi:
        refuse(who, name, f"an int in {lo} .. {hi}", value)
    return value


def _pyramid_sizes(who, sizes, apl: int):
    """[(H_l, W_l)] of 1 .. 8 levels, each side in 1 .. 16384 → (the list, A = the number of anchors, below 2^31)."""
    try:
        sizes = [(int(h), int(w)) for h, w in sizes]
    except (TypeError, ValueError):
        sizes = []
    if not 1 <= len(sizes) <= _MAX_LEVELS or min(min(s) for s in sizes) < 1 or max(max(s) for s in sizes) > _MAX_SIDE:
        refuse(who, "map_sizes", f"the (H, W) of 1 .. {_MAX_LEVELS} levels, each side in 1 .. {_MAX_SIDE}", sizes)
    a = apl * sum(h * w for h, w in sizes)
    if a >= 1 << 31:
        refuse(who, "map_sizes", "levels of fewer than 2^31 anchors in all", sizes)
    return sizes, a


def _index_and_num(who, index, num):
    index = checked(who, "index", index, _I32, (("B", 1), ("K", 1)), hint=" as anchor_compact returned it")
    b, k = index.shape
    if b > _MAX_IMAGES or k > _MAX_CAPACITY:
        refuse(who, "index", f"int32 [B,K] with B in 1 .. {_MAX_IMAGES} and K in 1 .. {_MAX_CAPACITY}", index)
    return index, checked(who, "num", num, _I32, (b,), hint=" as anchor_compact returned it"), b, k


def _level_args(sizes):
    pad = [1] * (_MAX_LEVELS - len(sizes))
    return (c_i32 * _MAX_LEVELS)(*[h for h, _ in sizes], *pad), (c_i32 * _MAX_LEVELS)(*[w for _, w in sizes], *pad)


def _level_ptrs(tensors):
    return (c_vp * _MAX_LEVELS)(*[_ptr(t) for t in tensors], *[None] * (_MAX_LEVELS - len(tensors)))


@_on_device
def anchor_compact(match: torch.Tensor, count: int):
    """match int32 [B,A] (rpn_match as sample_by_key leaves it) → (index int32 [B,count]: an image's anchors with match != 0 in
    ascending anchor index, -1 in the slots at or past num; num int32 [B] = min(count, their number); status int32 [B], bit 0: the
    image has more than count such anchors, of which the first count are kept). The rule is stated at mrcnn_anchor_compact in
    include/maskrcnn_hip.h. count in 1 .. 1024, B in 1 .. 65535, B * A < 2^31. One launch, no host synchronisation."""
    who = "anchor_compact"
    match = checked(who, "match", match, _I32, (("B", 1), ("A", 1)))
    b, a = match.shape
    if b > _MAX_IMAGES or b * a >= 1 << 31:
        refuse(who, "match", f"int32 [B,A] with B in 1 .. {_MAX_IMAGES} and B * A < 2^31", match)
    count = _int_in(who, "count", count, 1, _MAX_CAPACITY)
    dev = match.device
    index = torch.empty(b, count, dtype=_I32, device=dev)
    num = torch.empty(b, dtype=_I32, device=dev)
    status = torch.empty(b, dtype=_I32, device=dev)
    _launch(lib.mrcnn_anchor_compact, (match.data_ptr(), b, a, count, index.data_ptr(), num.data_ptr(), status.data_ptr(), _stream()),
            lambda: (0, (b, a, count), 4 * b * (a + count), "anchor_compact"))
    return index, num, status


@_on_device
def pyramid_patch_gather(maps, index: torch.Tensor, num: torch.Tensor, anchors_per_location: int = 3,
                         out: torch.Tensor | None = None) -> torch.Tensor:
    """The 3x3xC input patches of the sampled anchors, as GEMM rows; the rule is stated at mrcnn_pyramid_patch_gather_f32 in
    include/maskrcnn_hip.h. maps: 1 .. 8 float32 NHWC tensors [B,H_l,W_l,C] (C % 4 == 0), index int32 [B,K] and num int32 [B] as
    anchor_compact returned them → patches float32 [B*K,9*C]: row (b, k) holds map_l[b, py+ky-1, px+kx-1, c] at (ky*3+kx)*C + c for
    the pixel (py, px) and level l of anchor index[b,k] — the flattening of an OHWI weight —, +0 for a tap outside the map and for
    every tap of an empty slot (k >= num[b], or an index outside the pyramid). A copy: bit exact; every byte of out is written. One
    launch, no host synchronisation."""
    who = "pyramid_patch_gather"
    if not isinstance(maps, (list, tuple)) or not 1 <= len(maps) <= _MAX_LEVELS:
        refuse(who, "maps", f"a list of 1 .. {_MAX_LEVELS} float32 [B,H,W,C] tensors", maps if isinstance(maps, torch.Tensor) else type(maps).__name__)
    apl = _int_in(who, "anchors_per_location", anchors_per_location, 1, _MAX_APL)
    index, num, b, k = _index_and_num(who, index, num)
    first = checked(who, "maps[0]", maps[0], _F32, (b, ("H", 1), ("W", 1), ("C", 4)), align16=True)
    c = first.size(3)
    if c % 4:
        refuse(who, "maps[0]", "float32 [B,H,W,C] with C a multiple of 4", first)
    maps = [first] + [checked(who, f"maps[{l}]", m, _F32, (b, ("H", 1), ("W", 1), c), align16=True) for l, m in enumerate(maps) if l]
    sizes, _ = _pyramid_sizes(who, [(m.size(1), m.size(2)) for m in maps], apl)
    for l, m in enumerate(maps):
        if m.numel() > _MAX_ELEMENTS:
            refuse(who, f"maps[{l}]", "float32 [B,H,W,C] of at most 2^30 elements", m)
    if 9 * c * k * b > _MAX_ELEMENTS:
        refuse(who, "index", f"int32 [B,K] with B * K * 9 * C ({b} * {k} * 9 * {c}) at most 2^30", index)
    out = checked_out(who, "out", out, _F32, (b * k, 9 * c), first.device)
    if out.data_ptr() % 16:
        refuse(who, "out", "on a 16-byte boundary", out)
    hs, ws = _level_args(sizes)
    _launch(lib.mrcnn_pyramid_patch_gather_f32,
            (_level_ptrs(maps), hs, ws, len(maps), b, c, apl, index.data_ptr(), num.data_ptr(), k, out.data_ptr(), _stream()),
            lambda: (0, (b * k, 9 * c, 1), 8 * out.numel(), "pyramid_patch_gather"))
    return out


@_on_device
def pyramid_patch_scatter(dpatch: torch.Tensor, index: torch.Tensor, num: torch.Tensor, map_sizes, channels: int,
                          anchors_per_location: int = 3, needs=None, out=None):
    """The backward of pyramid_patch_gather; the rule is stated at mrcnn_pyramid_patch_scatter_f32 in include/maskrcnn_hip.h.
    dpatch float32 [B*K,9*C], index int32 [B,K] and num int32 [B] as the gather took them, map_sizes = [(H_l, W_l)] of the 1 .. 8
    levels, channels = C → [grad_l float32 [B,H_l,W_l,C]]: per element the fp32 sum from +0, in ascending slot k < num[b], of
    dpatch[b,k,y-py+1,x-px+1,c] over the entries of level l within one pixel of (y, x). needs: one flag per level (None: all); a
    level that is not needed is None in the result and costs nothing. out: the tensors to write into (an entry of a level that is
    not needed is ignored). Every byte of every returned map is written; no memset, no atomic; two calls give the same bits; index
    must be ascending within num[b], as anchor_compact writes it. One launch, no host synchronisation."""
    who = "pyramid_patch_scatter"
    apl = _int_in(who, "anchors_per_location", anchors_per_location, 1, _MAX_APL)
    if type(channels) is not int or channels < 4 or channels % 4:
        refuse(who, "channels", "an int, a multiple of 4", channels)
    index, num, b, k = _index_and_num(who, index, num)
    sizes, _ = _pyramid_sizes(who, map_sizes, apl)
    if 9 * channels * k * b > _MAX_ELEMENTS:
        refuse(who, "index", f"int32 [B,K] with B * K * 9 * C ({b} * {k} * 9 * {channels}) at most 2^30", index)
    dpatch = checked(who, "dpatch", dpatch, _F32, (b * k, 9 * channels), align16=True)
    needs = [True] * len(sizes) if needs is None else [bool(v) for v in needs]
    if len(needs) != len(sizes):
        raise RuntimeError(f"{who}: needs must hold {len(sizes)} flags (one per level), got {len(needs)}")
    if out is not None and len(out) != len(sizes):
        raise RuntimeError(f"{who}: out must hold {len(sizes)} tensors (one per level), got {len(out)}")
    dev, grads = dpatch.device, []
    for l, (h, w) in enumerate(sizes):
        if b * h * w * channels > _MAX_ELEMENTS:
            refuse(who, "map_sizes", f"levels of at most 2^30 elements each (level {l}: {b} * {h} * {w} * {channels})", sizes)
        g = checked_out(who, f"grad_{l}", None if out is None else out[l], _F32, (b, h, w, channels), dev) if needs[l] else None
        if g is not None and g.data_ptr() % 16:
            refuse(who, f"grad_{l}", "on a 16-byte boundary", g)
        grads.append(g)
    hs, ws = _level_args(sizes)
    _launch(lib.mrcnn_pyramid_patch_scatter_f32,
            (dpatch.data_ptr(), hs, ws, len(sizes), b, channels, apl, index.data_ptr(), num.data_ptr(), k, _level_ptrs(grads), _stream()),
            lambda: (0, (b * k, 9 * channels, 1), 4 * (dpatch.numel() + sum(g.numel() for g in grads if g is not None)),
                     "pyramid_patch_scatter"))
    return grads


# anchor_compact, pyramid_patch_gather and pyramid_patch_scatter have no torch.ops.maskrcnn schema and are not in ops.__all__
# either, for the same reason. The differentiable front end is maskrcnn_amd.rpn_train (pyramid_patches, TrainableRPN).


# --------------------------------------------------------------------------------------------------
# The mask head's class-plane branch in training (csrc/mask_train.hip)
# --------------------------------------------------------------------------------------------------
_MAX_CLASSES, _MAX_MASK_SIDE, _MAX_CIN = 4096, 64, 4096


def _plane_targets(who, ids, num, slots, classes=None):
    """target_class_ids int32 [B,count] and num int32 [B] of a class-plane op, with B, count and the checked P and C."""
    ids = checked(who, "ids", ids, _I32, (("B", 1), ("count", 1)))
    b, count = ids.shape
    if b > _MAX_IMAGES or count > _MAX_CAPACITY:
        refuse(who, "ids", f"int32 [B,count] with B in 1 .. {_MAX_IMAGES} and count in 1 .. {_MAX_CAPACITY}", ids)
    num = checked(who, "num", num, _I32, (b,))
    if type(slots) is not int or not 1 <= slots <= count:
        refuse(who, "plane slots P", f"in 1 .. count = {count}", slots)
    if classes is not None:
        _int_in(who, "num_classes", classes, 2, _MAX_CLASSES)
    return ids, num, b, count


def _plane_act(who, act) -> int:
    if type(act) is not int or act not in (0, 2):
        refuse(who, "act", "0 (none) or 2 (sigmoid)", act)
    return act


def _plane_x(who, name, x, optional=False):
    """x (or dx) float32 [S,mh,mw,Cin] of a class-plane op → (x, mh, mw, Cin)."""
    x = checked(who, name, x, _F32, (("S", 1), ("mh", 1), ("mw", 1), ("Cin", 4)), align16=True, optional=optional)
    if x is None:
        return None, 0, 0, 0
    _, mh, mw, cin = x.shape
    if cin % 4 or cin > _MAX_CIN or mh > _MAX_MASK_SIDE or mw > _MAX_MASK_SIDE:
        refuse(who, name, f"float32 [S,mh,mw,Cin] with mh, mw in 1 .. {_MAX_MASK_SIDE} and Cin a multiple of 4 in 4 .. {_MAX_CIN}", x)
    return x, mh, mw, cin


@_on_device
def class_plane_conv(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None, ids: torch.Tensor, num: torch.Tensor, act: int = 0,
                     out: torch.Tensor | None = None):
    """The 1x1 conv to each slot's OWN class; the rule is stated at mrcnn_class_plane_conv_f32 in include/maskrcnn_hip.h. x float32
    [B*P,mh,mw,Cin] (NHWC: the first P slots of each image), w float32 [C,Cin], bias float32 [C] or None, ids int32 [B,count]
    (target_class_ids, read in place), num int32 [B] → (y float32 [B*P,mh,mw], status int32 [B]). Slot (b, s) is active when
    s < min(num[b], P) and 0 < ids[b,s] < C: y = act(bias[k] + x . w[k]) with the dot product in fp64, act 0 none / 2 sigmoid. A slot
    that is not active: +0, and its x rows are never read. status bit 1: a class id outside 0 .. C-1 below num[b]; bit 2: a positive at
    or past P. Every byte of y is written. One launch, no host synchronisation."""
    who = "class_plane_conv"
    act = _plane_act(who, act)
    x, mh, mw, cin = _plane_x(who, "x", x)
    w = checked(who, "w", w, _F32, (("C", 2), cin), align16=True)
    c = w.size(0)
    bias = checked(who, "bias", bias, _F32, (c,), optional=True)
    s = x.size(0)
    b = ids.size(0) if isinstance(ids, torch.Tensor) and ids.dim() == 2 and ids.size(0) else 1
    ids, num, b, count = _plane_targets(who, ids, num, s // b if s % b == 0 else 0, c)
    out = checked_out(who, "out", out, _F32, (s, mh, mw), x.device)
    status = torch.empty(b, dtype=_I32, device=x.device)
    _launch(lib.mrcnn_class_plane_conv_f32,
            (x.data_ptr(), w.data_ptr(), _ptr(bias), ids.data_ptr(), num.data_ptr(), b, count, s // b, c, mh, mw, cin, act,
             out.data_ptr(), status.data_ptr(), _stream()),
            lambda: (2.0 * s * mh * mw * cin, (s * mh * mw, 1, cin), 4 * (x.numel() + out.numel()), "class_plane_conv"))
    return out, status


@_on_device
def class_plane_conv_backward(dy: torch.Tensor, y: torch.Tensor | None, x: torch.Tensor, w: torch.Tensor, ids: torch.Tensor,
                              num: torch.Tensor, act: int = 0, needs=(True, True, True), out=None):
    """The gradients of class_plane_conv; the rule is stated at mrcnn_class_plane_conv_backward_f32 in include/maskrcnn_hip.h. dy and
    y float32 [B*P,mh,mw] (y is read at act 2 only and may be None at act 0), x, w, ids, num and act as the forward took them;
    needs = (dx, dw, dbias) → (dx float32 [B*P,mh,mw,Cin], dw float32 [C,Cin], dbias float32 [C]), None where not needed. dx is one
    fp32 product g * w[k]; dw and dbias are fp64 sums in a fixed order (the pixels of a slot, then the slots of a class in ascending
    (b, s)), narrowed last. Every byte of every returned tensor is written, +0 for a slot that is not active and for a class without
    one; two calls give the same bits. out: the three tensors to write into (an entry that is not needed is ignored). Two launches (one
    for dx alone), no floating-point atomic, no host synchronisation."""
    who = "class_plane_conv_backward"
    act = _plane_act(who, act)
    if len(needs) != 3:
        raise RuntimeError(f"{who}: needs must hold 3 flags (dx, dw, dbias), got {len(needs)}")
    if out is not None and len(out) != 3:
        raise RuntimeError(f"{who}: out must hold 3 tensors (dx, dw, dbias), got {len(out)}")
    need_dx, need_dw, need_db = [bool(v) for v in needs]
    x, mh, mw, cin = _plane_x(who, "x", x)
    s, dev = x.size(0), x.device
    w = checked(who, "w", w, _F32, (("C", 2), cin), align16=True)
    c = w.size(0)
    dy = checked(who, "dy", dy, _F32, (s, mh, mw))
    y = checked(who, "y", y, _F32, (s, mh, mw), optional=act == 0)
    b = ids.size(0) if isinstance(ids, torch.Tensor) and ids.dim() == 2 and ids.size(0) else 1
    ids, num, b, count = _plane_targets(who, ids, num, s // b if s % b == 0 else 0, c)
    given = out or (None, None, None)
    dx = checked_out(who, "dx", given[0], _F32, (s, mh, mw, cin), dev) if need_dx else None
    dw = checked_out(who, "dw", given[1], _F32, (c, cin), dev) if need_dw else None
    db = checked_out(who, "dbias", given[2], _F32, (c,), dev) if need_db else None
    if dx is not None and dx.data_ptr() % 16:
        refuse(who, "dx", "on a 16-byte boundary", dx)
    nbytes = int(lib.mrcnn_class_plane_conv_backward_workspace_bytes(b, s // b, mh, mw, cin)) if need_dw or need_db else 0
    ws = workspace(nbytes, dev)
    _launch(lib.mrcnn_class_plane_conv_backward_f32,
            (dy.data_ptr(), _ptr(y), x.data_ptr(), w.data_ptr(), ids.data_ptr(), num.data_ptr(), b, count, s // b, c, mh, mw, cin, act,
             _ptr(dx), _ptr(dw), _ptr(db), ws.data_ptr(), nbytes, _stream()),
            lambda: (2.0 * s * mh * mw * cin * (need_dx + need_dw), (s * mh * mw, 1, cin),
                     4 * x.numel() * (need_dx + need_dw) + 2 * nbytes, "class_plane_conv_backward"))
    return dx, dw, db


def _plane_loss_inputs(who, p, target_mask, ids, num):
    p = checked(who, "p", p, _F32, (("B", 1), ("P", 1), ("mh", 1), ("mw", 1)))
    b, slots, mh, mw = p.shape
    if mh > _MAX_MASK_SIDE or mw > _MAX_MASK_SIDE:
        refuse(who, "p", f"float32 [B,P,mh,mw] with mh, mw in 1 .. {_MAX_MASK_SIDE}", p)
    ids = checked(who, "ids", ids, _I32, (b, ("count", 1)))
    ids, num, b, count = _plane_targets(who, ids, num, slots)
    return p, checked(who, "target_mask", target_mask, _F32, (b, count, mh, mw)), ids, num, b, count, slots, mh, mw


@_on_device
def mask_plane_loss(p: torch.Tensor, target_mask: torch.Tensor, ids: torch.Tensor, num: torch.Tensor, num_classes: int):
    """Mask.mask_loss (model.py:922-953) on class planes; the rule is stated at mrcnn_mask_plane_loss_forward in
    include/maskrcnn_hip.h. p float32 [B,P,mh,mw] (class_plane_conv's sigmoid output), target_mask float32 [B,count,mh,mw], ids int32
    [B,count] and num int32 [B] read in place, num_classes = C → (sums float64 [B], counts int32 [B] = mh * mw x the active slots,
    status int32 [B] as class_plane_conv's). The per-element term and the order of a slot's sum are ops.head_loss's: the sums equal its
    mask column on the dense tensor bit for bit. Two launches, no host synchronisation."""
    who = "mask_plane_loss"
    p, target_mask, ids, num, b, count, slots, mh, mw = _plane_loss_inputs(who, p, target_mask, ids, num)
    c = _int_in(who, "num_classes", num_classes, 2, _MAX_CLASSES)
    dev = p.device
    sums = torch.empty(b, dtype=torch.float64, device=dev)
    counts = torch.empty(b, dtype=_I32, device=dev)
    status = torch.empty(b, dtype=_I32, device=dev)
    nbytes = int(lib.mrcnn_mask_plane_loss_workspace_bytes(b, slots))
    ws = workspace(nbytes, dev)
    _launch(lib.mrcnn_mask_plane_loss_forward,
            (p.data_ptr(), target_mask.data_ptr(), ids.data_ptr(), num.data_ptr(), b, count, slots, c, mh, mw, sums.data_ptr(),
             counts.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes, _stream()),
            lambda: (0, (b, slots, mh * mw), 8 * p.numel(), "mask_plane_loss"))
    return sums, counts, status


@_on_device
def mask_plane_loss_backward(p: torch.Tensor, target_mask: torch.Tensor, ids: torch.Tensor, num: torch.Tensor, num_classes: int,
                             counts: torch.Tensor, grad_out: torch.Tensor, per_image: bool = False,
                             out: torch.Tensor | None = None) -> torch.Tensor:
    """The gradient of mask_plane_loss's loss → grad_p float32 [B,P,mh,mw], every byte written, +0 for a slot that is not active.
    counts as mask_plane_loss returned them; grad_out float32 [1] (the upstream gradient of the batch's sum / the batch's count) or,
    with per_image, [B] (of each image's own sum / count), both read on the device. One launch, no host synchronisation."""
    who = "mask_plane_loss_backward"
    p, target_mask, ids, num, b, count, slots, mh, mw = _plane_loss_inputs(who, p, target_mask, ids, num)
    c = _int_in(who, "num_classes", num_classes, 2, _MAX_CLASSES)
    counts = checked(who, "counts", counts, _I32, (b,), hint=" as the forward returned them")
    per_image = bool(per_image)
    grad_out = checked(who, "grad_out", grad_out, _F32, (b,) if per_image else (1,))
    out = checked_out(who, "out", out, _F32, (b, slots, mh, mw), p.device)
    _launch(lib.mrcnn_mask_plane_loss_backward,
            (p.data_ptr(), target_mask.data_ptr(), ids.data_ptr(), num.data_ptr(), counts.data_ptr(), grad_out.data_ptr(), int(per_image),
             b, count, slots, c, mh, mw, out.data_ptr(), _stream()),
            lambda: (0, (b, slots, mh * mw), 12 * p.numel(), "mask_plane_loss_backward"))
    return out


# class_plane_conv, class_plane_conv_backward, mask_plane_loss and mask_plane_loss_backward have no torch.ops.maskrcnn schema and are
# not in ops.__all__ either, for the same reason. The differentiable front end is maskrcnn_amd.head_train.
