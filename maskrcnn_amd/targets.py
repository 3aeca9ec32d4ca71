"""RPN training targets for a batch of images: the reference's data.rpn_samples (data.py:449-591, called per item at
data.py:727) — anchor matching, subsampling, regression deltas — on the device (csrc/targets.hip).

    rpn_match, rpn_bbox = rpn_targets(anchors.pyramid_anchors(cfg, dtype=torch.float64), gt_boxes, gt_class_ids)

The rule is stated at mrcnn_anchor_match in include/maskrcnn_hip.h. One thing differs from the reference by design: where it
draws the anchors to reset with np.random.choice, here every anchor has a key and the ones with the smallest (key, anchor index)
stay; independent uniform keys (the default: drawn on the device) give the same distribution, given keys a reproducible result.

device="cpu" runs the same rule in numpy, without the library's kernels (match_numpy / sample_numpy / deltas_numpy below): the
fixtures' generator and a user without a GPU read it, and it is what the device results are compared with.
"""
from __future__ import annotations

import numpy as np
import torch

__all__ = ["rpn_targets", "match_numpy", "sample_numpy", "deltas_numpy", "MAX_ROWS_PER_IMAGE"]

MAX_ROWS_PER_IMAGE = 1024      # an image's boxes are staged in LDS (the reference caps at MAX_GT_INSTANCES = 50)
NEG_IOU, POS_IOU, CROWD_IOU = 0.3, 0.7, 0.001


# ----------------------------------------------------------------------------------------------------------------------
# The rule in numpy, one image at a time
# ----------------------------------------------------------------------------------------------------------------------
def _overlaps(a32: np.ndarray, g32: np.ndarray) -> np.ndarray:
    """boxes_overlaps (data.py:151-189): fp32 [A,G], every operation rounded on its own."""
    a, g = a32[:, None, :], g32[None, :, :]
    y1, x1 = np.maximum(a[..., 0], g[..., 0]), np.maximum(a[..., 1], g[..., 1])
    y2, x2 = np.minimum(a[..., 2], g[..., 2]), np.minimum(a[..., 3], g[..., 3])
    zero = np.float32(0)
    inter = np.maximum(x2 - x1, zero) * np.maximum(y2 - y1, zero)
    a_area = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    g_area = (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        return (inter / ((a_area + g_area) - inter)).astype(np.float32)


def match_numpy(anchors, gt_boxes, gt_class_ids, neg_iou=NEG_IOU, pos_iou=POS_IOU, crowd_iou=CROWD_IOU):
    """Steps 1-6 for one image → (match int32 [A], iou_argmax int32 [A], iou_max float32 [A], gt_argmax int32 [G], status int).
    Row indices count all of the image's rows; status bit 0: no kept row (match 0, iou_argmax -1, iou_max 0)."""
    a32 = np.asarray(anchors, np.float64).astype(np.float32)
    boxes = np.asarray(gt_boxes, np.float32).reshape(-1, 4)
    ids = np.asarray(gt_class_ids, np.int32).reshape(-1)
    n = a32.shape[0]
    crowd = np.where(ids < 0)[0]
    kept = np.where(ids > 0)[0] if crowd.size else np.arange(ids.size)
    match = np.zeros(n, np.int32)
    gt_argmax = np.full(ids.size, -1, np.int32)
    if kept.size == 0:
        return match, np.full(n, -1, np.int32), np.zeros(n, np.float32), gt_argmax, 1
    no_crowd = np.ones(n, bool)
    if crowd.size:
        no_crowd = _overlaps(a32, boxes[crowd]).max(axis=1) < np.float32(crowd_iou)
    ov = _overlaps(a32, boxes[kept])
    arg = np.argmax(ov, axis=1)
    iou_max = ov[np.arange(n), arg]
    match[(iou_max < np.float32(neg_iou)) & no_crowd] = -1
    col = np.argmax(ov, axis=0)
    match[col] = 1
    match[iou_max >= np.float32(pos_iou)] = 1
    gt_argmax[kept] = col
    return match, kept[arg].astype(np.int32), iou_max, gt_argmax, 0


def sample_numpy(match, keys, count: int) -> np.ndarray:
    """Steps 7-8 for one image: the positives (then the negatives) with the largest (key, anchor index) are reset to 0."""
    match = np.array(match, np.int32)
    keys = np.asarray(keys)
    for value, limit in ((1, lambda: count // 2), (-1, lambda: count - int(np.sum(match == 1)))):
        ids = np.where(match == value)[0]
        extra = len(ids) - limit()
        if extra > 0:
            match[ids[np.lexsort((ids, keys[ids]))[len(ids) - extra:]]] = 0
    return match


def deltas_numpy(anchors, gt_boxes, match, iou_argmax, count: int, std_dev=(0.1, 0.1, 0.2, 0.2)):
    """Step 9 for one image, the reference's expressions on the reference's types (NumPy >= 2 promotion: the box side and centre
    stay float32, the anchor's are float64) → (rpn_bbox float32 [count,4], number of positives)."""
    anchors = np.asarray(anchors, np.float64)
    boxes = np.asarray(gt_boxes, np.float32).reshape(-1, 4)
    out = np.zeros((count, 4))
    std = np.asarray(std_dev, np.float64)
    ids = np.where(np.asarray(match) == 1)[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        for ix, i in enumerate(ids[:count]):
            a, gt = anchors[i], boxes[iou_argmax[i]]
            gt_h, gt_w = gt[2] - gt[0], gt[3] - gt[1]
            gt_center_y, gt_center_x = gt[0] + 0.5 * gt_h, gt[1] + 0.5 * gt_w
            a_h, a_w = a[2] - a[0], a[3] - a[1]
            a_center_y, a_center_x = a[0] + 0.5 * a_h, a[1] + 0.5 * a_w
            out[ix] = [(gt_center_y - a_center_y) / a_h, (gt_center_x - a_center_x) / a_w, np.log(gt_h / a_h), np.log(gt_w / a_w)]
            out[ix] /= std
        return out.astype(np.float32), len(ids)


# ----------------------------------------------------------------------------------------------------------------------
# Front end
# ----------------------------------------------------------------------------------------------------------------------
def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _on_gpu(x) -> bool:
    return isinstance(x, torch.Tensor) and x.is_cuda


def _check_anchors(a: np.ndarray) -> None:
    if a.ndim != 2 or a.shape[1] != 4 or a.shape[0] < 1:
        raise ValueError(f"rpn_targets: anchors must be [A,4] with A >= 1, got {a.shape}")
    if not np.isfinite(a).all() or not (((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])) > 0).all():
        raise ValueError("rpn_targets: anchors must be finite with positive area")


def _check_image(i: int, boxes: np.ndarray, ids: np.ndarray) -> None:
    if boxes.ndim != 2 or boxes.shape[1] != 4 or ids.shape != (boxes.shape[0],):
        raise ValueError(f"rpn_targets: image {i}: gt_boxes must be [G,4] and gt_class_ids [G], got {boxes.shape} and {ids.shape}")
    if boxes.shape[0] > MAX_ROWS_PER_IMAGE:
        raise ValueError(f"rpn_targets: image {i} has {boxes.shape[0]} rows; at most {MAX_ROWS_PER_IMAGE} per image")
    if not np.isfinite(boxes).all() or (boxes[:, 2] < boxes[:, 0]).any() or (boxes[:, 3] < boxes[:, 1]).any():
        raise ValueError(f"rpn_targets: image {i}: boxes must be finite with y2 >= y1 and x2 >= x1")
    kept = (ids > 0) if (ids < 0).any() else np.ones(ids.shape, bool)
    if not kept.any():
        raise ValueError(f"rpn_targets: image {i} has no usable ground truth (no row, or crowd and class-0 rows only)")


def _unpack(gt_boxes, gt_class_ids, gt_off):
    """Host copies per image: [(boxes float32 [G,4], ids int32 [G]), ...]."""
    if gt_off is None:
        if len(gt_boxes) != len(gt_class_ids) or len(gt_boxes) < 1:
            raise ValueError("rpn_targets: gt_boxes and gt_class_ids must be lists of the same length >= 1 (or packed, with gt_off)")
        return [(np.asarray(_host(b), np.float32).reshape(-1, 4), np.asarray(_host(c), np.int32).reshape(-1))
                for b, c in zip(gt_boxes, gt_class_ids)]
    off = np.asarray(_host(gt_off), np.int64).reshape(-1)
    boxes, ids = np.asarray(_host(gt_boxes), np.float32).reshape(-1, 4), np.asarray(_host(gt_class_ids), np.int32).reshape(-1)
    if off.size < 2 or off[0] != 0 or off[-1] != boxes.shape[0] or (np.diff(off) < 0).any() or ids.shape[0] != boxes.shape[0]:
        raise ValueError("rpn_targets: gt_off must be [B+1], ascending from 0 to the number of rows of gt_boxes / gt_class_ids")
    return [(boxes[s:e], ids[s:e]) for s, e in zip(off[:-1], off[1:])]


def rpn_targets(anchors, gt_boxes, gt_class_ids, count: int = 128, std_dev=(0.1, 0.1, 0.2, 0.2), keys=None, generator=None,
                device="cuda:0", gt_off=None):
    """data.rpn_samples for a batch → (rpn_match int32 [B,A,1], rpn_bbox float32 [B,count,4]), the shapes the reference's
    __getitem__ stacks into a batch (data.py:729-733).

    anchors: float64 [A,4] (anchors.pyramid_anchors(cfg, dtype=torch.float64)). gt_boxes / gt_class_ids: one array or tensor per
    image ([G,4] as (y1, x1, y2, x2), [G]; crowd rows have negative ids), or packed ([M,4], [M]) with gt_off [B+1]. keys: int32
    [B,A], non-negative — None draws them on the device from `generator`. An image without usable ground truth, a box with
    y2 < y1 and their like are a ValueError, checked on the host copies. Packed DEVICE tensors are not read back: they are the
    caller's responsibility (ops.anchor_match's status tells an image without a kept row).
    device="cpu": the same rule in numpy, returned as CPU tensors."""
    count = int(count)
    if count < 1:
        raise ValueError(f"rpn_targets: count={count} must be >= 1")
    dev = torch.device(device)
    on_device = gt_off is not None and _on_gpu(gt_boxes) and _on_gpu(gt_class_ids) and _on_gpu(gt_off)
    if not _on_gpu(anchors):
        _check_anchors(np.asarray(_host(anchors), np.float64))
    images = None
    if not on_device or dev.type == "cpu":
        images = _unpack(gt_boxes, gt_class_ids, gt_off)
        for i, (b, c) in enumerate(images):
            _check_image(i, b, c)
    batch = len(images) if images is not None else gt_off.numel() - 1
    n_anchors = anchors.shape[0]

    if dev.type == "cpu":
        a = np.asarray(_host(anchors), np.float64)
        if keys is None:
            keys = torch.randint(0, 2 ** 31 - 1, (batch, n_anchors), dtype=torch.int32, generator=generator)
        keys = np.asarray(_host(keys)).reshape(batch, n_anchors)
        rpn_match, rpn_bbox = np.zeros((batch, n_anchors, 1), np.int32), np.zeros((batch, count, 4), np.float32)
        for i, (b, c) in enumerate(images):
            match, arg, _, _, _ = match_numpy(a, b, c)
            match = sample_numpy(match, keys[i], count)
            rpn_match[i, :, 0] = match
            rpn_bbox[i] = deltas_numpy(a, b, match, arg, count, std_dev)[0]
        return torch.from_numpy(rpn_match), torch.from_numpy(rpn_bbox)

    from . import ops
    anchors_d = (anchors if isinstance(anchors, torch.Tensor) else torch.from_numpy(np.array(anchors, np.float64))).to(dev, torch.float64)
    if on_device:
        boxes_d, ids_d, off_d = gt_boxes.to(dev), gt_class_ids.to(dev), gt_off.to(dev)
    else:
        off = np.concatenate([[0], np.cumsum([len(c) for _, c in images])]).astype(np.int32)
        boxes_d = torch.from_numpy(np.concatenate([b for b, _ in images]).astype(np.float32)).to(dev)
        ids_d = torch.from_numpy(np.concatenate([c for _, c in images]).astype(np.int32)).to(dev)
        off_d = torch.from_numpy(off).to(dev)
    if keys is None:
        keys_d = torch.randint(0, 2 ** 31 - 1, (batch, n_anchors), dtype=torch.int32, device=dev, generator=generator)
    else:
        keys_d = (keys if isinstance(keys, torch.Tensor) else torch.from_numpy(np.array(keys, np.int32))).to(dev, torch.int32)
        keys_d = keys_d.reshape(batch, n_anchors)
    match, arg, _, _, _ = ops.anchor_match(anchors_d, boxes_d, ids_d, off_d, NEG_IOU, POS_IOU, CROWD_IOU)
    ops.sample_by_key(match, keys_d, count, out=match)
    rpn_bbox, _ = ops.rpn_deltas(anchors_d, boxes_d, off_d, match, arg, count, std_dev)
    return match.unsqueeze(-1), rpn_bbox
