"""Training targets for a batch of images, on the device.

RPN targets: the reference's data.rpn_samples (data.py:449-591, called per item at data.py:727) — anchor matching, subsampling,
regression deltas (csrc/targets.hip).

    rpn_match, rpn_bbox = rpn_targets(anchors.pyramid_anchors(cfg, dtype=torch.float64), gt_boxes, gt_class_ids)

Detection targets: the reference's model.mrn_samples (model.py:396-576, called from MaskRCNN.extract at model.py:1270, batch size
1 there) — RoI matching, subsampling, deltas, mask targets (csrc/detection_targets.hip; the rule is stated at
mrcnn_detection_targets in include/maskrcnn_hip.h).

    t = detection_targets(rois, gt_boxes, gt_class_ids, gt_masks)        # rois [B,N,4] from rpn_refine, normalised as the boxes
    rois_i, class_ids_i, deltas_i, masks_i = t.unpad(i)                   # image i in the reference's shapes (synchronises)

The rule is stated at mrcnn_anchor_match in include/maskrcnn_hip.h. One thing differs from the reference by design: where it
draws the anchors to reset with np.random.choice, here every anchor has a key and the ones with the smallest (key, anchor index)
stay; independent uniform keys (the default: drawn on the device) give the same distribution, given keys a reproducible result.

device="cpu" runs the same rule in numpy, without the library's kernels (match_numpy / sample_numpy / deltas_numpy below): the
fixtures' generator and a user without a GPU read it, and it is what the device results are compared with.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

__all__ = ["rpn_targets", "match_numpy", "sample_numpy", "deltas_numpy", "MAX_ROWS_PER_IMAGE",
           "detection_targets", "DetectionTargets", "roi_match_numpy", "roi_sample_numpy", "roi_deltas_numpy", "mask_targets_numpy",
           "MAX_ROIS_PER_IMAGE", "MAX_TARGET_COUNT"]

MAX_ROWS_PER_IMAGE = 1024      # an image's boxes are staged in LDS (the reference caps at MAX_GT_INSTANCES = 50)
NEG_IOU, POS_IOU, CROWD_IOU = 0.3, 0.7, 0.001
MAX_ROIS_PER_IMAGE = 4096      # detection targets: an image's RoIs are sorted in LDS (the reference proposes 2000)
MAX_TARGET_COUNT = 1024
ROI_POS_IOU = 0.5


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


def _crowd_and_kept(ids: np.ndarray):
    """The crowd rule, quirk included (data.py:496-502, model.py:435-442) → (crowd rows, kept rows): with a crowd row (id < 0) in
    the image the rows with id > 0 are kept and id 0 is dropped; without one every row is kept."""
    crowd = np.where(ids < 0)[0]
    return crowd, np.where(ids > 0)[0] if crowd.size else np.arange(ids.size)


def match_numpy(anchors, gt_boxes, gt_class_ids, neg_iou=NEG_IOU, pos_iou=POS_IOU, crowd_iou=CROWD_IOU):
    """Steps 1-6 for one image → (match int32 [A], iou_argmax int32 [A], iou_max float32 [A], gt_argmax int32 [G], status int).
    Row indices count all of the image's rows; status bit 0: no kept row (match 0, iou_argmax -1, iou_max 0)."""
    a32 = np.asarray(anchors, np.float64).astype(np.float32)
    boxes = np.asarray(gt_boxes, np.float32).reshape(-1, 4)
    ids = np.asarray(gt_class_ids, np.int32).reshape(-1)
    n = a32.shape[0]
    crowd, kept = _crowd_and_kept(ids)
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


def _check_image(i: int, boxes: np.ndarray, ids: np.ndarray, who: str = "rpn_targets") -> None:
    if boxes.ndim != 2 or boxes.shape[1] != 4 or ids.shape != (boxes.shape[0],):
        raise ValueError(f"{who}: image {i}: gt_boxes must be [G,4] and gt_class_ids [G], got {boxes.shape} and {ids.shape}")
    if boxes.shape[0] > MAX_ROWS_PER_IMAGE:
        raise ValueError(f"{who}: image {i} has {boxes.shape[0]} rows; at most {MAX_ROWS_PER_IMAGE} per image")
    if not np.isfinite(boxes).all() or (boxes[:, 2] < boxes[:, 0]).any() or (boxes[:, 3] < boxes[:, 1]).any():
        raise ValueError(f"{who}: image {i}: boxes must be finite with y2 >= y1 and x2 >= x1")
    if _crowd_and_kept(ids)[1].size == 0:
        raise ValueError(f"{who}: image {i} has no usable ground truth (no row, or crowd and class-0 rows only)")


def _unpack(gt_boxes, gt_class_ids, gt_off, who: str = "rpn_targets"):
    """Host copies per image: [(boxes float32 [G,4], ids int32 [G]), ...]."""
    if gt_off is None:
        if len(gt_boxes) != len(gt_class_ids) or len(gt_boxes) < 1:
            raise ValueError(f"{who}: gt_boxes and gt_class_ids must be lists of the same length >= 1 (or packed, with gt_off)")
        return [(np.asarray(_host(b), np.float32).reshape(-1, 4), np.asarray(_host(c), np.int32).reshape(-1))
                for b, c in zip(gt_boxes, gt_class_ids)]
    off = np.asarray(_host(gt_off), np.int64).reshape(-1)
    boxes, ids = np.asarray(_host(gt_boxes), np.float32).reshape(-1, 4), np.asarray(_host(gt_class_ids), np.int32).reshape(-1)
    if off.size < 2 or off[0] != 0 or off[-1] != boxes.shape[0] or (np.diff(off) < 0).any() or ids.shape[0] != boxes.shape[0]:
        raise ValueError(f"{who}: gt_off must be [B+1], ascending from 0 to the number of rows of gt_boxes / gt_class_ids")
    return [(boxes[s:e], ids[s:e]) for s, e in zip(off[:-1], off[1:])]


def _ground_truth(who: str, gt_boxes, gt_class_ids, gt_off, dev):
    """→ (images, boxes_d, ids_d, off_d, batch). images: the checked host copies per image — None for packed DEVICE tensors bound
    for the device, which are not read back. boxes_d float32 [M,4] / ids_d int32 [M] / off_d int32 [B+1]: the packed form on `dev`
    — None on the cpu route."""
    on_device = gt_off is not None and _on_gpu(gt_boxes) and _on_gpu(gt_class_ids) and _on_gpu(gt_off)
    if on_device and dev.type != "cpu":
        return None, gt_boxes.to(dev), gt_class_ids.to(dev), gt_off.to(dev), gt_off.numel() - 1
    images = _unpack(gt_boxes, gt_class_ids, gt_off, who)
    for i, (b, c) in enumerate(images):
        _check_image(i, b, c, who)
    if dev.type == "cpu":
        return images, None, None, None, len(images)
    off = np.concatenate([[0], np.cumsum([len(c) for _, c in images])]).astype(np.int32)
    boxes_d = torch.from_numpy(np.concatenate([b for b, _ in images]).astype(np.float32)).to(dev)
    ids_d = torch.from_numpy(np.concatenate([c for _, c in images]).astype(np.int32)).to(dev)
    return images, boxes_d, ids_d, torch.from_numpy(off).to(dev), len(images)


def _keys(keys, batch: int, n: int, dev, generator) -> torch.Tensor:
    """int32 [batch,n] on `dev`: the caller's keys, or uniform ones drawn there from `generator`."""
    if keys is None:
        return torch.randint(0, 2 ** 31 - 1, (batch, n), dtype=torch.int32, device=dev, generator=generator)
    if not isinstance(keys, torch.Tensor):
        keys = torch.from_numpy(np.array(keys, np.int32))
    return keys.to(dev, torch.int32).reshape(batch, n)


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
    if not _on_gpu(anchors):
        _check_anchors(np.asarray(_host(anchors), np.float64))
    images, boxes_d, ids_d, off_d, batch = _ground_truth("rpn_targets", gt_boxes, gt_class_ids, gt_off, dev)
    n_anchors = anchors.shape[0]
    keys = _keys(keys, batch, n_anchors, dev, generator)

    if dev.type == "cpu":
        a = np.asarray(_host(anchors), np.float64)
        keys = keys.numpy()
        rpn_match, rpn_bbox = np.zeros((batch, n_anchors, 1), np.int32), np.zeros((batch, count, 4), np.float32)
        for i, (b, c) in enumerate(images):
            match, arg, _, _, _ = match_numpy(a, b, c)
            match = sample_numpy(match, keys[i], count)
            rpn_match[i, :, 0] = match
            rpn_bbox[i] = deltas_numpy(a, b, match, arg, count, std_dev)[0]
        return torch.from_numpy(rpn_match), torch.from_numpy(rpn_bbox)

    from . import ops
    anchors_d = (anchors if isinstance(anchors, torch.Tensor) else torch.from_numpy(np.array(anchors, np.float64))).to(dev, torch.float64)
    match, arg, _, _, _ = ops.anchor_match(anchors_d, boxes_d, ids_d, off_d, NEG_IOU, POS_IOU, CROWD_IOU)
    ops.sample_by_key(match, keys, count, out=match)
    rpn_bbox, _ = ops.rpn_deltas(anchors_d, boxes_d, off_d, match, arg, count, std_dev)
    return match.unsqueeze(-1), rpn_bbox


# ----------------------------------------------------------------------------------------------------------------------
# Detection targets: the rule in numpy, one image at a time
# ----------------------------------------------------------------------------------------------------------------------
def roi_match_numpy(rois, gt_boxes, gt_class_ids, pos_iou=ROI_POS_IOU, crowd_iou=CROWD_IOU):
    """Steps 1-3 for one image → (cls int32 [N]: 0 positive, 1 negative, 2 neither; gt_index int32 [N] within all of the image's
    rows; iou_max float32 [N]; status int). status bit 0: no kept row (cls 2, gt_index -1, iou_max 0)."""
    r32 = np.asarray(rois, np.float32).reshape(-1, 4)
    boxes = np.asarray(gt_boxes, np.float32).reshape(-1, 4)
    ids = np.asarray(gt_class_ids, np.int32).reshape(-1)
    n = r32.shape[0]
    crowd, kept = _crowd_and_kept(ids)
    cls = np.full(n, 2, np.int32)
    if kept.size == 0:
        return cls, np.full(n, -1, np.int32), np.zeros(n, np.float32), 1
    crowd_max = np.zeros(n, np.float32)
    if crowd.size:
        crowd_max = np.fmax.reduce(_overlaps(r32, boxes[crowd]), axis=1, initial=np.float32(0))
    ov = _overlaps(r32, boxes[kept])
    ov = np.where(np.isnan(ov), np.float32(-2), ov)      # a NaN (a pair whose union is 0) never wins the maximum
    arg = np.argmax(ov, axis=1)                          # the first, as torch.max(dim=1) on the CPU
    best = ov[np.arange(n), arg]
    valid = best > np.float32(-1)
    cls[valid & (best >= np.float32(pos_iou))] = 0
    cls[valid & (best < np.float32(pos_iou)) & (crowd_max < np.float32(crowd_iou))] = 1
    return cls, np.where(valid, kept[arg], -1).astype(np.int32), np.where(valid, best, np.float32(0)), 0


def roi_sample_numpy(cls, keys, count: int, positive_ratio: float = 0.33):
    """Steps 4-5 for one image → (roi_index int32 [count]: the kept positives, then the kept negatives, each by ascending
    (key, roi index), padded with -1; num_pos; num_neg)."""
    cls = np.asarray(cls)
    keys = np.asarray(keys).astype(np.int64) & 0x7fffffff
    pos_limit = int(count * positive_ratio)
    order = lambda ids: ids[np.lexsort((ids, keys[ids]))]
    pos = order(np.where(cls == 0)[0])[:pos_limit]
    neg = np.zeros(0, np.int64)
    if len(pos):
        r = 1.0 / positive_ratio
        neg_limit = int(r * len(pos) - len(pos))
        neg = order(np.where(cls == 1)[0])[:max(min(neg_limit, count - len(pos)), 0)]
    out = np.full(count, -1, np.int32)
    out[:len(pos)] = pos
    out[len(pos):len(pos) + len(neg)] = neg
    return out, len(pos), len(neg)


def roi_deltas_numpy(rois, gt_boxes, std_dev=(0.1, 0.1, 0.2, 0.2)) -> np.ndarray:
    """Step 6's deltas: boxes_deltas (data.py:103-121) of rois [n,4] against THEIR rows gt_boxes [n,4], float32 operation by
    operation (the logarithm in float64, narrowed), each divided by its float32 std_dev → float32 [n,4]."""
    b = np.asarray(rois, np.float32).reshape(-1, 4)
    g = np.asarray(gt_boxes, np.float32).reshape(-1, 4)
    std = np.asarray(std_dev, np.float32)
    half = np.float32(0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        h, w = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        cy, cx = b[:, 0] + half * h, b[:, 1] + half * w
        gh, gw = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
        gcy, gcx = g[:, 0] + half * gh, g[:, 1] + half * gw
        dy, dx = (gcy - cy) / h, (gcx - cx) / w
        dh, dw = np.log((gh / h).astype(np.float64)).astype(np.float32), np.log((gw / w).astype(np.float64)).astype(np.float32)
        out = np.stack([dy / std[0], dx / std[1], dh / std[2], dw / std[3]], axis=1)
    assert out.dtype == np.float32
    return out


def _crop_samples(c1: np.float32, c2: np.float32, size: int, crop: int):
    """crop_cpu.cpp:52-61 / :82-84, as csrc/crop_math.hpp's make_sample: (lo, hi, lerp, inside) of the crop's rows or columns."""
    last = np.float32(size - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        if crop > 1:
            s = (c2 - c1) * last
            scale = s / np.float32(crop - 1)
            pos = c1 * last + np.arange(crop, dtype=np.float32) * scale
        else:
            pos = np.array([np.float32(0.5 * np.float64(c1 + c2) * np.float64(size - 1))], np.float32)
        inside = ~((pos < 0) | (pos > last))
        safe = np.where(inside & np.isfinite(pos), pos, np.float32(0))
        lo, hi = np.floor(safe).astype(np.int64), np.ceil(safe).astype(np.int64)
        lerp = pos - lo.astype(np.float32)
    return np.clip(lo, 0, size - 1), np.clip(hi, 0, size - 1), lerp.astype(np.float32), inside


def mask_targets_numpy(gt_masks, gt_index, rois, mask_shape=(28, 28)) -> np.ndarray:
    """Step 7: for every i, CropFunction(mh, mw, 0) of gt_masks[gt_index[i]] ([M,H,W]; any dtype, read as float32 at the taps) with
    box rois[i], float32 operation by operation, then np.round (ties to even) → float32 [n,mh,mw]. gt_index < 0: zeros."""
    masks = np.asarray(gt_masks)
    boxes = np.asarray(rois, np.float32).reshape(-1, 4)
    mh, mw = int(mask_shape[0]), int(mask_shape[1])
    hh, ww = masks.shape[1], masks.shape[2]
    out = np.zeros((boxes.shape[0], mh, mw), np.float32)
    for i, g in enumerate(np.asarray(gt_index).reshape(-1)):
        if g < 0:
            continue
        y_lo, y_hi, y_l, y_in = _crop_samples(boxes[i, 0], boxes[i, 2], hh, mh)
        x_lo, x_hi, x_l, x_in = _crop_samples(boxes[i, 1], boxes[i, 3], ww, mw)
        img = masks[g]
        tap = lambda ys, xs: img[ys[:, None], xs[None, :]].astype(np.float32)
        tl, tr, bl, br = tap(y_lo, x_lo), tap(y_lo, x_hi), tap(y_hi, x_lo), tap(y_hi, x_hi)
        xl, yl = x_l[None, :], y_l[:, None]
        with np.errstate(invalid="ignore"):
            top = tl + (tr - tl) * xl
            bot = bl + (br - bl) * xl
            v = top + (bot - top) * yl
        assert v.dtype == np.float32
        out[i] = np.round(np.where(y_in[:, None] & x_in[None, :], v, np.float32(0)))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# Detection targets: front end
# ----------------------------------------------------------------------------------------------------------------------
class DetectionTargets(NamedTuple):
    """What detection_targets returns: the padded tensors of the batch, `count` slots per image — the positives first, then the
    negatives, then zeros (indices -1). gt_index is -1 for a negative; status bit 0: the image has no usable ground truth."""
    rois: torch.Tensor                 # float32 [B,count,4]
    target_class_ids: torch.Tensor     # int32 [B,count]
    target_deltas: torch.Tensor        # float32 [B,count,4]
    target_mask: torch.Tensor          # float32 [B,count,mh,mw]
    roi_index: torch.Tensor            # int32 [B,count]
    gt_index: torch.Tensor             # int32 [B,count]
    num_pos: torch.Tensor              # int32 [B]
    num_neg: torch.Tensor              # int32 [B]
    status: torch.Tensor               # int32 [B]

    def unpad(self, i: int):
        """Image i as the reference's mrn_samples returns it: (rois float32 [n,4], roi_gt_class_ids int32 [n], deltas float32
        [n,4], masks float32 [n,mh,mw]) with n = num_pos + num_neg; four empty tensors when n is 0 (model.py:566-569). The one
        call that synchronises with the host."""
        n = int(self.num_pos[i]) + int(self.num_neg[i])
        if n == 0:
            dev = self.rois.device
            return (torch.empty(0, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                    torch.empty(0, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.float32, device=dev))
        return self.rois[i, :n], self.target_class_ids[i, :n], self.target_deltas[i, :n], self.target_mask[i, :n]


def _check_rois(who: str, i: int, r: np.ndarray) -> None:
    if not np.isfinite(r).all() or (r[:, 2] < r[:, 0]).any() or (r[:, 3] < r[:, 1]).any():
        raise ValueError(f"{who}: image {i}: rois must be finite with y2 >= y1 and x2 >= x1")


def detection_targets(rois, gt_boxes, gt_class_ids, gt_masks, count: int = 100, positive_ratio: float = 0.33,
                      std_dev=(0.1, 0.1, 0.2, 0.2), mask_shape=(28, 28), pos_iou: float = ROI_POS_IOU, keys=None, generator=None,
                      device="cuda:0", gt_off=None) -> DetectionTargets:
    """model.mrn_samples for a batch → DetectionTargets (padded to `count` slots per image; .unpad(i) gives image i in the
    reference's shapes).

    rois: float32 [B,N,4] as (y1, x1, y2, x2) (or one [N,4] per image, the same N), in the coordinates of gt_boxes (the reference
    normalises both); zero rows are ordinary RoIs. gt_boxes / gt_class_ids / gt_masks: one array or tensor per image ([G,4], [G],
    [G,H,W] uint8 / bool / float32; crowd rows have negative ids), or packed ([M,4], [M], [M,H,W]) with gt_off [B+1]; one H x W for
    the call. keys: int32 [B,N], non-negative — None draws them on the device from `generator`; they stand in for the reference's
    torch.randperm: the RoIs with the smallest (key, roi index) are kept, in that order. An image without usable ground truth, a
    box with y2 < y1, more than 1024 rows or 4096 RoIs per image, masks that do not match the boxes are a ValueError, checked on
    the host copies. Packed DEVICE tensors are not read back: they are the caller's responsibility (status tells an image without
    a kept row, whose slots are all empty). Nothing here synchronises with the host when the inputs are on the device.
    device="cpu": the same rule in numpy, returned as CPU tensors."""
    who = "detection_targets"
    count, mh, mw = int(count), int(mask_shape[0]), int(mask_shape[1])
    if not 1 <= count <= MAX_TARGET_COUNT:
        raise ValueError(f"{who}: count={count} must be in [1, {MAX_TARGET_COUNT}]")
    if not 0.0 < float(positive_ratio) <= 1.0:
        raise ValueError(f"{who}: positive_ratio={positive_ratio} must be in (0, 1]")
    if not (1 <= mh <= 64 and 1 <= mw <= 64):
        raise ValueError(f"{who}: mask_shape={tuple(mask_shape)}: both sides must be in [1, 64]")
    positive_ratio = float(positive_ratio)
    dev = torch.device(device)
    if isinstance(rois, (list, tuple)):
        if len({tuple(r.shape) for r in rois}) != 1:
            raise ValueError(f"{who}: every image needs the same number of rois [N,4], got {[tuple(r.shape) for r in rois]}")
        rois = torch.stack(list(rois)) if isinstance(rois[0], torch.Tensor) else np.stack([np.asarray(r) for r in rois])
    if len(rois.shape) != 3 or rois.shape[2] != 4 or rois.shape[0] < 1 or rois.shape[1] < 1:
        raise ValueError(f"{who}: rois must be [B,N,4] with B, N >= 1, got {tuple(rois.shape)}")
    batch, n = int(rois.shape[0]), int(rois.shape[1])
    if n > MAX_ROIS_PER_IMAGE:
        raise ValueError(f"{who}: N={n} rois per image; at most {MAX_ROIS_PER_IMAGE}")
    images, boxes_d, ids_d, off_d, gt_batch = _ground_truth(who, gt_boxes, gt_class_ids, gt_off, dev)
    if gt_batch != batch:
        raise ValueError(f"{who}: rois of {batch} images, {'gt_off' if images is None else 'ground truth'} of {gt_batch}")
    # masks: [M,H,W] in one piece, rows as the boxes'
    if gt_off is not None:
        masks = gt_masks
        rows = int(gt_boxes.shape[0])
        if len(masks.shape) != 3 or int(masks.shape[0]) != rows:
            raise ValueError(f"{who}: gt_masks must be [M,H,W] with one row per row of gt_boxes ({rows}), got {tuple(masks.shape)}")
    else:
        if len(gt_masks) != batch:
            raise ValueError(f"{who}: gt_masks of {len(gt_masks)} images, rois of {batch}")
        for i, (mk, (b, _)) in enumerate(zip(gt_masks, images)):
            if len(mk.shape) != 3 or int(mk.shape[0]) != b.shape[0]:
                raise ValueError(f"{who}: image {i}: gt_masks must be [G,H,W] with one mask per box ({b.shape[0]}), got {tuple(mk.shape)}")
        if len({(tuple(mk.shape[1:]), str(mk.dtype).replace("torch.", "")) for mk in gt_masks}) != 1:
            raise ValueError(f"{who}: the masks of every image must have one H x W and one dtype")
        masks = torch.cat(list(gt_masks)) if isinstance(gt_masks[0], torch.Tensor) else np.concatenate([np.asarray(mk) for mk in gt_masks])
    if str(masks.dtype).replace("torch.", "") not in ("uint8", "bool", "float32"):
        raise ValueError(f"{who}: gt_masks must be uint8, bool or float32, got {masks.dtype}")
    if not (1 <= int(masks.shape[1]) <= 16384 and 1 <= int(masks.shape[2]) <= 16384):
        raise ValueError(f"{who}: masks of {int(masks.shape[1])} x {int(masks.shape[2])}; height and width must be in [1, 16384]")
    if not _on_gpu(rois):
        r_host = np.asarray(_host(rois), np.float32)
        for i in range(batch):
            _check_rois(who, i, r_host[i])

    keys = _keys(keys, batch, n, dev, generator)
    if dev.type == "cpu":
        r_host, m_host = np.asarray(_host(rois), np.float32), _host(masks)
        keys = keys.numpy()
        out = DetectionTargets(np.zeros((batch, count, 4), np.float32), np.zeros((batch, count), np.int32),
                               np.zeros((batch, count, 4), np.float32), np.zeros((batch, count, mh, mw), np.float32),
                               np.full((batch, count), -1, np.int32), np.full((batch, count), -1, np.int32),
                               np.zeros(batch, np.int32), np.zeros(batch, np.int32), np.zeros(batch, np.int32))
        start = 0
        for i, (b, c) in enumerate(images):
            cls, arg, _, out.status[i] = roi_match_numpy(r_host[i], b, c, pos_iou, CROWD_IOU)
            idx, p, q = roi_sample_numpy(cls, keys[i], count, positive_ratio)
            out.num_pos[i], out.num_neg[i] = p, q
            out.roi_index[i] = idx
            out.rois[i, :p + q] = r_host[i][idx[:p + q]]
            out.gt_index[i, :p] = arg[idx[:p]]
            out.target_class_ids[i, :p] = c[arg[idx[:p]]]
            out.target_deltas[i, :p] = roi_deltas_numpy(r_host[i][idx[:p]], b[arg[idx[:p]]], std_dev)
            out.target_mask[i, :p] = mask_targets_numpy(m_host[start:start + len(c)], arg[idx[:p]], r_host[i][idx[:p]], (mh, mw))
            start += len(c)
        return DetectionTargets(*[torch.from_numpy(v) for v in out])

    from . import ops
    def as_dev(x, dtype=None):
        if not isinstance(x, torch.Tensor):
            x = np.ascontiguousarray(x)
            x = torch.from_numpy(x if x.flags.writeable else x.copy())
        return x.to(dev, dtype)

    rois_d, masks_d = as_dev(rois, torch.float32), as_dev(masks)
    rois_out, class_ids, deltas, roi_index, gt_index, num_pos, num_neg, status = ops.detection_targets(
        rois_d, boxes_d, ids_d, off_d, keys, count, positive_ratio, std_dev, pos_iou, CROWD_IOU)
    target_mask = ops.mask_targets(masks_d, off_d, rois_out, gt_index, num_pos, (mh, mw))
    return DetectionTargets(rois_out, class_ids, deltas, target_mask, roi_index, gt_index, num_pos, num_neg, status)
