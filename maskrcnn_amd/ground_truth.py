"""Ground truth for training, made on the GPU from a COCO data set: what the reference's dataset class does per image on the host
— CocoMaskRCNNDataset.load (data.py:797-876) and encode_image / encode_masks / encode_boxes (:191-223, :246-262, :317-328) —
for a batch of images at once, bit for bit (tests/golden/ground_truth.npz).

    gt = load_batch("instances_train.json", image_ids, cfg.image_min_dim, cfg.image_max_dim, hflip=generator)
    rpn_match, rpn_bbox = targets.rpn_targets(anchors, gt.gt_boxes, gt.gt_class_ids, gt_off=gt.gt_off)
    t = targets.detection_targets(rois, gt.gt_boxes, gt.gt_class_ids, gt.gt_masks, gt_off=gt.gt_off)

The rule, for image i with flip flag f (h x w: the image's size):
  1. annotations in data set order; label = labels[category_id]; label 0 is skipped; an unknown category id is a ValueError
     (the reference: KeyError);
  2. the mask is annToMask of the annotation; a mask without an on pixel is skipped; a crowd annotation whose RLE size differs
     from the image's becomes an all-ones mask of the image's size;
  3. with f the mask is mirrored left to right;
  4. the box is (y1, x1, y2+1, x2+1) of the on pixels, float32;
  5. no annotation kept: ONE row — label 0, box (0, 0, h, w), an all-ones mask;
  6. scale and window are encode_image's: image.resize_plan(h, w, min_dim, max_dim, True), except that for scale == 1 the
     reference neither resizes nor pads and its window is (0, 0, h, w);
  7. scale != 1: each 0 / 1 mask is resized with Pillow's BILINEAR to (round(h*scale), round(w*scale)) and zero-padded by
     (left, top, left, top); the boxes are fp32(box * fp32(scale)), then + top / + left in fp32, operation by operation.
Decisions where the reference's output cannot be used as it is:
  * canvas: the reference pads symmetrically, so its mask is new_h + 2*top by new_w + 2*left — one row or column short of
    max_dim when the pad is odd. Here every mask is max_dim x max_dim (detection_targets takes one H x W per call): the bytes
    on the reference's extent are the reference's, the extra last row or column is zero, as it is in the reference's image.
  * scale == 1: the mask is copied unresampled to the canvas's top-left corner and the boxes are not shifted: the reference's
    window (0, 0, h, w). (A source side above max_dim cannot occur with scale == 1.)
  * crowd ids: load() writes class_id *= -1 and then appends the unchanged label_id, so the reference's crowd rows are in fact
    positive, while rpn_samples, mrn_samples and this package's target ops expect negative ids. crowds="negative" (the default)
    gives -label for iscrowd rows, crowds="reference" what load() returns.
  * the image itself is not molded here: callers use ops.mold_images_u8 at the returned window and mirror the image themselves
    when the flip flag is set. (normalize_image's float32(px/255)*255 - mean may differ from that kernel's
    float(double(px) - mean) in the last bit.)
  * the MAX_GT_INSTANCES slice of data.py:870-874 is a no-op ([:m]) and stays one.
"""
from __future__ import annotations

import json
from typing import NamedTuple

import numpy as np
import torch

from . import image as imagelib

__all__ = ["GroundTruth", "load_batch", "default_labels", "MAX_ROWS_PER_IMAGE"]

MAX_ROWS_PER_IMAGE = 1024      # what ops.anchor_match / ops.detection_targets take per image


class GroundTruth(NamedTuple):
    """What load_batch returns. The first four go straight into targets.rpn_targets(..., gt_off=) and
    targets.detection_targets(..., gt_off=)."""
    gt_boxes: torch.Tensor        # float32 [M,4] (y1, x1, y2, x2) in canvas pixels
    gt_class_ids: torch.Tensor    # int32 [M]
    gt_masks: torch.Tensor        # uint8 [M,max_dim,max_dim], 0 / 1
    gt_off: torch.Tensor          # int32 [B+1]: image i owns rows [gt_off[i], gt_off[i+1])
    windows: torch.Tensor         # int64 [B,4] (y1, x1, y2, x2)
    scales: list                  # B Python numbers, encode_image's
    flips: list                   # B bools


def default_labels(gt) -> dict:
    """category id → contiguous label 1, 2, ... over gt["categories"] sorted by id (for COCO's 80 categories: the reference's
    CocoLabel.from_class), and 0 → 0."""
    ids = sorted(int(c["id"]) for c in gt["categories"] if int(c["id"]) != 0)
    return {0: 0, **{c: i + 1 for i, c in enumerate(ids)}}


def _flips(hflip, n: int) -> list:
    if hflip is None:
        return [False] * n
    if isinstance(hflip, (int, np.integer)) and not isinstance(hflip, bool):
        hflip = torch.Generator().manual_seed(int(hflip))
    if isinstance(hflip, torch.Generator):
        return [bool(v) for v in torch.randint(0, 2, (n,), generator=hflip).tolist()]
    hflip = list(hflip)
    if len(hflip) != n:
        raise ValueError(f"load_batch: hflip has {len(hflip)} entries for {n} images")
    return [bool(v) for v in hflip]


class _Image(NamedTuple):
    h: int
    w: int
    new_h: int
    new_w: int
    top: int
    left: int
    scale: float
    window: tuple


def _plan(h: int, w: int, min_dim: int, max_dim: int) -> _Image:
    new_h, new_w, window, scale, _ = imagelib.resize_plan(h, w, min_dim, max_dim, True)
    if scale == 1:        # data.py:207: neither resized nor padded
        return _Image(h, w, h, w, 0, 0, scale, (0, 0, h, w))
    return _Image(h, w, new_h, new_w, window[0], window[1], scale, tuple(window))


def _candidates(gt, image_ids, labels, plans_of):
    """Rule 1 on the host → (rows, sizes): rows [(image index, annotation, label, crowd, kind, segmentation, (h, w) of the RLE,
    replaced)], kind "poly" / "string" / "counts"; replaced: a crowd whose RLE size differs from the image's."""
    images = {img["id"]: img for img in gt["images"]}
    by_image = {}
    for ann in gt["annotations"]:
        by_image.setdefault(ann["image_id"], []).append(ann)
    rows, plans = [], []
    for i, image_id in enumerate(image_ids):
        if image_id not in images:
            raise ValueError(f"load_batch: image id {image_id!r} is not in the data set")
        h, w = int(images[image_id]["height"]), int(images[image_id]["width"])
        plans.append(plans_of(h, w))
        for ann in by_image.get(image_id, []):
            who = f"annotation {ann.get('id')}"
            if ann["category_id"] not in labels:
                raise ValueError(f"load_batch: {who} has category id {ann['category_id']!r}, which the label map does not know")
            label = int(labels[ann["category_id"]])
            if not label:
                continue
            seg = ann.get("segmentation")
            if seg is None or (isinstance(seg, (list, tuple, dict)) and len(seg) == 0):
                raise ValueError(f"load_batch: {who} has no segmentation")
            crowd = bool(ann.get("iscrowd", 0))
            if isinstance(seg, (list, tuple)):
                rows.append((i, ann, label, crowd, "poly", seg, (h, w), False))
                continue
            if not isinstance(seg, dict) or "counts" not in seg or "size" not in seg:
                raise ValueError(f"load_batch: {who}: a segmentation is a polygon list or an RLE dict with 'size' and 'counts'")
            size = (int(seg["size"][0]), int(seg["size"][1]))
            kind = "counts" if imagelib._string_of(seg) is None else "string"
            replaced = size != (h, w)
            if replaced and not crowd:
                raise ValueError(f"load_batch: {who} is an RLE of {list(size)} on an image of {[h, w]}")
            rows.append((i, ann, label, crowd, kind, seg, size, replaced))
    return rows, plans


def _finish(rows, plans, flips, areas, bboxes, crowds):
    """Rules 2-7 for the boxes, ids and offsets, on the host → (kept: [(row index or -1 - image index for an all-ones row, image
    index)], gt_boxes float32 [M,4], ids int32 [M], gt_off int32 [B+1])."""
    kept, boxes, ids, off = [], [], [], [0]
    by_image = [[] for _ in plans]
    for r, row in enumerate(rows):
        by_image[row[0]].append(r)
    for i, (p, flip) in enumerate(zip(plans, flips)):
        mine = [r for r in by_image[i] if areas[r] > 0]            # m.max() < 1: skipped
        for r in mine:
            _, _, label, crowd, _, _, _, replaced = rows[r]
            if replaced:                                            # data.py:832-833: all ones
                kept.append((-1 - i, i))
                x, y, bw, bh = 0, 0, p.w, p.h
            else:
                kept.append((r, i))
                x, y, bw, bh = (int(v) for v in bboxes[r])
            x1, x2 = (p.w - (x + bw), p.w - x) if flip else (x, x + bw)
            boxes.append([y, x1, y + bh, x2])
            ids.append(-label if crowd and crowds == "negative" else label)
        if not mine:                                                # data.py:859-867: the fake row
            kept.append((-1 - i, i))
            boxes.append([0, 0, p.h, p.w])
            ids.append(0)
        if len(kept) - off[-1] > MAX_ROWS_PER_IMAGE:
            raise ValueError(f"load_batch: image {i} of the batch has {len(kept) - off[-1]} ground-truth rows; the target ops take "
                             f"{MAX_ROWS_PER_IMAGE}")
        off.append(len(kept))
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    for i, p in enumerate(plans):                                   # encode_boxes, operation by operation in fp32
        if p.scale != 1:
            s = b[off[i]:off[i + 1]]
            s *= np.float32(p.scale)
            s += np.array([p.top, p.left, p.top, p.left], dtype=np.float32)
    return kept, b, np.asarray(ids, dtype=np.int32), np.asarray(off, dtype=np.int32)


# ------------------------------------------------------------------------------------------------ the host route
def _poly_keys(xy, h: int, w: int) -> np.ndarray:
    """Steps 1-3 of rleFrPoly (cocoapi/common/maskApi.c:162-191): the kept column crossings' keys x*h + y."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    X, Y = np.trunc(5.0 * xy[:, 0] + .5).astype(np.int64), np.trunc(5.0 * xy[:, 1] + .5).astype(np.int64)
    k, us, vs = len(X), [], []
    minor = lambda a0, s, t: np.trunc(float(a0) + s * t.astype(np.float64) + .5).astype(np.int64)
    for j in range(k):
        xs, xe, ys, ye = int(X[j]), int(X[(j + 1) % k]), int(Y[j]), int(Y[(j + 1) % k])
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        d = np.arange(max(dx, dy) + 1, dtype=np.int64)
        if dx >= dy:
            t = dx - d if flip else d
            us.append(t + xs)
            vs.append(np.full(1, -2 ** 31, np.int64) if dx == 0 else minor(ys, float(ye - ys) / float(dx), t))   # (int)NaN
        else:
            t = dy - d if flip else d
            vs.append(t + ys)
            us.append(minor(xs, float(xe - xs) / float(dy), t))
    u, v = np.concatenate(us), np.concatenate(vs)
    j = np.nonzero(u[1:] != u[:-1])[0] + 1
    xd = (np.where(u[j] < u[j - 1], u[j], u[j] - 1).astype(np.float64) + .5) / 5.0 - .5
    keep = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    yd = np.ceil(np.clip((np.minimum(v[j], v[j - 1]).astype(np.float64) + .5) / 5.0 - .5, 0, h))
    return xd[keep].astype(np.int64) * h + yd[keep].astype(np.int64)


def _poly_mask(parts, h: int, w: int) -> np.ndarray:
    """annToMask of a polygon annotation on the host: rleFrPoly per part by the parity rule (a pixel boundary falls at every key
    below h*w that occurs an odd number of times), the union of the parts (rleMerge), decoded column-major."""
    on = np.zeros(h * w, dtype=bool)
    for part in parts:
        keys = _poly_keys(part[:2 * (len(part) // 2)], h, w)
        vals, cnt = np.unique(keys[keys < h * w], return_counts=True)
        toggles = np.zeros(h * w + 1, dtype=np.int64)
        toggles[vals[cnt % 2 == 1]] = 1
        on |= (np.cumsum(toggles[:-1]) & 1).astype(bool)
    return on.reshape(w, h).T


def _load_host(rows, plans, flips, max_dim, crowds):
    from PIL import Image
    from .cocoeval import _polygon_parts
    dense, areas, bboxes = [], [], []
    for _, ann, _, _, kind, seg, (h, w), _ in rows:
        if kind == "poly":
            m = _poly_mask(_polygon_parts(ann), h, w)
        else:
            try:
                m = imagelib.rle_decode(imagelib._checked_counts(seg, "load_batch", 0, h, w), (h, w))
            except ValueError as e:
                raise ValueError(f"load_batch: annotation {ann.get('id')}: {e}") from e
        dense.append(m)
        ys, xs = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
        areas.append(int(m.sum()))
        bboxes.append([xs[0], ys[0], xs[-1] - xs[0] + 1, ys[-1] - ys[0] + 1] if xs.size else [0, 0, 0, 0])
    kept, boxes, ids, off = _finish(rows, plans, flips, areas, bboxes, crowds)
    masks = np.zeros((len(kept), max_dim, max_dim), dtype=np.uint8)
    for k, (r, i) in enumerate(kept):
        p = plans[i]
        m = np.ones((p.h, p.w), dtype=np.uint8) if r < 0 else dense[r].astype(np.uint8)
        if flips[i]:
            m = m[:, ::-1]
        if (p.new_h, p.new_w) != (p.h, p.w):
            m = np.array(Image.fromarray(np.ascontiguousarray(m)).resize((p.new_w, p.new_h), Image.BILINEAR))
        masks[k, p.top:p.top + p.new_h, p.left:p.left + p.new_w] = m
    return torch.from_numpy(boxes), torch.from_numpy(ids), torch.from_numpy(masks), torch.from_numpy(off)


# ------------------------------------------------------------------------------------------------ the device route
def _load_device(rows, plans, flips, max_dim, crowds, device):
    from . import ops
    from .cocoeval import _polygon_table
    n, b = len(rows), len(plans)
    # one table: the candidates' rows, then one all-ones row [0, h*w] per image (the fake row; a replaced crowd)
    parts = []
    sizes = [row[6] for row in rows] + [(p.h, p.w) for p in plans]
    poly = [r for r, row in enumerate(rows) if row[4] == "poly"]
    if poly:
        nr, cnt = _polygon_table([rows[r][1] for r in poly], [rows[r][6] for r in poly], device)
        parts.append((np.asarray(poly, np.int64), nr, cnt))
    host_idx, host_rows = list(range(n, n + b)), [np.array([0, p.h * p.w], dtype=np.uint32) for p in plans]
    for r, row in enumerate(rows):
        if row[4] == "counts":
            try:
                host_rows.append(imagelib._checked_counts(row[5], "load_batch", 0, *row[6]))
            except ValueError as e:
                raise ValueError(f"load_batch: annotation {row[1].get('id')}: {e}") from e
            host_idx.append(r)
    parts.append((np.asarray(host_idx, np.int64), *imagelib._pack_table(host_rows, device)))
    strs = [r for r, row in enumerate(rows) if row[4] == "string"]
    status = torch.zeros(n + b, dtype=torch.int32, device=device)
    if strs:
        nr, cnt, st = imagelib._strings_to_device([imagelib._string_of(rows[r][5]) for r in strs], [rows[r][6][0] for r in strs],
                                                  [rows[r][6][1] for r in strs], device)
        at = torch.from_numpy(np.asarray(strs, np.int64)).to(device)
        status[at] = st
        parts.append((np.asarray(strs, np.int64), nr, cnt))
    num_runs, counts = imagelib._merge_tables(n + b, parts, device)
    hw = torch.tensor(sizes, dtype=torch.int32).to(device)
    hs, ws = hw[:, 0].contiguous(), hw[:, 1].contiguous()
    areas, bboxes = ops.rle_area_bbox(num_runs, counts, hs, ws)
    back = torch.cat([areas[:, None], bboxes, status[:, None], num_runs[:, None]], dim=1).cpu().numpy()      # THE copy back
    for r in strs:
        if back[r, 5] or back[r, 6] < 0:
            d = imagelib._Decoded(num_runs, counts, back[:, 6], back[:, 5])
            h, w = rows[r][6]
            err = imagelib._status_error(d, r, f"load_batch: annotation {rows[r][1].get('id')}: the segmentation",
                                         (f"load_batch: annotation {rows[r][1].get('id')}", 0, h, w))
            if err is not None:
                raise err
    kept, boxes, ids, off = _finish(rows, plans, flips, back[:, 0], back[:, 1:5], crowds)
    index = np.array([n + (-1 - r) if r < 0 else r for r, _ in kept], dtype=np.int64)
    geom = np.array([[plans[i].new_h, plans[i].new_w, plans[i].top, plans[i].left, int(flips[i])] for _, i in kept], dtype=np.int64)
    ints = torch.from_numpy(np.concatenate([index[:, None], geom], axis=1)).to(device)                       # one copy up
    at = ints[:, 0]
    # no row is refused: _check_sizes has applied the op's own limits to every image, and every row of the table is usable
    masks, _ = ops.rle_resample(num_runs[at], counts[at], hs[at], ws[at], ints[:, 1:].to(torch.int32), max_dim, max_dim)
    return torch.from_numpy(boxes).to(device), torch.from_numpy(ids).to(device), masks, torch.from_numpy(off).to(device)


def _check_sizes(plans, image_ids, max_dim: int) -> None:
    """What ops.rle_resample would refuse with a status bit, found on the host before anything is launched: reading the status
    back would be a second synchronisation."""
    for p, image_id in zip(plans, image_ids):
        who = f"load_batch: image {image_id!r} ({p.h} x {p.w})"
        if not (1 <= p.h <= 16384 and 1 <= p.w <= 16384 and 1 <= p.new_h <= 16384 and 1 <= p.new_w <= 16384):
            raise ValueError(f"{who}: sizes must be in [1, 16384] before and after the resize ({p.new_h} x {p.new_w})")
        if p.top < 0 or p.left < 0 or p.top + p.new_h > max_dim or p.left + p.new_w > max_dim:
            raise ValueError(f"{who}: the resized image ({p.new_h} x {p.new_w}) does not fit the {max_dim} x {max_dim} canvas")
        if p.h > 16 * p.new_h or p.w > 16 * p.new_w:
            raise ValueError(f"{who}: shrinking to {p.new_h} x {p.new_w} is by more than 16, the limit of ops.rle_resample")


def load_batch(gt, image_ids, min_dim: int, max_dim: int, hflip=None, crowds: str = "negative", labels=None,
               device="cuda:0") -> GroundTruth:
    """The packed ground truth of a batch of images of a COCO data set (the module docstring has the rule and the decisions).

    gt: a COCO dict (images, annotations, categories) or its path. image_ids: the batch. hflip: None (no flips), one bool per
    image, or a torch.Generator / an int seed that draws one bool per image on the host (the reference's random.randint stream is
    not part of the rule). crowds: "negative" (-label for iscrowd rows, what the target ops expect) or "reference" (load()'s
    positive ids). labels: {category id: label}; None: default_labels(gt).
    → GroundTruth: gt_boxes float32 [M,4], gt_class_ids int32 [M], gt_masks uint8 [M,max_dim,max_dim], gt_off int32 [B+1], windows
    int64 [B,4] — all on `device` — and scales, flips (lists).

    On a GPU device: polygons go through ONE ops.rle_from_poly and ONE ops.rle_merge for the whole batch, compressed strings
    through ONE ops.rle_from_string, count lists are packed on the host, and all are merged into one table; ONE ops.rle_area_bbox
    call and ONE device-to-host copy of 28 bytes per annotation (area, bbox, the string decoder's status, the run count) decide
    which rows are kept and give the boxes (mirrored as x1' = w - x2 when flipped) and gt_off; ONE ops.rle_resample call makes
    all masks of the batch. That copy is the only synchronisation with the device.
    device="cpu": the same rule with numpy and Pillow, without the library.
    ValueError, naming the image or the annotation: an unknown image id, an unknown category id, a missing or malformed
    segmentation, a non-crowd RLE of another size than its image, a size ops.rle_resample refuses (outside [1, 16384], not
    inside the canvas, shrinking by more than 16), more than 1024 rows for one image."""
    if crowds not in ("negative", "reference"):
        raise ValueError(f"load_batch: crowds={crowds!r}: 'negative' or 'reference'")
    if isinstance(gt, str):
        with open(gt) as fh:
            gt = json.load(fh)
    min_dim, max_dim = int(min_dim), int(max_dim)
    image_ids = list(image_ids)
    if labels is None:
        labels = default_labels(gt)
    flips = _flips(hflip, len(image_ids))
    rows, plans = _candidates(gt, image_ids, labels, lambda h, w: _plan(h, w, min_dim, max_dim))
    _check_sizes(plans, image_ids, max_dim)
    dev = torch.device(device)
    windows = torch.tensor([p.window for p in plans], dtype=torch.int64).reshape(-1, 4)
    scales = [p.scale for p in plans]
    if not image_ids:
        return GroundTruth(torch.zeros(0, 4, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                           torch.zeros(0, max_dim, max_dim, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                           windows.to(dev), scales, flips)
    if dev.type == "cpu":
        boxes, ids, masks, off = _load_host(rows, plans, flips, max_dim, crowds)
        return GroundTruth(boxes, ids, masks, off, windows, scales, flips)
    boxes, ids, masks, off = _load_device(rows, plans, flips, max_dim, crowds, dev)
    return GroundTruth(boxes, ids, masks, off, windows.to(dev), scales, flips)
