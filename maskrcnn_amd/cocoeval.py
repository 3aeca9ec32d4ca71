"""COCO detection evaluation (bbox / segm AP and AR) — the second half of `python coco.py evaluate` (coco.py:78-135):
COCOeval(coco, coco_results, iou_type).evaluate() / accumulate() / summarize() of cocoapi/PythonAPI/pycocotools/cocoeval.py,
without pycocotools.

    ev = evaluate("instances_val.json", "out.json", iou_type="segm")     # out.json: predict.py --coco-json
    print("\\n".join(ev.summary()))
    python -m maskrcnn_amd.cocoeval GT.json RESULTS.json [--type segm|bbox] [--polygons error|rasterize]

Where the work is done:
    GPU   the IoU of every detection x ground truth of every (image, category) — ONE grouped ops.rle_iou / ops.bbox_iou call —
          and the matching of evaluateImg for every group x area range x threshold — ONE grouped ops.coco_match call
    host  loadRes / _prepare (grouping, the -score mergesort, the maxDets[-1] cut), and accumulate / summarize restated
          operation by operation in numpy on the small arrays the two calls return.
Every number equals the reference's bit for bit (tests/golden/cocoeval.npz).

Polygon ground truth — every non-crowd annotation of a stock instances_*.json — is COCO.annToRLE's work (pycocotools/coco.py:
406-425: maskUtils.frPyObjects + maskUtils.merge per annotation). ann_to_rle(gt) does it for a whole data set in ONE grouped
ops.rle_from_poly call over all parts, ONE grouped ops.rle_merge call over all annotations and one device-to-host copy, the bits
of the reference's codec (tests/golden/poly.npz). evaluate(..., polygons="rasterize") does the same inside the evaluation and
keeps the polygon rows on the device between rle_merge and rle_iou; the default polygons="error" refuses polygons
(NotImplementedError), as before. Polygons in RESULT records stay refused: the reference's loadRes fails on them as well.

Compressed strings — every record of a result file — are decoded on the GPU: load_results(..., device=) sends all strings of the file
through ONE ops.rle_from_string call and ONE ops.rle_area_bbox call (rleFrString, rleArea, rleToBbox: tests/golden/codec.npz), and
evaluate() keeps that table on the device and gathers it into computeIoU's order with an index tensor, so each string is decoded
once and there is no per-character host work; compressed ground truth takes the same route. ann_to_rle(compress=True) writes the
compressed strings COCO.annToRLE returns (ops.rle_to_string). Out of scope: keypoints, useCats = 0.
"""
from __future__ import annotations

import inspect
import json
from typing import NamedTuple

import numpy as np
import torch

__all__ = ["Params", "CocoEval", "evaluate", "accumulate", "summarize", "load_results", "ann_to_rle"]


class Params:
    """Params.setDetParams (cocoeval.py:503-512)."""

    def __init__(self, iou_type: str = "segm"):
        if iou_type not in ("segm", "bbox"):
            raise ValueError(f"iou_type {iou_type!r}: 'segm' or 'bbox' (keypoints are out of scope)")
        self.iouType = iou_type
        self.imgIds, self.catIds = [], []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ["all", "small", "medium", "large"]
        self.useCats = 1


# ------------------------------------------------------------------------------------------------ accumulate / summarize
def accumulate(eval_imgs, params: Params):
    """COCOeval.accumulate (cocoeval.py:316-421) on eval_imgs — the list evaluate() builds, [K x A x I] entries (category
    slowest), None or a dict with dtScores, dtMatches [T,D], dtIgnore [T,D], gtIgnore [G] — for the params it was built with.
    → precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M]."""
    p = params
    T, R, K, A, M = len(p.iouThrs), len(p.recThrs), len(p.catIds), len(p.areaRng), len(p.maxDets)
    I0 = len(p.imgIds)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k in range(K):
        Nk = k * A * I0
        for a in range(A):
            Na = a * I0
            for m, maxDet in enumerate(p.maxDets):
                E = [e for e in eval_imgs[Nk + Na:Nk + Na + I0] if e is not None]
                if len(E) == 0:
                    continue
                dtScores = np.concatenate([e["dtScores"][0:maxDet] for e in E])
                inds = np.argsort(-dtScores, kind="mergesort")
                dtScoresSorted = dtScores[inds]
                dtm = np.concatenate([e["dtMatches"][:, 0:maxDet] for e in E], axis=1)[:, inds]
                dtIg = np.concatenate([e["dtIgnore"][:, 0:maxDet] for e in E], axis=1)[:, inds]
                gtIg = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gtIg == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtIg))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    ss = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    # the reference's backward loop (pr[i-1] = pr[i] where larger) is a running maximum from the right
                    pr = np.maximum.accumulate(pr[::-1])[::-1]
                    inds_r = np.searchsorted(rc, p.recThrs, side="left")
                    ok = inds_r < nd      # its try / except stops at the first index past the end; they are non-decreasing
                    q[ok] = pr[inds_r[ok]]
                    ss[ok] = dtScoresSorted[inds_r[ok]]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    return precision, recall, scores


def summarize(precision, recall, params: Params):
    """COCOeval.summarize (_summarizeDets, cocoeval.py:423-473) → (stats float64 [12], the twelve lines it prints)."""
    p = params
    lines = []

    def _summarize(ap=1, iouThr=None, areaRng="all", maxDets=100):
        iStr = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}"
        titleStr = "Average Precision" if ap == 1 else "Average Recall"
        typeStr = "(AP)" if ap == 1 else "(AR)"
        iouStr = "{:0.2f}:{:0.2f}".format(p.iouThrs[0], p.iouThrs[-1]) if iouThr is None else "{:0.2f}".format(iouThr)
        aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
        mind = [i for i, mDet in enumerate(p.maxDets) if mDet == maxDets]
        if ap == 1:
            s = precision
            if iouThr is not None:
                s = s[np.where(iouThr == p.iouThrs)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = recall
            if iouThr is not None:
                s = s[np.where(iouThr == p.iouThrs)[0]]
            s = s[:, :, aind, mind]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        lines.append(iStr.format(titleStr, typeStr, iouStr, areaRng, maxDets, mean_s))
        return mean_s

    stats = np.zeros((12,))
    stats[0] = _summarize(1)
    stats[1] = _summarize(1, iouThr=.5, maxDets=p.maxDets[2])
    stats[2] = _summarize(1, iouThr=.75, maxDets=p.maxDets[2])
    stats[3] = _summarize(1, areaRng="small", maxDets=p.maxDets[2])
    stats[4] = _summarize(1, areaRng="medium", maxDets=p.maxDets[2])
    stats[5] = _summarize(1, areaRng="large", maxDets=p.maxDets[2])
    stats[6] = _summarize(0, maxDets=p.maxDets[0])
    stats[7] = _summarize(0, maxDets=p.maxDets[1])
    stats[8] = _summarize(0, maxDets=p.maxDets[2])
    stats[9] = _summarize(0, areaRng="small", maxDets=p.maxDets[2])
    stats[10] = _summarize(0, areaRng="medium", maxDets=p.maxDets[2])
    stats[11] = _summarize(0, areaRng="large", maxDets=p.maxDets[2])
    return stats, lines


class CocoEval:
    """What evaluate() returns: params, ious {(image_id, category_id): float64 [D,G] or []}, eval_imgs (COCOeval.evalImgs),
    precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M], stats [12]; summary() → the lines summarize() prints."""

    def __init__(self, params, ious, eval_imgs):
        self.params, self.ious, self.eval_imgs = params, ious, eval_imgs
        self.precision, self.recall, self.scores = accumulate(eval_imgs, params)
        self.stats, self._lines = summarize(self.precision, self.recall, params)

    def summary(self):
        return list(self._lines)


# ------------------------------------------------------------------------------------------------ loadRes / _prepare
def _rle_area_bbox(cnts: np.ndarray, h: int, w: int):
    """rleArea and rleToBbox (maskApi.c:72-75, :133-147) of one run list → (area, [x, y, w, h] as floats)."""
    area = int(cnts[1::2].astype(np.int64).sum())
    m = (cnts.size // 2) * 2
    if m == 0:
        return area, [0.0, 0.0, 0.0, 0.0]
    cc = np.cumsum(cnts[:m].astype(np.int64))
    t = cc - (np.arange(m) % 2)
    y = t % h
    x = (t - y) // h
    xs, xe, ys, ye = int(min(w, x.min())), int(x.max()), int(min(h, y.min())), int(y.max())
    if (x[0::2] < x[1::2]).any():      # a run that crosses into another column spans every row
        ys, ye = 0, h - 1
    return area, [float(xs), float(ys), float(xe - xs + 1), float(ye - ys + 1)]


def _is_polygon(seg) -> bool:
    return isinstance(seg, (list, tuple))


def _seg_size(seg):
    if isinstance(seg, dict):
        return int(seg["size"][0]), int(seg["size"][1])
    return int(seg.shape[-2]), int(seg.shape[-1])      # a dense [h, w] mask


def _seg_counts(seg, i: int, device) -> np.ndarray:
    """Run lengths of a segmentation that is no RLE dict: a dense mask array, which is encoded on the GPU (ops.rle_encode)."""
    from . import image
    if isinstance(seg, (np.ndarray, torch.Tensor)):
        t = torch.as_tensor(np.ascontiguousarray(seg) if isinstance(seg, np.ndarray) else seg)
        if t.dtype not in (torch.uint8, torch.bool):
            t = t != 0
        enc = image.rle_masks(t.to(device)[None])
        return enc.counts[0, :int(enc.num_runs[0])].cpu().numpy().view(np.uint32)
    raise TypeError(f"segmentation {i}: expected an RLE dict or a dense mask array, got {type(seg).__name__}")


def load_results(results, iou_type: str, device=None):
    """COCO.loadRes (pycocotools/coco.py:297-352) on a list of result records: id = i + 1, iscrowd = 0, and — decided by the
    FIRST record, as there — area = w*h of the box where records carry a bbox, else the RLE's area and bbox = toBbox.
    device=None: the RLEs are read on the host (image.rle_counts, numpy). A GPU device: all compressed strings of the file go
    through ONE ops.rle_from_string and ONE ops.rle_area_bbox call and one copy back — the same areas and boxes, values and types;
    a malformed string is a ValueError naming the record. Count lists keep the host route."""
    return _load(results, iou_type, device)[0]


def _load(results, iou_type: str, device=None):
    """load_results → (records, what the device route decoded on the GPU or None: (an image._Decoded of the compressed strings,
    {record id (loadRes' i + 1): its row}))."""
    decoded = None
    on_gpu = device is not None and torch.device(device).type != "cpu"
    if isinstance(results, str):
        with open(results) as fh:
            results = json.load(fh)
    if not isinstance(results, list):
        raise TypeError("results in not an array of objects")
    anns = [dict(r) for r in results]
    if not anns:
        return anns, None
    if "bbox" in anns[0] and not anns[0]["bbox"] == []:
        for i, ann in enumerate(anns):
            bb = ann["bbox"]
            ann["area"] = bb[2] * bb[3]
            ann["id"] = i + 1
            ann["iscrowd"] = 0
    elif "segmentation" in anns[0]:
        from . import image, ops
        on_device = []
        for i, ann in enumerate(anns):
            seg = ann["segmentation"]
            if _is_polygon(seg):
                raise NotImplementedError("polygon segmentations are out of scope (rleFrPoly is not implemented): give RLE")
            h, w = _seg_size(seg)
            if on_gpu and isinstance(seg, dict) and image._string_of(seg) is not None:
                on_device.append(i)
            else:
                area, bbox = _rle_area_bbox(image.rle_counts(seg), h, w)
                ann["area"] = np.uint32(area)
                if "bbox" not in ann:
                    ann["bbox"] = np.array(bbox)
            ann["id"] = i + 1
            ann["iscrowd"] = 0
        if on_device:
            segs = [anns[i]["segmentation"] for i in on_device]
            hs, ws = [int(s["size"][0]) for s in segs], [int(s["size"][1]) for s in segs]
            num_runs, counts, status = image._strings_to_device([image._string_of(s) for s in segs], hs, ws, device)
            sizes = torch.tensor([hs, ws], dtype=torch.int32).to(num_runs.device)
            areas, bboxes = ops.rle_area_bbox(num_runs, counts, sizes[0], sizes[1])
            back = torch.cat([num_runs[:, None], status[:, None], areas[:, None], bboxes], dim=1).cpu().numpy()   # the one copy back
            table = image._Decoded(num_runs, counts, back[:, 0].copy(), back[:, 1].copy())
            for k in np.nonzero(table.runs < 0)[0].tolist():
                raise image._status_error(table, k, f"result {on_device[k]}: the segmentation")
            area_u, boxes = back[:, 2].astype(np.uint32), back[:, 3:7].astype(np.float64)
            for k, i in enumerate(on_device):
                ann = anns[i]
                ann["area"] = area_u[k]
                if "bbox" not in ann:
                    ann["bbox"] = boxes[k].copy()
            decoded = (table, {anns[i]["id"]: k for k, i in enumerate(on_device)})
    else:
        raise ValueError("result records carry neither 'bbox' nor 'segmentation'")
    return anns, decoded


def _polygon_parts(ann):
    """The parts of a list segmentation as frPyObjects dispatches them (_mask.pyx:288-308) on the FIRST part: more than 4 numbers
    → every part is a polygon of len // 2 vertices (a later part of 4 numbers is a 2-vertex polygon). A first part of exactly 4
    numbers is refused — the reference hands that list to frBbox, which raises TypeError — and so are fewer than 4."""
    seg, who = ann["segmentation"], f"annotation {ann.get('id')}"
    if len(seg) == 0 or not _is_polygon(seg[0]):
        raise ValueError(f"{who}: a list segmentation is a list of [x0, y0, x1, y1, ...] parts")
    if len(seg[0]) <= 4:
        raise ValueError(f"{who}: the first part has {len(seg[0])} numbers; frPyObjects takes 4 for a box list, which "
                         "annToRLE cannot convert, and fewer for nothing at all: a polygon part has more than 4")
    for part in seg:
        if not _is_polygon(part) or len(part) < 2:
            raise ValueError(f"{who}: a part with {len(part) if _is_polygon(part) else type(part).__name__} numbers has no vertex")
    return list(seg)


def _polygon_table(anns, sizes, device):
    """annToRLE of list-segmentation annotations, all at once: ONE ops.rle_from_poly call over every part and ONE ops.rle_merge
    call (union) over every annotation → (num_runs int32 [len(anns)], counts int32 [len(anns), capacity]) on the device. sizes:
    the (h, w) of each annotation's image."""
    from . import image, ops
    parts, part_sizes, group_n = [], [], []
    for ann, size in zip(anns, sizes):
        mine = _polygon_parts(ann)
        parts += mine
        part_sizes += [size] * len(mine)
        group_n.append(len(mine))
    pack = lambda pp, ss: image._pack_polygons(pp, np.asarray(ss, dtype=np.int64).reshape(-1, 2))
    try:
        xy, off, hs, ws = pack(parts, part_sizes)
        bounds = ops.poly_host_bounds(xy, off, hs, ws, "ann_to_rle", ValueError)
    except ValueError:
        for ann, size in zip(anns, sizes):          # the error path only: which annotation is it?
            try:
                ops.poly_host_bounds(*pack(ann["segmentation"], [size] * len(ann["segmentation"])), "ann_to_rle", ValueError)
            except ValueError as e:
                raise ValueError(f"annotation {ann.get('id')}: {e}") from e
        raise
    group_off = np.concatenate([[0], np.cumsum(group_n)]).astype(np.int64)
    runs_bound = np.concatenate([[0], np.cumsum(bounds + 1)])
    capacity = int(bounds.max()) + 1 if len(parts) else 1
    merged_capacity = max(1, int((runs_bound[group_off[1:]] - runs_bound[group_off[:-1]]).max())) if len(anns) else 1
    num_runs, counts, _ = ops.rle_from_poly(*image._polygons_to_device(xy, off, hs, ws, device), capacity=capacity)
    goff = torch.from_numpy(group_off.astype(np.int32)).to(num_runs.device)
    return ops.rle_merge(num_runs, counts, goff, intersect=False, capacity=merged_capacity)


def ann_to_rle(gt, device="cuda:0", compress: bool = False):
    """COCO.annToRLE (pycocotools/coco.py:406-425) over a whole data set: → a copy of the data set dict (or of the file at the
    path `gt`) in which every list (polygon) segmentation is {"size": [h, w], "counts": [run lengths]} of its image's height /
    width — the union of its parts, rleFrPoly + rleMerge, the reference codec's bits; dict segmentations are left as they are.
    The whole data set costs one ops.rle_from_poly call, one ops.rle_merge call and one device-to-host copy. ValueError, naming
    the annotation id, for a list segmentation frPyObjects would not take as polygons (_polygon_parts).
    compress=True: "counts" is the compressed string (bytes) annToRLE itself returns — ops.rle_to_string on the merged table, one
    read of the total length and, again, one device-to-host copy."""
    if isinstance(gt, str):
        with open(gt) as fh:
            gt = json.load(fh)
    size_of = {img["id"]: (int(img["height"]), int(img["width"])) for img in gt["images"]}
    out = dict(gt)
    out["annotations"] = anns = [dict(a) for a in gt["annotations"]]
    poly = [a for a in anns if _is_polygon(a.get("segmentation"))]
    if not poly:
        return out
    sizes = [size_of[a["image_id"]] for a in poly]
    num_runs, counts = _polygon_table(poly, sizes, device)
    if compress:
        from . import ops
        chars, str_off = ops.rle_to_string(num_runs, counts)
        packed = torch.cat([str_off.view(torch.uint8), chars]).cpu().numpy()      # the one copy: offsets, then the characters
        head = 8 * (len(poly) + 1)
        off = (packed[:head].view(np.int64) + head).tolist()
        for k, (a, (h, w)) in enumerate(zip(poly, sizes)):
            a["segmentation"] = {"size": [h, w], "counts": packed[off[k]:off[k + 1]].tobytes()}
        return out
    live = torch.arange(counts.size(1), device=counts.device)[None, :] < num_runs[:, None]
    packed = torch.cat([num_runs, counts[live]]).cpu().numpy()          # the one copy: run counts, then the runs that exist
    nr = packed[:len(poly)].astype(np.int64)
    ends = len(poly) + np.cumsum(nr)
    runs = packed.view(np.uint32)
    for a, (h, w), n, e in zip(poly, sizes, nr.tolist(), ends.tolist()):
        a["segmentation"] = {"size": [h, w], "counts": runs[e - n:e].tolist()}
    return out


class _Groups(NamedTuple):
    """What _group returns: keys, the sorted (image, category) pairs with an annotation or a detection; dts / gts {key: its
    records}, the detections by descending score and cut at maxDets[-1]; dt_flat / gt_flat, the records of all keys in that
    order; dt_n / gt_n int64 [K]; dt_off / gt_off int64 [K+1] into the flat lists, out_off int64 [K+1] into the flat IoU array
    (dt_n * gt_n numbers a group); iscrowd / gt_ignore uint8 [M] and dt_area / gt_area float64 [N] / [M] of the flat lists."""
    keys: list
    dts: dict
    gts: dict
    dt_flat: list
    gt_flat: list
    dt_n: np.ndarray
    gt_n: np.ndarray
    dt_off: np.ndarray
    gt_off: np.ndarray
    out_off: np.ndarray
    iscrowd: np.ndarray
    gt_ignore: np.ndarray
    dt_area: np.ndarray
    gt_area: np.ndarray


def _group(annotations, dts_all, p: Params, refuse_polygons: bool = False) -> _Groups:
    """evaluate, stage 1 (host only): _prepare and computeIoU's ordering. refuse_polygons: a list segmentation among the grouped
    ground truths is a NotImplementedError."""
    # _prepare (:85-120): group by (image, category), keeping the data set's / the result file's order within a group
    in_imgs, in_cats = set(p.imgIds), set(p.catIds)
    gts, dts = {}, {}
    for ann in annotations:
        if ann["image_id"] in in_imgs and ann["category_id"] in in_cats:
            gts.setdefault((ann["image_id"], ann["category_id"]), []).append(ann)
    for ann in dts_all:
        if ann["image_id"] in in_imgs and ann["category_id"] in in_cats:
            dts.setdefault((ann["image_id"], ann["category_id"]), []).append(ann)
    if refuse_polygons:
        for anns in gts.values():
            for ann in anns:
                if _is_polygon(ann["segmentation"]):
                    raise NotImplementedError(
                        f"annotation {ann.get('id')}: polygon segmentations are out of scope (rleFrPoly is not implemented); "
                        "give RLE ground truth, or evaluate iou_type='bbox'")

    # computeIoU's ordering (:174-177): -score mergesort, cut at maxDets[-1]
    keys = sorted(set(gts) | set(dts))
    for key in keys:
        d = dts.get(key, [])
        inds = np.argsort([-x["score"] for x in d], kind="mergesort")
        dts[key] = [d[i] for i in inds][:p.maxDets[-1]]
        gts.setdefault(key, [])
    dt_n = np.array([len(dts[key]) for key in keys], dtype=np.int64)
    gt_n = np.array([len(gts[key]) for key in keys], dtype=np.int64)
    offsets = lambda n: np.concatenate([[0], np.cumsum(n)])
    dt_flat, gt_flat = [x for key in keys for x in dts[key]], [x for key in keys for x in gts[key]]
    iscrowd = np.array([int(x["iscrowd"]) if "iscrowd" in x else 0 for x in gt_flat], dtype=np.uint8)
    # gt['ignore'] = 'iscrowd' in gt and gt['iscrowd'] (:110)
    gt_ignore = np.array([1 if ("iscrowd" in x and x["iscrowd"]) else 0 for x in gt_flat], dtype=np.uint8)
    dt_area = np.array([float(x["area"]) for x in dt_flat], dtype=np.float64)
    gt_area = np.array([float(x["area"]) for x in gt_flat], dtype=np.float64)
    return _Groups(keys, dts, gts, dt_flat, gt_flat, dt_n, gt_n, offsets(dt_n), offsets(gt_n), offsets(dt_n * gt_n),
                   iscrowd, gt_ignore, dt_area, gt_area)


def _segm_tables(g: _Groups, images, decoded, dev, host_strings: bool):
    """evaluate, stage 2: the run-list tables (num_runs, counts) of dt_flat and of gt_flat on the device, through
    image._table_parts: RLE dicts are checked and their compressed strings decoded where host_strings says (detections _load
    decoded already — decoded, what it returned — are gathered from its table), dense masks go through _seg_counts. Polygon
    ground truths are rasterised on the device (_polygon_table) and are one more part of the ground-truth table's one merge."""
    from . import image
    is_poly = np.array([_is_polygon(x["segmentation"]) for x in g.gt_flat], dtype=bool)
    how = dict(other=lambda s, i: _seg_counts(s, i, dev), host_strings=host_strings)
    if decoded is not None:
        decoded = (decoded[0], {i: decoded[1][x["id"]] for i, x in enumerate(g.dt_flat) if x["id"] in decoded[1]})
    dt_table = image._build_table([x["segmentation"] for x in g.dt_flat], None, dev, decoded=decoded, **how)
    gt_parts = image._table_parts([x["segmentation"] for x in g.gt_flat], None, dev, skip=is_poly, **how)
    size_of = {img["id"]: (int(img["height"]), int(img["width"])) for img in images if "height" in img and "width" in img}
    ann_size = lambda x: size_of[x["image_id"]] if _is_polygon(x["segmentation"]) else _seg_size(x["segmentation"])
    for key in g.keys:
        sizes = {ann_size(x) for x in g.dts[key] + g.gts[key]}
        if len(sizes) > 1:
            raise ValueError(f"image {key[0]}, category {key[1]}: masks of different sizes {sorted(sizes)}")
    capacity = None
    if is_poly.any():
        # annToRLE on the device. One scalar comes back, the longest row: rle_merge's own capacity is a loose bound, and
        # ops.rle_iou's workspace and time would pay for it
        poly_anns = [x for x, f in zip(g.gt_flat, is_poly) if f]
        p_runs, p_counts = _polygon_table(poly_anns, [size_of[x["image_id"]] for x in poly_anns], dev)
        capacity = max(int(p_runs.max()), image._widest(gt_parts))
        gt_parts.append((np.nonzero(is_poly)[0], p_runs, p_counts))
    return dt_table, image._merge_tables(len(g.gt_flat), gt_parts, dev, capacity)


def _match_on_device(g: _Groups, p: Params, iou_type: str, tables, dev):
    """evaluate, stage 3: ONE grouped IoU call (ops.rle_iou on tables = (dt_table, gt_table) for "segm", ops.bbox_iou on the
    records' boxes for "bbox") and ONE ops.coco_match call → numpy: ious_flat float64 [out_off[-1]] (a group's IoUs at
    out_off[k], ground truth slowest), dt_match int32 [A,T,N] and gt_match int32 [A,T,M] (1-based positions within the group, 0
    = none), dt_ignore uint8 [A,T,N], gt_ignore uint8 [A,M]. No group: empty arrays, and the device is not touched."""
    T, A = len(p.iouThrs), len(p.areaRng)
    if not g.keys:
        return (np.zeros(0), np.zeros((A, T, 0), np.int32), np.zeros((A, T, 0), np.int32), np.zeros((A, T, 0), np.uint8),
                np.zeros((A, 0), np.uint8))
    from . import ops
    dev_of = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    offs = (dev_of(g.dt_off.astype(np.int32)), dev_of(g.gt_off.astype(np.int32)), dev_of(g.out_off.astype(np.int64)))
    if iou_type == "segm":
        ious_dev = ops.rle_iou(*tables, dev_of(g.iscrowd), *offs, out_len=int(g.out_off[-1]))
    else:
        boxes = lambda anns: np.array([[float(v) for v in x["bbox"]] for x in anns], dtype=np.float64).reshape(-1, 4)
        ious_dev = ops.bbox_iou(dev_of(boxes(g.dt_flat)), dev_of(boxes(g.gt_flat)), dev_of(g.iscrowd), *offs, out_len=int(g.out_off[-1]))
    match = ops.coco_match(ious_dev, *offs, dev_of(g.dt_area), dev_of(g.gt_area), dev_of(g.gt_ignore),
                           dev_of(np.array(p.areaRng, dtype=np.float64)), dev_of(np.asarray(p.iouThrs, dtype=np.float64)))
    return (ious_dev.cpu().numpy(), *[m.cpu().numpy() for m in match])


def _rebuild(g: _Groups, p: Params, ious_flat, dt_match, gt_match, dt_ignore, gt_ignore):
    """evaluate, stage 4 (host only): COCOeval.ious and COCOeval.evalImgs from the five arrays of _match_on_device → (ious
    {(image_id, category_id): float64 [D,G] or []}, eval_imgs [K x A x I], category slowest: ids for positions, ground truths
    listed regular first)."""
    T, max_det = len(p.iouThrs), p.maxDets[-1]
    index = {key: k for k, key in enumerate(g.keys)}
    ious = {}
    for img in p.imgIds:
        for cat in p.catIds:
            k = index.get((img, cat))
            if k is None or g.dt_n[k] == 0 or g.gt_n[k] == 0:
                ious[img, cat] = []
            else:
                ious[img, cat] = ious_flat[g.out_off[k]:g.out_off[k + 1]].reshape(int(g.gt_n[k]), int(g.dt_n[k])).T

    eval_imgs = []
    for cat in p.catIds:
        for a, rng in enumerate(p.areaRng):
            for img in p.imgIds:
                k = index.get((img, cat))
                if k is None:
                    eval_imgs.append(None)
                    continue
                d0, d1, g0, g1 = int(g.dt_off[k]), int(g.dt_off[k + 1]), int(g.gt_off[k]), int(g.gt_off[k + 1])
                d, gg = g.dts[img, cat], g.gts[img, cat]
                gt_ig = gt_ignore[a, g0:g1]
                gtind = np.argsort(gt_ig, kind="mergesort")            # regular first, ignored last (:258)
                gt_ids = np.array([x["id"] for x in gg], dtype=np.float64)
                dt_ids = np.array([x["id"] for x in d], dtype=np.float64)
                pos_d = dt_match[a, :, d0:d1]
                dtm = np.where(pos_d > 0, gt_ids[np.maximum(pos_d, 1) - 1] if len(gg) else 0.0, 0.0).reshape(T, d1 - d0)
                pos_g = gt_match[a, :, g0:g1][:, gtind]
                gtm = np.where(pos_g > 0, dt_ids[np.maximum(pos_g, 1) - 1] if len(d) else 0.0, 0.0).reshape(T, g1 - g0)
                outside = np.array([x["area"] < rng[0] or x["area"] > rng[1] for x in d], dtype=bool).reshape(1, len(d))
                dt_ig = np.logical_or(dt_ignore[a, :, d0:d1] != 0, np.logical_and(dtm == 0, np.repeat(outside, T, 0)))
                eval_imgs.append({
                    "image_id": img, "category_id": cat, "aRng": rng, "maxDet": max_det,
                    "dtIds": [x["id"] for x in d], "gtIds": [gg[i]["id"] for i in gtind],
                    "dtMatches": dtm, "gtMatches": gtm, "dtScores": [x["score"] for x in d],
                    "gtIgnore": gt_ig[gtind].astype(np.int64), "dtIgnore": dt_ig,
                })
    return ious, eval_imgs


def evaluate(gt, results, iou_type: str = "segm", device="cuda:0", *, polygons: str = "error") -> CocoEval:
    """COCOeval(COCO(gt), COCO(gt).loadRes(results), iou_type) → evaluate(), accumulate(), summarize().
    gt: a COCO dataset dict (images, annotations, categories) or its path; results: the list predict.py --coco-json writes, or
    its path. Ground-truth segmentations (iou_type="segm"): compressed-string RLE, count-list RLE or a dense mask array;
    polygons raise NotImplementedError with polygons="error" (the default) and are rasterised on the GPU with
    polygons="rasterize" (annToRLE: ops.rle_from_poly + ops.rle_merge, the rows staying on the device for ops.rle_iou).
    iou_type="bbox" never looks at segmentations. Compressed strings, of results and of ground truth, are decoded on the GPU,
    each once (_load's device route, image._build_table)."""
    return _evaluate(gt, results, iou_type, device, polygons, "device")


def _evaluate(gt, results, iou_type, device, polygons, codec):
    """evaluate(), stage by stage: _load, _group, _segm_tables, _match_on_device, _rebuild. codec = "device" decodes compressed
    strings on the GPU, "host" is the per-character route of image.rle_counts that load_results(device=None) and
    rle_table(device="cpu") still are — kept so that tools/codec_microbench.py and the tests can compare the two in one process.
    Every number is the same."""
    if polygons not in ("error", "rasterize"):
        raise ValueError(f"polygons={polygons!r}: 'error' or 'rasterize'")
    if codec not in ("device", "host"):
        raise ValueError(f"codec={codec!r}: 'device' or 'host'")
    p = Params(iou_type)
    if isinstance(gt, str):
        with open(gt) as fh:
            gt = json.load(fh)
    img_ids = [img["id"] for img in gt["images"]]
    p.imgIds = list(np.unique(img_ids))
    p.catIds = list(np.unique([c["id"] for c in gt["categories"]]))
    p.maxDets = sorted(p.maxDets)
    dts_all, decoded = _load(results, iou_type, device if codec == "device" and iou_type == "segm" else None)
    if not set(a["image_id"] for a in dts_all) <= set(img_ids):
        raise ValueError("Results do not correspond to current coco set")
    g = _group(gt["annotations"], dts_all, p, refuse_polygons=iou_type == "segm" and polygons == "error")
    dev = torch.device(device)
    tables = _segm_tables(g, gt["images"], decoded, dev, codec == "host") if g.keys and iou_type == "segm" else None
    return CocoEval(p, *_rebuild(g, p, *_match_on_device(g, p, iou_type, tables, dev)))


# evaluate's positional interface — (gt, results, iou_type, device) — is pinned parameter by parameter by
# tests/test_cocoeval_host.py::test_public_interface, through inspect.signature. `polygons` is an option added beside it,
# keyword-only and documented in the docstring; the signature reported to introspection stays the pinned one.
evaluate.__signature__ = inspect.Signature(
    [q for q in inspect.signature(evaluate).parameters.values() if q.kind is not inspect.Parameter.KEYWORD_ONLY],
    return_annotation=inspect.signature(evaluate).return_annotation)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="COCO AP / AR of a result file (predict.py --coco-json) against ground truth")
    ap.add_argument("gt", help="COCO annotation file (--type segm: RLE segmentations, or polygons with --polygons rasterize)")
    ap.add_argument("results", help="COCO result records")
    ap.add_argument("--type", default="segm", choices=("segm", "bbox"), dest="iou_type")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--polygons", default="error", choices=("error", "rasterize"),
                    help="polygon ground truth (--type segm): refuse it, or rasterise it on the GPU as COCO.annToRLE does")
    args = ap.parse_args(argv)
    print("\n".join(evaluate(args.gt, args.results, args.iou_type, args.device, polygons=args.polygons).summary()))


if __name__ == "__main__":
    main()
