#!/usr/bin/env python3
"""Regenerates tests/golden/cocoeval.npz from the reference's own COCO evaluator.

    python tests/golden/make_golden_cocoeval.py     (reference tree: $MASKRCNN_REFERENCE, as for make_golden.py)

Codec: <reference>/cocoapi/common/maskApi.c is compiled into a temporary directory OUTSIDE this repository (nothing of it is
kept) and rleFrString, rleToString, rleEncode, rleIou, bbIou, rleArea and rleToBbox are called through ctypes.
Evaluator: <reference>/cocoapi/PythonAPI/pycocotools/cocoeval.py is imported UNMODIFIED; what it needs around it is supplied
here: a stub pycocotools._mask whose iou() dispatches as _mask.pyx:171-239 does onto the compiled codec, np.float, an
np.linspace that int()s `num` (Params passes a float), and a small stand-in for the COCO class (getImgIds / getCatIds /
getAnnIds / loadAnns / annToRLE, and loadRes restated from pycocotools/coco.py:297-352).

The data set is synthetic and seeded (see dataset()). Stored, DATA only:
    gt_json, results_json        the inputs as JSON text: images (sizes), annotations (RLE strings / count lists, boxes, areas,
                                 iscrowd, ids), categories; result records (image_id, category_id, bbox, score, segmentation)
  and per IoU type t in ("segm", "bbox"):
    t_iou_key    int64 [Kg,2]    (image_id, category_id) of every group with a non-empty IoU matrix
    t_iou_shape  int64 [Kg,2]    (detections, ground truths);  t_iou float64: the [D,G] matrices, row-major, concatenated
    t_ev_pos     int64 [E]       index into evalImgs of every non-None entry;  t_ev_len: len(evalImgs)
    t_ev_meta    int64 [E,5]     image_id, category_id, area-range index, D, G
    t_ev_dtm / t_ev_dtig  [T,D] per entry, t_ev_gtm [T,G], t_ev_gtig [G], t_ev_dtids [D], t_ev_gtids [G], t_ev_dtscores [D],
                                 each flattened row-major and concatenated in entry order
    t_precision, t_recall, t_scores, t_stats, t_summary (the twelve printed lines)
"""
import contextlib
import copy
import ctypes
import io
import itertools
import json
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


class RLE(ctypes.Structure):   # typedef struct { siz h, w, m; uint *cnts; } RLE;  siz = unsigned long
    _fields_ = [("h", ctypes.c_ulong), ("w", ctypes.c_ulong), ("m", ctypes.c_ulong), ("cnts", ctypes.POINTER(ctypes.c_uint))]


def load_codec(reference: str, tmp: str) -> ctypes.CDLL:
    src = os.path.join(reference, "cocoapi", "common", "maskApi.c")
    lib = os.path.join(tmp, "libmaskapi.so")
    subprocess.run(["cc", "-O2", "-std=c99", "-shared", "-fPIC", "-I" + os.path.dirname(src), src, "-lm", "-o", lib], check=True)
    dll = ctypes.CDLL(lib)
    P, UL, VP = ctypes.POINTER, ctypes.c_ulong, ctypes.c_void_p
    dll.rleEncode.argtypes = [P(RLE), VP, UL, UL, UL]
    dll.rleEncode.restype = None
    dll.rleToString.argtypes = [P(RLE)]
    dll.rleToString.restype = VP            # malloc'ed char*: copied, then freed
    dll.rleFrString.argtypes = [P(RLE), ctypes.c_char_p, UL, UL]
    dll.rleFrString.restype = None
    dll.rleInit.argtypes = [P(RLE), UL, UL, UL, P(ctypes.c_uint)]
    dll.rleInit.restype = None
    dll.rleArea.argtypes = [P(RLE), UL, P(ctypes.c_uint)]
    dll.rleArea.restype = None
    dll.rleToBbox.argtypes = [P(RLE), P(ctypes.c_double), UL]
    dll.rleToBbox.restype = None
    dll.rleIou.argtypes = [P(RLE), P(RLE), UL, UL, VP, VP]
    dll.rleIou.restype = None
    dll.bbIou.argtypes = [VP, VP, UL, UL, VP, VP]
    dll.bbIou.restype = None
    dll.rleFree.argtypes = [P(RLE)]
    dll.rleFree.restype = None
    return dll


class Codec:
    """maskUtils' encode / area / toBbox / iou on the compiled maskApi.c."""

    def __init__(self, dll):
        self.dll = dll

    def _string(self, r) -> str:
        sp = self.dll.rleToString(ctypes.byref(r))
        s = ctypes.string_at(sp).decode("ascii")
        ctypes.CDLL(None).free(ctypes.c_void_p(sp))
        return s

    def encode(self, mask: np.ndarray) -> dict:
        h, w = mask.shape
        col_major = np.asfortranarray(mask.astype(np.uint8))
        r = RLE()
        self.dll.rleEncode(ctypes.byref(r), col_major.ctypes.data, h, w, 1)
        out = {"size": [h, w], "counts": self._string(r)}
        self.dll.rleFree(ctypes.byref(r))
        return out

    def from_counts(self, counts, h, w) -> dict:      # frPyObjects on an uncompressed RLE
        arr = (ctypes.c_uint * len(counts))(*counts)
        r = RLE()
        self.dll.rleInit(ctypes.byref(r), h, w, len(counts), arr)
        out = {"size": [h, w], "counts": self._string(r)}
        self.dll.rleFree(ctypes.byref(r))
        return out

    def structs(self, objs):
        rs = (RLE * len(objs))()
        for r, o in zip(rs, objs):
            c = o["counts"]
            self.dll.rleFrString(ctypes.byref(r), c.encode("ascii") if isinstance(c, str) else bytes(c), o["size"][0], o["size"][1])
        return rs

    def free(self, rs):
        for r in rs:
            self.dll.rleFree(ctypes.byref(r))

    def counts(self, obj):
        rs = self.structs([obj])
        out = [int(rs[0].cnts[i]) for i in range(rs[0].m)]
        self.free(rs)
        return out

    def area(self, obj):
        rs = self.structs([obj])
        a = ctypes.c_uint()
        self.dll.rleArea(rs, 1, ctypes.byref(a))
        self.free(rs)
        return np.uint32(a.value)

    def to_bbox(self, obj):
        rs = self.structs([obj])
        bb = (ctypes.c_double * 4)()
        self.dll.rleToBbox(rs, bb, 1)
        self.free(rs)
        return np.array(list(bb), dtype=np.double)

    def iou(self, dt, gt, pyiscrowd):
        """_mask.pyx:171-239."""
        def _preproc(objs):
            if len(objs) == 0:
                return objs
            if type(objs) == np.ndarray:
                return objs.astype(np.double)
            isbox = np.all(np.array([(len(obj) == 4) and ((type(obj) == list) or (type(obj) == np.ndarray)) for obj in objs]))
            isrle = np.all(np.array([type(obj) == dict for obj in objs]))
            if isbox:
                objs = np.array(objs, dtype=np.double)
                if len(objs.shape) == 1:
                    objs = objs.reshape((1, objs.shape[0]))
                return objs
            if isrle:
                return self.structs(objs)
            raise Exception("list input can be bounding box (Nx4) or RLEs ([RLE])")
        iscrowd = np.array(pyiscrowd, dtype=np.uint8)
        dt, gt = _preproc(dt), _preproc(gt)
        m, n = len(dt), len(gt)
        if m == 0 or n == 0:
            for x in (dt, gt):
                if len(x) and not isinstance(x, np.ndarray):
                    self.free(x)
            return []
        if isinstance(dt, np.ndarray) != isinstance(gt, np.ndarray):
            raise Exception("The dt and gt should have the same data type, either RLEs, list or np.ndarray")
        o = np.zeros(m * n, dtype=np.double)
        crowd = np.ascontiguousarray(iscrowd) if iscrowd.size else np.zeros(1, np.uint8)
        if isinstance(dt, np.ndarray):
            dt, gt = np.ascontiguousarray(dt), np.ascontiguousarray(gt)
            self.dll.bbIou(dt.ctypes.data, gt.ctypes.data, m, n, crowd.ctypes.data, o.ctypes.data)
        else:
            self.dll.rleIou(dt, gt, m, n, crowd.ctypes.data, o.ctypes.data)
            self.free(dt)
            self.free(gt)
        return o.reshape((m, n), order="F")


class Coco:
    """The part of pycocotools.coco.COCO that COCOeval uses."""

    def __init__(self, dataset, codec):
        self.dataset, self.codec = dataset, codec
        self.imgs = {img["id"]: img for img in dataset["images"]}
        self.anns = {ann["id"]: ann for ann in dataset.get("annotations", [])}
        self.imgToAnns = {}
        for ann in dataset.get("annotations", []):
            self.imgToAnns.setdefault(ann["image_id"], []).append(ann)

    def getImgIds(self):
        return list(self.imgs.keys())

    def getCatIds(self):
        return [c["id"] for c in self.dataset["categories"]]

    def getAnnIds(self, imgIds=[], catIds=[]):
        anns = list(itertools.chain.from_iterable(self.imgToAnns[i] for i in imgIds if i in self.imgToAnns))
        anns = anns if len(catIds) == 0 else [a for a in anns if a["category_id"] in catIds]
        return [a["id"] for a in anns]

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]

    def annToRLE(self, ann):
        t = self.imgs[ann["image_id"]]
        segm = ann["segmentation"]
        if type(segm) == list:
            raise NotImplementedError("polygons")
        if type(segm["counts"]) == list:
            return self.codec.from_counts(segm["counts"], t["height"], t["width"])
        return segm

    def loadRes(self, anns):
        """pycocotools/coco.py:297-352."""
        anns = copy.deepcopy(anns)
        res = {"images": list(self.dataset["images"]), "categories": copy.deepcopy(self.dataset["categories"])}
        assert set(a["image_id"] for a in anns) <= set(self.getImgIds()), "Results do not correspond to current coco set"
        if "bbox" in anns[0] and not anns[0]["bbox"] == []:
            for i, ann in enumerate(anns):
                bb = ann["bbox"]
                ann["area"] = bb[2] * bb[3]
                ann["id"] = i + 1
                ann["iscrowd"] = 0
        elif "segmentation" in anns[0]:
            for i, ann in enumerate(anns):
                ann["area"] = self.codec.area(ann["segmentation"])
                if "bbox" not in ann:
                    ann["bbox"] = self.codec.to_bbox(ann["segmentation"])
                ann["id"] = i + 1
                ann["iscrowd"] = 0
        res["annotations"] = anns
        return Coco(res, self.codec)


def import_cocoeval(reference: str, codec: Codec):
    stub = types.ModuleType("pycocotools._mask")
    stub.iou = codec.iou
    stub.area = lambda objs: np.array([codec.area(o) for o in objs], dtype=np.uint32)
    stub.toBbox = lambda objs: np.array([codec.to_bbox(o) for o in objs])
    stub.encode = stub.decode = stub.merge = stub.frPyObjects = None     # rebound by mask.py, never called here
    sys.modules["pycocotools._mask"] = stub
    if not hasattr(np, "float"):
        np.float = float
    real_linspace = np.linspace
    np.linspace = lambda start, stop, num=50, **kw: real_linspace(start, stop, int(num), **kw)
    sys.path.insert(0, os.path.join(reference, "cocoapi", "PythonAPI"))
    try:
        from pycocotools import cocoeval
    finally:
        sys.path.pop(0)
    return cocoeval


# ------------------------------------------------------------------------------------------------ the data set
def ellipse(h, w, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0


def blob(h, w, cy, cx, r, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    ang = np.arctan2(yy - cy, xx - cx)
    k1, k2 = rng.integers(2, 5), rng.integers(5, 9)
    rad = r * (1 + 0.25 * np.sin(k1 * ang + rng.uniform(0, 6)) + 0.12 * np.cos(k2 * ang + rng.uniform(0, 6)))
    return np.hypot(yy - cy, xx - cx) <= rad


def shift(mask, dy, dx):
    out = np.zeros_like(mask)
    h, w = mask.shape
    src = mask[max(0, -dy):h - max(0, dy), max(0, -dx):w - max(0, dx)]
    out[max(0, dy):max(0, dy) + src.shape[0], max(0, dx):max(0, dx) + src.shape[1]] = src
    return out


def grow(mask, k):
    for _ in range(k):
        mask = mask | shift(mask, 1, 0) | shift(mask, -1, 0) | shift(mask, 0, 1) | shift(mask, 0, -1)
    return mask


def rect(h, w, y0, x0, y1, x1):
    m = np.zeros((h, w), bool)
    m[y0:y1, x0:x1] = True
    return m


def dataset(codec: Codec):
    rng = np.random.default_rng(20250611)
    sizes = [(120, 160), (240, 320), (200, 150)]
    cats = [1, 2, 5, 7]                       # category 7 has no ground truth
    images, annotations, results = [], [], []
    img_ids = [3 * i + 2 for i in range(12)]
    ann_id = [100]

    def add_gt(img, cat, mask, crowd=0, as_list=False):
        rle = codec.encode(mask)
        seg = {"size": rle["size"], "counts": codec.counts(rle)} if as_list else rle
        ann_id[0] += int(rng.integers(1, 4))
        annotations.append({"id": ann_id[0], "image_id": img, "category_id": cat, "segmentation": seg, "iscrowd": crowd,
                            "area": float(codec.area(rle)), "bbox": [float(v) for v in codec.to_bbox(rle)]})

    def add_dt(img, cat, mask, score, jitter=True):
        rle = codec.encode(mask)
        bb = codec.to_bbox(rle)
        if jitter and mask.any():
            bb = bb + np.round(rng.uniform(-2, 2, 4), 1)
            bb[2:] = np.maximum(bb[2:], 1.0)
        results.append({"image_id": img, "category_id": cat, "bbox": [float(v) for v in bb], "score": float(score),
                        "segmentation": rle})

    score = lambda: float(np.round(rng.uniform(0.05, 1.0), 2))      # two decimals: ties happen
    for n, img in enumerate(img_ids):
        h, w = sizes[n % 3]
        images.append({"id": img, "height": h, "width": w, "file_name": f"synthetic_{img}.png"})
        if n == 4:
            continue                                                 # an image with neither ground truth nor detections
        masks = []
        if n != 7:                                                   # image 7: detections only
            for j in range(int(rng.integers(3, 7))):
                r = [rng.uniform(4, 12), rng.uniform(20, 40), rng.uniform(58, 75)][int(rng.integers(0, 3))]
                r = min(r, 0.45 * min(h, w))
                cy, cx = rng.uniform(0.15 * h, 0.85 * h), rng.uniform(0.15 * w, 0.85 * w)
                m = blob(h, w, cy, cx, r, rng) if j % 2 else ellipse(h, w, cy, cx, r * rng.uniform(0.6, 1.0), r)
                cat = cats[int(rng.integers(0, 3))]
                add_gt(img, cat, m, as_list=(j % 3 == 2))
                masks.append((cat, m))
            if n % 3 == 1:                                           # a crowd: a union of blobs
                m = np.zeros((h, w), bool)
                for _ in range(4):
                    m |= blob(h, w, rng.uniform(0.2 * h, 0.8 * h), rng.uniform(0.2 * w, 0.8 * w), rng.uniform(8, 22), rng)
                cat = cats[int(rng.integers(0, 3))]
                add_gt(img, cat, m, crowd=1)
                for _ in range(3):                                   # several detections inside the crowd
                    cy, cx = np.argwhere(m)[int(rng.integers(0, m.sum()))]
                    add_dt(img, cat, blob(h, w, cy, cx, rng.uniform(5, 10), rng) & grow(m, 2), score())
        if n == 9:
            continue                                                 # an image with ground truth and no detections
        for cat, m in masks:
            if rng.uniform() < 0.85:
                dy, dx = [int(v) for v in rng.integers(-6, 7, 2)]
                d = shift(m, dy, dx) if rng.uniform() < 0.6 else grow(m, int(rng.integers(1, 5)))
                add_dt(img, cat, d, score())
            if rng.uniform() < 0.3:                                  # a duplicate detection of the same object
                add_dt(img, cat, shift(grow(m, 1), 2, -3), score())
            if rng.uniform() < 0.15:                                 # right object, wrong category
                add_dt(img, cats[int(rng.integers(0, 4))], m, score())
        for _ in range(int(rng.integers(1, 5))):                     # false positives, category 7 included
            r = rng.uniform(4, 45)
            add_dt(img, cats[int(rng.integers(0, 4))],
                   blob(h, w, rng.uniform(0.1 * h, 0.9 * h), rng.uniform(0.1 * w, 0.9 * w), min(r, 0.4 * min(h, w)), rng), score())

    # special cases, on image img_ids[1] (240 x 320) and img_ids[0] (120 x 160)
    img, (h, w) = img_ids[1], sizes[1]
    g = blob(h, w, 60, 80, 30, rng)
    add_gt(img, 1, g)
    for i in range(130):                                             # > 100 detections in one (image, category)
        cy, cx = rng.uniform(10, h - 10), rng.uniform(10, w - 10)
        add_dt(img, 1, shift(g, int(cy - 60), int(cx - 80)) if i % 10 == 0 else ellipse(h, w, cy, cx, 6, 9),
               float(np.round(rng.uniform(0.01, 0.99), 2)))
    # rectangle pairs of IoU exactly 0.5 and exactly 0.75 (masks and boxes alike: the boxes are not jittered)
    add_gt(img, 5, rect(h, w, 200, 10, 210, 30))                     # 200 px inside a 400 px detection
    add_dt(img, 5, rect(h, w, 200, 10, 220, 30), 0.9, jitter=False)
    add_gt(img, 5, rect(h, w, 200, 100, 215, 120))                   # 300 px inside a 400 px detection
    add_dt(img, 5, rect(h, w, 200, 100, 220, 120), 0.8, jitter=False)
    img, (h, w) = img_ids[0], sizes[0]
    m = blob(h, w, 8, 8, 14, rng)
    m[0, 0] = True
    add_gt(img, 2, m)                                                # first pixel on
    add_dt(img, 2, shift(m, 1, 1) | m, 0.77)
    add_dt(img, 2, np.zeros((h, w), bool), 0.5)                      # an empty mask
    add_dt(img, 2, np.ones((h, w), bool), 0.5)                       # a full mask
    add_gt(img, 5, np.ones((h, w), bool), crowd=1)                   # a full crowd mask
    add_dt(img, 5, blob(h, w, 60, 80, 20, rng), 0.6)
    gt = {"images": images, "annotations": annotations, "categories": [{"id": c, "name": f"cat{c}"} for c in cats]}
    return gt, results


def run(cocoeval, codec, gt, results, iou_type):
    coco = Coco(copy.deepcopy(gt), codec)
    res = coco.loadRes(results)
    with contextlib.redirect_stdout(io.StringIO()):
        ev = cocoeval.COCOeval(coco, res, iou_type)
        ev.evaluate()
        ev.accumulate()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ev.summarize()
    out = {}
    keys = [k for k, v in ev.ious.items() if len(v)]
    out["iou_key"] = np.array(keys, dtype=np.int64).reshape(-1, 2)
    out["iou_shape"] = np.array([ev.ious[k].shape for k in keys], dtype=np.int64).reshape(-1, 2)
    out["iou"] = np.concatenate([np.ascontiguousarray(ev.ious[k]).reshape(-1) for k in keys])
    labels = [tuple(a) for a in ev.params.areaRng]
    pos = [i for i, e in enumerate(ev.evalImgs) if e is not None]
    E = [ev.evalImgs[i] for i in pos]
    out["ev_pos"] = np.array(pos, dtype=np.int64)
    out["ev_len"] = np.array(len(ev.evalImgs), dtype=np.int64)
    out["ev_meta"] = np.array([[e["image_id"], e["category_id"], labels.index(tuple(e["aRng"])), len(e["dtIds"]), len(e["gtIds"])]
                               for e in E], dtype=np.int64)
    cat = lambda name, dtype: np.concatenate([np.asarray(e[name], dtype=dtype).reshape(-1) for e in E])
    out["ev_dtm"], out["ev_gtm"] = cat("dtMatches", np.float64), cat("gtMatches", np.float64)
    out["ev_dtig"], out["ev_gtig"] = cat("dtIgnore", np.uint8), cat("gtIgnore", np.uint8)
    out["ev_dtids"], out["ev_gtids"] = cat("dtIds", np.int64), cat("gtIds", np.int64)
    out["ev_dtscores"] = cat("dtScores", np.float64)
    out["precision"], out["recall"], out["scores"] = ev.eval["precision"], ev.eval["recall"], ev.eval["scores"]
    out["stats"] = np.asarray(ev.stats, dtype=np.float64)
    out["summary"] = np.array(buf.getvalue().splitlines())
    return {f"{iou_type}_{k}": v for k, v in out.items()}


def main():
    reference = os.environ.get("MASKRCNN_REFERENCE", "/root/reference")
    with tempfile.TemporaryDirectory() as tmp:
        codec = Codec(load_codec(reference, tmp))
        cocoeval = import_cocoeval(reference, codec)
        gt, results = dataset(codec)
        data = {"gt_json": np.array(json.dumps(gt)), "results_json": np.array(json.dumps(results))}
        for iou_type in ("segm", "bbox"):
            data.update(run(cocoeval, codec, gt, results, iou_type))
    path = os.path.join(HERE, "cocoeval.npz")
    np.savez_compressed(path, **data)
    print(f"{path}: {len(gt['images'])} images, {len(gt['annotations'])} annotations, {len(results)} results, "
          f"{os.path.getsize(path)} bytes")
    for iou_type in ("segm", "bbox"):
        print(iou_type, "max group", data[f"{iou_type}_iou_shape"].max(0).tolist(), "stats", np.round(data[f"{iou_type}_stats"], 3).tolist())


if __name__ == "__main__":
    main()
