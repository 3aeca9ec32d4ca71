#!/usr/bin/env python3
"""Regenerates tests/golden/ground_truth.npz from the reference's own dataset code: CocoMaskRCNNDataset.load, encode_image,
encode_masks and encode_boxes of <reference>/data.py, imported UNMODIFIED and driven on a small synthetic in-memory data set.

    python tests/golden/make_golden_ground_truth.py     (reference tree: $MASKRCNN_REFERENCE, as for make_golden_cocoeval.py)

What is supplied around data.py (helpers of make_golden_cocoeval.py / make_golden_poly.py are imported, not edited):
  * placeholders for skimage and torchvision, as in make_golden.py, with transforms.Resize((h, w)) = img.resize((w, h),
    Image.BILINEAR) and transforms.Pad = ImageOps.expand (what torchvision does for a PIL image and a zero fill), and a
    CocoDetection base whose __getitem__ returns (a blank PIL image of the image's size, the image's annotations) from a COCO
    object — the reference's own pycocotools/coco.py, unmodified, on the data set written to a temporary file;
  * <reference>/cocoapi/common/maskApi.c compiled into a temporary directory OUTSIDE this repository behind a stub
    pycocotools._mask (frPyObjects, merge, decode), and np.float = float;
  * random.randint pinned per case (load() draws its flip from it).
The dataset object is made without CocoMaskRCNNDataset.__init__ (which wants the COCO directory layout and the anchors): its
attributes coco, ids, root and config are set here.

Stored, DATA only (nothing of the reference's text):
    gt_json                  the synthetic data set: images (sizes), annotations (polygons, compressed strings, count lists,
                             iscrowd, category ids), categories (the ids CocoLabel.from_class knows)
    from_class   int64 [91]  CocoLabel.from_class(c) for c = 0 .. 90, -1 where it raises KeyError
    case_min_dim, case_max_dim int64 [C]; case_image_ids int64 and case_flips uint8, concatenated, case_off int64 [C+1]
  and per (case, image), T in all, in case order:
    exp_count int64 [T]; exp_labels int32 (concatenated); exp_boxes uint32 [M,4]: the float32 boxes' bit patterns;
    exp_scale float64 [T]; exp_window int64 [T,4]; exp_mask_shape int64 [T,2]: the reference's mask extent (new_h + 2*top,
    new_w + 2*left; h, w for scale == 1); exp_masks uint8: np.packbits of every image's [count, H, W] 0 / 1 masks, concatenated,
    exp_mask_off int64 [T+1]
"""
import contextlib
import ctypes
import io
import json
import os
import random
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_cocoeval as mg  # noqa: E402
import make_golden_poly as mp  # noqa: E402


def stub_mask_module(dll, codec):
    """pycocotools._mask's frPyObjects (_mask.pyx:288-308), merge (:160-168) and decode (:145-158) on the compiled codec."""
    dll.rleDecode.argtypes = [ctypes.POINTER(mg.RLE), ctypes.c_void_p, ctypes.c_ulong]
    dll.rleDecode.restype = None
    stub = types.ModuleType("pycocotools._mask")

    def fr_py_objects(obj, h, w):
        if type(obj) == list and len(obj[0]) > 4:
            return [codec.from_counts([int(v) for v in mp.ref_poly(dll, np.asarray(p[:2 * int(len(p) / 2)], np.float64), h, w)], h, w)
                    for p in obj]
        if type(obj) == dict and "counts" in obj and "size" in obj:
            return codec.from_counts([int(v) for v in obj["counts"]], h, w)
        raise Exception("input type is not supported.")

    def merge(rles, intersect=0):
        h, w = rles[0]["size"]
        return codec.from_counts([int(v) for v in mp.ref_merge(dll, [codec.counts(r) for r in rles], h, w, intersect)], h, w)

    def decode(rles):
        h, w = rles[0]["size"]
        out = np.zeros((h, w, len(rles)), dtype=np.uint8, order="F")
        rs = codec.structs(rles)
        dll.rleDecode(rs, out.ctypes.data, len(rles))
        codec.free(rs)
        return out

    stub.frPyObjects, stub.merge, stub.decode = fr_py_objects, merge, decode
    stub.iou = stub.area = stub.toBbox = stub.encode = None
    sys.modules["pycocotools._mask"] = stub


def load_reference(reference):
    from PIL import Image, ImageOps

    def placeholder(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class CocoDetection:                               # torchvision.datasets.CocoDetection.__getitem__, without the files
        def __getitem__(self, index):
            img_id = self.ids[index]
            info = self.coco.loadImgs(img_id)[0]
            return Image.new("RGB", (info["width"], info["height"])), self.coco.loadAnns(self.coco.getAnnIds(imgIds=img_id))

    class Resize:
        def __init__(self, size):
            self.size = size

        def __call__(self, img):
            return img.resize((self.size[1], self.size[0]), Image.BILINEAR)

    class Pad:
        def __init__(self, padding):
            self.padding = padding

        def __call__(self, img):
            return ImageOps.expand(img, border=tuple(self.padding), fill=0)

    sk = placeholder("skimage")
    sk.io, sk.color = placeholder("skimage.io"), placeholder("skimage.color")
    sk.measure = placeholder("skimage.measure", find_contours=None)
    sk.transform = placeholder("skimage.transform")
    tv = placeholder("torchvision")
    tv.datasets = placeholder("torchvision.datasets", CocoDetection=CocoDetection)
    tv.transforms = placeholder("torchvision.transforms", Resize=Resize, Pad=Pad)
    import scipy
    if not hasattr(scipy, "misc"):
        scipy.misc = placeholder("scipy.misc")
    if not hasattr(np, "float"):
        np.float = float
    sys.path.insert(0, reference)
    sys.path.insert(0, os.path.join(reference, "cocoapi", "PythonAPI"))
    try:
        import data as rdata
        from pycocotools.coco import COCO
    finally:
        del sys.path[:2]
    return rdata, COCO


# ------------------------------------------------------------------------------------------------ the data set
# image id -> (h, w). 48 / 64: enlarging by 1.6 with even pads (30x40), odd left / top pads (30x37, 37x30), shrinking by 1.5 (96x72)
# and by 4 (256x200), scale == 1 (50x60), one pixel wide / high (40x1, 1x40). 100 / 130: 60x80 (x1.625), 77x91 (x1.2987, even pad),
# 101x75 (x1.287, odd left pad), 130x100 (scale == 1 at the canvas's own height), 300x410 (shrinking by 3.15).
SMALL = {11: (30, 40), 12: (30, 37), 13: (37, 30), 14: (96, 72), 15: (256, 200), 16: (50, 60), 17: (40, 1), 18: (1, 40), 19: (30, 40)}
LARGE = {21: (60, 80), 22: (77, 91), 23: (101, 75), 24: (130, 100), 25: (300, 410)}


def dataset(codec, categories):
    rng = np.random.default_rng(20260115)
    images, anns = [], []
    ann_id = [500]
    cats = [c for c in categories if c]

    def add(img, cat, seg, crowd=0):
        ann_id[0] += int(rng.integers(1, 5))
        anns.append({"id": ann_id[0], "image_id": img, "category_id": int(cat), "segmentation": seg, "iscrowd": crowd})

    def rle(mask, as_list=False):
        r = codec.encode(mask)
        return {"size": r["size"], "counts": codec.counts(r)} if as_list else r

    def poly(h, w):
        k = int(rng.integers(3, 8))
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        cy, cx, r = rng.uniform(0.3 * h, 0.7 * h), rng.uniform(0.3 * w, 0.7 * w), rng.uniform(0.2, 0.6) * max(min(h, w), 3)
        pts = np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1)
        return [float(v) for v in np.round(pts, 2).reshape(-1)]

    for img, (h, w) in {**SMALL, **LARGE}.items():
        images.append({"id": img, "height": h, "width": w, "file_name": f"synthetic_{img}.png"})
        if img == 19:                                                         # nothing kept: the fake row
            add(img, 0, rle(mg.rect(h, w, 2, 2, 9, 9)))                       # category 0
            add(img, cats[3], rle(np.zeros((h, w), bool)))                    # an empty mask
            continue
        if min(h, w) == 1:
            line = np.zeros((h, w), bool)
            line.reshape(-1)[3:17] = True
            add(img, cats[1], rle(line))
            add(img, cats[2], rle(np.ones((h, w), bool), as_list=True))
            add(img, cats[4], rle(line[::-1, ::-1].copy()), crowd=1)
            continue
        add(img, cats[int(rng.integers(0, 80))], [poly(h, w)])                                          # a polygon
        add(img, cats[int(rng.integers(0, 80))], [poly(h, w), poly(h, w), [1.0, 1.0, 6.5, 1.0, 3.0, 7.25]])    # three parts
        add(img, cats[int(rng.integers(0, 80))], rle(mg.blob(h, w, 0.4 * h, 0.6 * w, 0.3 * min(h, w), rng)))   # a compressed string
        add(img, cats[int(rng.integers(0, 80))], rle(mg.ellipse(h, w, 0.6 * h, 0.3 * w, 0.25 * h, 0.2 * w), as_list=True))   # a count list
        add(img, 0, rle(mg.rect(h, w, 1, 1, h // 2, w // 2)))                                           # category 0: skipped
        edges = mg.rect(h, w, 0, 0, h, w) & ~mg.rect(h, w, 2, 3, h - 3, w - 2)
        add(img, cats[int(rng.integers(0, 80))], rle(edges))                                            # touches all four edges
        add(img, cats[int(rng.integers(0, 80))], rle(np.zeros((h, w), bool), as_list=True))             # an empty mask: skipped
        add(img, cats[int(rng.integers(0, 80))], [[-9.0, -9.0, -5.0, -9.0, -7.0, -4.0]])                # a polygon off the image: empty
        crowd = mg.blob(h, w, 0.5 * h, 0.5 * w, 0.2 * min(h, w), rng) | mg.rect(h, w, h - 4, 0, h, 5)
        add(img, cats[int(rng.integers(0, 80))], rle(crowd), crowd=1)                                   # a crowd
        add(img, cats[int(rng.integers(0, 80))], rle(mg.ellipse(h + 3, w + 5, h / 2, w / 2, 6, 8)), crowd=1)   # a crowd of another size
        add(img, cats[int(rng.integers(0, 80))], rle(mg.rect(h, w, 0, w - 1, 1, w)))                    # one pixel, the top-right corner
    return {"images": images, "annotations": anns, "categories": [{"id": int(c), "name": f"cat{c}"} for c in cats]}


CASES = [(48, 64, list(SMALL), 0), (48, 64, list(SMALL), 1), (100, 130, list(LARGE), 0), (100, 130, list(LARGE), 1),
         (48, 64, [16, 11, 19], None)]           # a mixed batch: flips 1, 0, 1


def main():
    reference = os.environ.get("MASKRCNN_REFERENCE", "/root/reference")
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        dll = mp.bind(mg.load_codec(reference, tmp))
        codec = mg.Codec(dll)
        stub_mask_module(dll, codec)
        rdata, COCO = load_reference(reference)
        table = []
        for c in range(91):
            try:
                table.append(int(rdata.CocoLabel.from_class(c)))
            except KeyError:
                table.append(-1)
        gt = dataset(codec, [c for c in range(91) if table[c] >= 0])
        path = os.path.join(tmp, "gt.json")
        with open(path, "w") as fh:
            json.dump(gt, fh)
        ds = object.__new__(rdata.CocoMaskRCNNDataset)
        with contextlib.redirect_stdout(io.StringIO()):
            ds.coco = COCO(path)
        ds.root = "synthetic"
        out = {k: [] for k in ("count", "labels", "boxes", "scale", "window", "mask_shape", "masks")}
        ids_all, flips_all, case_off = [], [], [0]
        for min_dim, max_dim, image_ids, flip in CASES:
            ds.config = types.SimpleNamespace(IMAGE_MIN_DIM=min_dim, IMAGE_MAX_DIM=max_dim, MAX_GT_INSTANCES=100)
            ds.ids = list(image_ids)
            flips = [flip] * len(image_ids) if flip is not None else [1, 0, 1]
            for index, f in enumerate(flips):
                real = random.randint
                rdata.random.randint = lambda a, b, f=f: f
                try:
                    with contextlib.redirect_stdout(io.StringIO()):
                        image, label_ids, _, boxes, masks = ds.load(index, hflip=True)
                finally:
                    rdata.random.randint = real
                image, scale, cropbox = rdata.encode_image(image, min_dim, max_dim)
                masks = rdata.encode_masks(masks, scale, cropbox)
                boxes = rdata.encode_boxes(boxes, scale, cropbox)
                m = np.asarray(masks.numpy())
                assert set(np.unique(m).tolist()) <= {0, 1} and boxes.dtype == torch.float32 and m.shape[0] == len(label_ids)
                win = [int(cropbox.top()), int(cropbox.left()), int(cropbox.bottom()), int(cropbox.right())]
                assert m.shape[1:] == ((image.height, image.width) if scale == 1 else (win[2] + win[0], win[3] + win[1]))
                out["count"].append(len(label_ids))
                out["labels"].append(np.asarray(label_ids.numpy(), np.int32))
                out["boxes"].append(np.ascontiguousarray(boxes.numpy(), np.float32).view(np.uint32).reshape(-1, 4))
                out["scale"].append(float(scale))
                out["window"].append(win)
                out["mask_shape"].append(m.shape[1:])
                out["masks"].append(np.packbits(m.astype(np.uint8).reshape(-1)))
            ids_all += list(image_ids)
            flips_all += flips
            case_off.append(len(ids_all))
    data = {
        "gt_json": np.array(json.dumps(gt)), "from_class": np.array(table, np.int64),
        "case_min_dim": np.array([c[0] for c in CASES], np.int64), "case_max_dim": np.array([c[1] for c in CASES], np.int64),
        "case_image_ids": np.array(ids_all, np.int64), "case_flips": np.array(flips_all, np.uint8), "case_off": np.array(case_off, np.int64),
        "exp_count": np.array(out["count"], np.int64), "exp_labels": np.concatenate(out["labels"]),
        "exp_boxes": np.concatenate(out["boxes"]), "exp_scale": np.array(out["scale"], np.float64),
        "exp_window": np.array(out["window"], np.int64), "exp_mask_shape": np.array(out["mask_shape"], np.int64),
        "exp_masks": np.concatenate(out["masks"]),
        "exp_mask_off": np.concatenate([[0], np.cumsum([m.size for m in out["masks"]])]).astype(np.int64),
    }
    path = os.path.join(HERE, "ground_truth.npz")
    np.savez_compressed(path, **data)
    print(f"{path}: {len(gt['images'])} images, {len(gt['annotations'])} annotations, {len(ids_all)} (case, image) pairs, "
          f"{int(sum(out['count']))} rows, {os.path.getsize(path)} bytes")
    print("rows per image", out["count"], "scales", np.round(out["scale"], 4).tolist())


if __name__ == "__main__":
    main()
