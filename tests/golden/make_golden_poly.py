#!/usr/bin/env python3
"""Regenerates tests/golden/poly.npz from the reference's own codec: rleFrPoly, rleFrBbox and rleMerge.

    python tests/golden/make_golden_poly.py     (reference tree: $MASKRCNN_REFERENCE, as for make_golden_cocoeval.py)

As make_golden_cocoeval.py (whose helpers are imported, not edited): <reference>/cocoapi/common/maskApi.c is compiled into a
temporary directory OUTSIDE this repository and called through ctypes, and <reference>/.../pycocotools/cocoeval.py is imported
unmodified with a stand-in COCO class — whose annToRLE here does what pycocotools/coco.py:406-425 does for polygons:
frPyObjects (rleFrPoly per part) and merge (rleMerge).

Stored, DATA only:
  cases     case_names [C]; case_xy float64 [V,2] with case_off int64 [C+1] (vertices of case c: case_xy[case_off[c]:case_off[c+1]]);
            case_h, case_w int32 [C]; case_cnt uint32 with case_cnt_off int64 [C+1]: rleFrPoly's run lengths;
            case_fma bool [C]: a restatement of steps 1-2 with a fused multiply-add differs from the reference on this case
  groups    group_names [G]; group_members int64 with group_off int64 [G+1] (indices into the cases); group_union /
            group_inter uint32 with group_union_off / group_inter_off: rleMerge's run lengths, intersect = 0 / 1
  boxes     box_bb float64 [B,4] (x, y, w, h); box_h, box_w; box_cnt with box_cnt_off: rleFrBbox's run lengths
  evaluation set: the synthetic data set of cocoeval.npz with every non-crowd ground truth as 1-4 polygon parts
            gt_json, results_json; ann_ids int64 [P] (the polygon annotations, data set order) with ann_cnt / ann_cnt_off: annToRLE's
            run lengths; and segm_* as in cocoeval.npz (IoU matrices, evalImgs, precision, recall, scores, stats, summary)
"""
import ctypes
import json
import os
import sys
import tempfile
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_cocoeval as mg  # noqa: E402

RLE = mg.RLE


def bind(dll):
    P, UL = ctypes.POINTER, ctypes.c_ulong
    dll.rleFrPoly.argtypes = [P(RLE), ctypes.c_void_p, UL, UL, UL]
    dll.rleFrPoly.restype = None
    dll.rleFrBbox.argtypes = [P(RLE), ctypes.c_void_p, UL, UL, UL]
    dll.rleFrBbox.restype = None
    dll.rleMerge.argtypes = [P(RLE), P(RLE), UL, ctypes.c_int]
    dll.rleMerge.restype = None
    return dll


def take(dll, r) -> np.ndarray:
    out = np.array([r.cnts[i] for i in range(r.m)], dtype=np.uint32)
    dll.rleFree(ctypes.byref(r))
    return out


def ref_poly(dll, xy, h, w) -> np.ndarray:
    xy = np.ascontiguousarray(np.asarray(xy, dtype=np.float64).reshape(-1, 2))
    r = RLE()
    dll.rleFrPoly(ctypes.byref(r), xy.ctypes.data, xy.shape[0], h, w)
    return take(dll, r)


def ref_bbox(dll, bb, h, w) -> np.ndarray:
    bb = np.ascontiguousarray(np.asarray(bb, dtype=np.float64).reshape(4))
    r = RLE()
    dll.rleFrBbox(ctypes.byref(r), bb.ctypes.data, h, w, 1)
    return take(dll, r)


def ref_merge(dll, rows, h, w, intersect) -> np.ndarray:
    rs = (RLE * len(rows))()
    for r, c in zip(rs, rows):
        arr = (ctypes.c_uint * len(c))(*[int(v) for v in c])
        dll.rleInit(ctypes.byref(r), h, w, len(c), arr)
    m = RLE()
    dll.rleMerge(rs, ctypes.byref(m), len(rows), intersect)
    for r in rs:
        dll.rleFree(ctypes.byref(r))
    return take(dll, m)


# ------------------------------------------------------------------------------------------------ the restatement (FMA search)
# The parity formulation of rleFrPoly in numpy, as tests/test_poly_host.py has it; fma=True evaluates 5*x + .5 and ys + s*t as one
# fused multiply-add (exact rational arithmetic, rounded once) wherever that can change the integer the value is cast to.
def _fma(a, b, c) -> float:
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _grid(c, fma):
    t = 5.0 * c + .5
    if fma:
        for i in np.nonzero(np.abs(t - np.rint(t)) < 1e-6 * np.maximum(1.0, np.abs(t)))[0]:
            t[i] = _fma(5.0, c[i], .5)
    return np.trunc(t).astype(np.int64)


def _minor(a0, s, t, fma):
    r = float(a0) + s * t.astype(np.float64)
    if fma:
        for i in np.nonzero(np.abs((r + .5) - np.rint(r + .5)) < 1e-6 * np.maximum(1.0, np.abs(r)))[0]:
            r[i] = _fma(s, float(t[i]), float(a0))
    return np.trunc(r + .5).astype(np.int64)


def poly_keys(xy, h, w, fma=False):
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    X, Y = _grid(xy[:, 0].copy(), fma), _grid(xy[:, 1].copy(), fma)
    k, us, vs = len(X), [], []
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
            vs.append(np.full(1, -2 ** 31, np.int64) if dx == 0 else _minor(ys, float(ye - ys) / float(dx), t, fma))
        else:
            t = dy - d if flip else d
            vs.append(t + ys)
            us.append(_minor(xs, float(xe - xs) / float(dy), t, fma))
    u, v = np.concatenate(us), np.concatenate(vs)
    j = np.nonzero(u[1:] != u[:-1])[0] + 1
    xd = (np.where(u[j] < u[j - 1], u[j], u[j] - 1).astype(np.float64) + .5) / 5.0 - .5
    keep = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    yd = np.ceil(np.clip((np.minimum(v[j], v[j - 1]).astype(np.float64) + .5) / 5.0 - .5, 0, h))
    return xd[keep].astype(np.int64) * h + yd[keep].astype(np.int64)


def fr_poly_restated(xy, h, w, fma=False) -> np.ndarray:
    keys = poly_keys(xy, h, w, fma)
    vals, cnt = np.unique(keys[keys < h * w], return_counts=True)
    return np.diff(np.concatenate([[0], vals[cnt % 2 == 1], [h * w]])).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ the cases
def star(cx, cy, r_out, r_in, points=5, phase=-np.pi / 2):
    a = phase + np.arange(2 * points) * np.pi / points
    r = np.where(np.arange(2 * points) % 2 == 0, r_out, r_in)
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1)


def pentagram(cx, cy, r):
    a = -np.pi / 2 + np.arange(5) * 4 * np.pi / 5            # every second corner: the edges cross
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1)


def serpentine(bands=32, pitch=16, half=4.0, x0=4.3, x1=507.6):
    """A snake of `bands` horizontal bands joined at alternating ends: 4 * bands vertices, two long horizontal edges per band."""
    c = []
    for i in range(bands):
        y = pitch * i + 8.2
        c += [(x0, y), (x1, y)] if i % 2 == 0 else [(x1, y), (x0, y)]
    c = np.array(c)
    d = np.sign(np.diff(c, axis=0))
    nrm = np.stack([-d[:, 1], d[:, 0]], 1)
    off = np.concatenate([nrm[:1], nrm[:-1] + nrm[1:], nrm[-1:]]) * half
    return np.concatenate([c + off, (c - off)[::-1]])


def random_poly(rng, h, w):
    k = int(rng.integers(3, 41))
    kind = int(rng.integers(0, 5))
    cx, cy, r = rng.uniform(-0.1 * w, 1.1 * w), rng.uniform(-0.1 * h, 1.1 * h), rng.uniform(1, max(1.5, 0.6 * max(h, w)))
    a = np.sort(rng.uniform(0, 2 * np.pi, k)) if rng.uniform() < 0.8 else rng.uniform(0, 2 * np.pi, k)
    rr = r * rng.uniform(0.3, 1.0, k)
    xy = np.stack([cx + rr * np.cos(a), cy + rr * np.sin(a)], 1)
    if kind == 0:
        xy = np.round(xy)
    elif kind == 1:
        xy = np.round(xy * 2) / 2
    elif kind == 2:
        xy = np.round(xy, 1)
    elif kind == 3:
        xy = np.round(xy, 2)
    if rng.uniform() < 0.1:
        i = int(rng.integers(0, k))
        xy[(i + 1) % k] = xy[i]                               # a repeated vertex
    return xy


def build_cases(dll):
    cases = []                                                # (name, xy, h, w)
    add = lambda name, xy, h, w: cases.append((name, np.asarray(xy, dtype=np.float64).reshape(-1, 2), int(h), int(w)))
    # trivial images
    add("img1x1_cover", [-1, -1, 3, -1, 3, 3, -1, 3], 1, 1)
    add("img1x1_miss", [2, 2, 5, 2, 5, 5], 1, 1)
    add("h1", [2, -1, 9, -1, 9, 2, 2, 2], 1, 12)
    add("w1", [-1, 3, 2, 3, 2, 9, -1, 9], 12, 1)
    # basic shapes on integer, half-integer and fractional coordinates
    for tag, sh in (("int", 0.0), ("half", 0.5), ("frac", 0.37)):
        add(f"triangle_{tag}", np.array([[5, 4], [30, 10], [12, 28]]) + sh, 33, 37)
        add(f"rect_{tag}", np.array([[6, 5], [25, 5], [25, 20], [6, 20]]) + sh, 33, 37)
    # outside the image
    h, w = 30, 40
    add("out_left", [-30, 5, -10, 5, -10, 20, -30, 20], h, w)
    add("out_right", [50, 5, 70, 5, 70, 20, 50, 20], h, w)
    add("out_top", [5, -30, 20, -30, 20, -10, 5, -10], h, w)
    add("out_bottom", [5, 40, 20, 40, 20, 60, 5, 60], h, w)
    add("over_left", [-10, 8, 12, 8, 12, 20, -10, 20], h, w)
    add("over_right", [30, 8, 55, 8, 55, 20, 30, 20], h, w)
    add("over_top", [8, -9, 20, -9, 20, 12, 8, 12], h, w)
    add("over_bottom", [8, 18, 20, 18, 20, 44, 8, 44], h, w)
    add("over_corner_tl", [-8, -8, 10, -3, 4, 12], h, w)
    add("over_corner_tr", [48, -8, 30, -3, 36, 12], h, w)
    add("over_corner_bl", [-8, 38, 10, 33, 4, 18], h, w)
    add("over_corner_br", [48, 38, 30, 33, 36, 18], h, w)
    # key aliases
    add("pixel0_on", [-2, -2, 6, -2, 6, 7, -2, 7], h, w)
    add("whole_image", [-5, -5, 60, -5, 60, 50, -5, 50], h, w)
    add("y_eq_h_last_column", [30, 20, 45, 20, 45, 45, 30, 45], h, w)     # bottom edge below the image, reaching the last column
    add("y_eq_h_inner_column", [10, 20, 25, 20, 25, 45, 10, 45], h, w)
    add("y_eq_h_slanted", [10.4, 33, 38.7, 31, 39.6, 36, 9, 39], h, w)     # wholly below: every crossing clamps to y == h
    # degenerate vertices
    add("k1", [7, 9], h, w)
    add("k2", [3, 4, 30, 22], h, w)
    add("repeat_first", [5, 5, 5, 5, 30, 8, 14, 25], h, w)
    add("repeat_middle", [5, 5, 30, 8, 30, 8, 14, 25], h, w)
    add("repeat_closing", [5, 5, 30, 8, 14, 25, 5, 5], h, w)
    add("repeat_triple", [5.5, 5.5, 30, 8, 30, 8, 30, 8, 14, 25], h, w)
    add("collinear", [4, 4, 12, 4, 20, 4, 30, 4, 30, 14, 30, 24, 17, 24, 4, 24], h, w)
    # parity
    add("bowtie", [5, 5, 35, 25, 35, 5, 5, 25], h, w)
    add("star5", star(20, 15, 14, 5.5), h, w)
    add("pentagram", pentagram(20, 15, 14), h, w)
    add("spike", [5, 5, 30, 5, 30, 20, 38, 27, 30, 20, 5, 20], h, w)       # out and back along one edge
    add("spike_only", [6, 6, 33, 21, 6, 6, 33, 21], h, w)
    # slopes on integer coordinates
    for name, (dx, dy) in {"1_2": (2, 1), "3_2": (2, 3), "1_10": (10, 1), "7_10": (10, 7)}.items():
        add(f"slope_{name}", [3, 3, 3 + 2 * dx, 3 + 2 * dy, 3 + 2 * dx, 28, 3, 28], h, w)
        add(f"slope_inv_{name}", [3, 3, 3 + 2 * dy, 3 + 2 * dx, 36, 3 + 2 * dx, 36, 3], h, w)
    # the serpentine: far more keys than an on-chip sort holds
    snake = serpentine()
    add("serpentine", snake, 516, 512)
    assert snake.shape[0] == 128
    n_fixed = len(cases)
    # FMA-sensitive cases, searched
    rng = np.random.default_rng(20250712)
    found = 0
    for trial in range(50000):
        hh, ww = int(rng.integers(4, 60)), int(rng.integers(4, 60))
        xy = random_poly(rng, hh, ww)[: int(rng.integers(3, 9))]
        want = ref_poly(dll, xy, hh, ww)
        assert np.array_equal(fr_poly_restated(xy, hh, ww), want), ("restatement", trial)
        if not np.array_equal(fr_poly_restated(xy, hh, ww, fma=True), want):
            add(f"fma_{found}", xy, hh, ww)
            found += 1
            if found == 6:
                break
    assert found >= 4, f"only {found} FMA-sensitive cases in the search"
    n_fma = found
    # ordinary parts
    rng = np.random.default_rng(20250713)
    sizes = [(1, 1), (7, 5), (48, 64), (120, 160), (200, 150), (240, 320), (500, 650), (33, 257)]
    for i in range(300):
        hh, ww = sizes[int(rng.integers(1, len(sizes)))] if i >= 4 else sizes[i % 2]
        add(f"random_{i}", random_poly(rng, hh, ww), hh, ww)
    return cases, n_fixed, n_fma


def build_groups(cases):
    """Group members are extra cases on one 40 x 50 image; returns [(name, [case indices])]."""
    h, w = 40, 50
    idx = {}

    def add(name, xy):
        cases.append((f"g_{name}", np.asarray(xy, dtype=np.float64).reshape(-1, 2), h, w))
        idx[name] = len(cases) - 1

    rect = lambda x0, y0, x1, y1: [x0, y0, x1, y0, x1, y1, x0, y1]
    add("a", rect(4, 4, 14, 14))
    add("b", rect(20, 6, 32, 18))
    add("c", rect(36, 22, 47, 36))
    add("big", rect(2, 2, 46, 38))
    add("mid", rect(8, 8, 30, 30))
    add("small", rect(12, 12, 20, 20))
    add("empty", rect(60, 60, 70, 70))
    add("full", rect(-5, -5, 60, 60))
    add("corner0", rect(-3, -3, 5, 6))
    add("tri", [6, 30, 25, 12, 44, 33])
    add("star", star(25, 20, 17, 7))
    rng = np.random.default_rng(7)
    for i in range(12):
        cx, cy = rng.uniform(5, 45), rng.uniform(5, 35)
        add(f"r{i}", star(cx, cy, rng.uniform(4, 14), rng.uniform(2, 6), points=int(rng.integers(3, 7)), phase=rng.uniform(0, 6)))
    g = lambda name, *members: (name, [idx[m] for m in members])
    return [
        g("one", "star"), g("one_empty", "empty"), g("one_full", "full"),
        g("disjoint2", "a", "b"), g("disjoint3", "a", "b", "c"), g("nested3", "big", "mid", "small"),
        g("identical2", "tri", "tri"), g("identical3", "star", "star", "star"),
        g("with_empty", "tri", "empty"), g("with_empty3", "empty", "mid", "star"), g("with_full", "full", "star"),
        g("with_full3", "a", "full", "tri"), g("pixel0_union", "b", "corner0"), g("pixel0_both", "corner0", "full"),
        g("overlap2", "mid", "tri"), g("overlap3", "mid", "tri", "star"), g("empty_intersection", "a", "c", "star"),
        g("five", "a", "tri", "star", "mid", "corner0"), g("five_nested", "big", "mid", "small", "star", "tri"),
        g("twelve", *[f"r{i}" for i in range(12)]),
        g("twelve_mixed", "a", "b", "c", "big", "mid", "small", "tri", "star", "corner0", "r0", "r1", "empty"),
    ]


BOXES = [  # (x, y, w, h), image (h, w)
    ([4, 5, 10, 8], (30, 40)), ([4.5, 5.5, 10, 8], (30, 40)), ([4.3, 5.7, 10.2, 8.9], (30, 40)), ([0, 0, 40, 30], (30, 40)),
    ([10, 10, 0, 0], (30, 40)), ([10, 10, 0, 7], (30, 40)), ([10, 10, 7, 0], (30, 40)), ([-6, -4, 12, 11], (30, 40)),
    ([33, 22, 20, 20], (30, 40)), ([-10, 8, 70, 5], (30, 40)), ([0.2, 0.2, 0.5, 0.5], (1, 1)), ([100.25, 50.75, 33.5, 80.125], (200, 150)),
]


# ------------------------------------------------------------------------------------------------ the evaluation set
def polygon_dataset(codec):
    """dataset() of make_golden_cocoeval.py with every non-crowd ground truth as 1-4 polygon parts inside its box (area, bbox and
    everything else as there; crowds stay RLE, as count lists)."""
    gt, results = mg.dataset(codec)
    rng = np.random.default_rng(20250714)
    for n, ann in enumerate(gt["annotations"]):
        if ann["iscrowd"]:
            rle = ann["segmentation"]
            if isinstance(rle["counts"], str):
                ann["segmentation"] = {"size": rle["size"], "counts": codec.counts(rle)}
            continue
        x, y, bw, bh = ann["bbox"]
        parts = []
        for part in range(1 + n % 4):
            k = int(rng.integers(3, 25))
            a = np.sort(rng.uniform(0, 2 * np.pi, k))
            s = 1.0 if part == 0 else rng.uniform(0.15, 0.4)
            cx, cy = (x + bw / 2, y + bh / 2) if part == 0 else (x + rng.uniform(0, bw), y + rng.uniform(0, bh))
            rr = rng.uniform(0.75, 1.0, k)
            px, py = cx + s * rr * (bw / 2 + 0.5) * np.cos(a), cy + s * rr * (bh / 2 + 0.5) * np.sin(a)
            p = np.round(np.stack([px, py], 1).reshape(-1), [0, 1, 2, 2][n % 4])
            flat = [float(v) for v in p]
            if part == 2:
                flat = flat[:4]                               # a later part with 4 numbers: a 2-vertex polygon
            if part == 3:
                flat = flat + [flat[0]]                       # an odd trailing number: dropped (len // 2)
            parts.append(flat)
        ann["segmentation"] = parts
    return gt, results


def main():
    reference = os.environ.get("MASKRCNN_REFERENCE", "/root/reference")
    with tempfile.TemporaryDirectory() as tmp:
        dll = bind(mg.load_codec(reference, tmp))
        codec = mg.Codec(dll)
        cases, n_fixed, n_fma = build_cases(dll)
        groups = build_groups(cases)
        counts = [ref_poly(dll, xy, h, w) for _, xy, h, w in cases]
        names = [c[0] for c in cases]
        assert counts[names.index("serpentine")].size > 8192, counts[names.index("serpentine")].size
        assert counts[names.index("whole_image")].tolist() == [0, 30 * 40] and counts[names.index("pixel0_on")][0] == 0
        for (name, xy, h, w), c in zip(cases, counts):        # the parity formulation equals the reference on every case
            assert int(c.astype(np.int64).sum()) == h * w and np.array_equal(fr_poly_restated(xy, h, w), c), name
        cat = lambda rows, dtype: np.concatenate([np.asarray(r, dtype=dtype).reshape(-1) for r in rows] + [np.zeros(0, dtype)])
        offs = lambda rows: np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        data = {
            "case_names": np.array(names), "case_xy": np.concatenate([c[1] for c in cases]), "case_off": offs([c[1] for c in cases]),
            "case_h": np.array([c[2] for c in cases], np.int32), "case_w": np.array([c[3] for c in cases], np.int32),
            "case_cnt": cat(counts, np.uint32), "case_cnt_off": offs(counts),
            "case_fma": np.array([n.startswith("fma_") for n in names]),
        }
        uni = [ref_merge(dll, [counts[m] for m in mem], 40, 50, 0) for _, mem in groups]
        inter = [ref_merge(dll, [counts[m] for m in mem], 40, 50, 1) for _, mem in groups]
        data.update({"group_names": np.array([g[0] for g in groups]), "group_members": cat([g[1] for g in groups], np.int64),
                     "group_off": offs([g[1] for g in groups]), "group_union": cat(uni, np.uint32), "group_union_off": offs(uni),
                     "group_inter": cat(inter, np.uint32), "group_inter_off": offs(inter)})
        bcnt = [ref_bbox(dll, bb, h, w) for bb, (h, w) in BOXES]
        data.update({"box_bb": np.array([b[0] for b in BOXES], np.float64), "box_h": np.array([b[1][0] for b in BOXES], np.int32),
                     "box_w": np.array([b[1][1] for b in BOXES], np.int32), "box_cnt": cat(bcnt, np.uint32), "box_cnt_off": offs(bcnt)})

        # the evaluation set, through the reference's unmodified cocoeval.py
        cocoeval = mg.import_cocoeval(reference, codec)
        gt, results = polygon_dataset(codec)
        ann_cnt = {}

        def string_of(cnts, h, w):
            return codec.from_counts([int(v) for v in cnts], h, w)

        class PolyCoco(mg.Coco):
            def annToRLE(self, ann):                          # pycocotools/coco.py:406-425
                t = self.imgs[ann["image_id"]]
                h, w, segm = t["height"], t["width"], ann["segmentation"]
                if type(segm) == list:
                    assert len(segm[0]) > 4                   # frPyObjects' dispatch: polygons
                    parts = [ref_poly(dll, np.asarray(p[:2 * int(len(p) / 2)], np.float64), h, w) for p in segm]
                    merged = ref_merge(dll, parts, h, w, 0)
                    ann_cnt[ann["id"]] = merged
                    return string_of(merged, h, w)
                if type(segm["counts"]) == list:
                    return self.codec.from_counts(segm["counts"], h, w)
                return segm

        real_coco, mg.Coco = mg.Coco, PolyCoco                # run() builds mg.Coco; loadRes returns one too
        try:
            data.update(mg.run(cocoeval, codec, gt, results, "segm"))
        finally:
            mg.Coco = real_coco
        poly_ids = [a["id"] for a in gt["annotations"] if isinstance(a["segmentation"], list)]
        assert sorted(ann_cnt) == sorted(poly_ids) and len(poly_ids) > 40
        data.update({"gt_json": np.array(json.dumps(gt)), "results_json": np.array(json.dumps(results)),
                     "ann_ids": np.array(poly_ids, np.int64), "ann_cnt": cat([ann_cnt[i] for i in poly_ids], np.uint32),
                     "ann_cnt_off": offs([ann_cnt[i] for i in poly_ids])})
    path = os.path.join(HERE, "poly.npz")
    np.savez_compressed(path, **data)
    print(f"{path}: {len(cases)} cases ({n_fixed} fixed, {n_fma} FMA-sensitive), {len(groups)} groups, {len(BOXES)} boxes, "
          f"{len(poly_ids)} polygon annotations, {os.path.getsize(path)} bytes")
    print("serpentine runs", counts[names.index("serpentine")].size, "stats", np.round(data["segm_stats"], 3).tolist())


if __name__ == "__main__":
    main()
