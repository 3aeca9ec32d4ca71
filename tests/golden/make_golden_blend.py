#!/usr/bin/env python3
"""Regenerates tests/golden/blend.npz from the reference's own renderer.

    python tests/golden/make_golden_blend.py        (reference tree: $MASKRCNN_REFERENCE, as for make_golden.py)

Imports <reference>/data.py (third-party modules this image lacks replaced by empty placeholders, as make_golden.py does) and
calls its blend_image(image, None, boxes, masks) and random_colors under random.seed(k) with Pillow, exactly as predict.py
there does; the one case with prescribed colours chains its blend_mask(image, mask, colour). Stores DATA only:
    names                       case names
    shapes    int32 [K,3]       (N, H, W)
    seeds     int32 [K]         random.seed(k) before random_colors(N) / blend_image; -1: the colours were prescribed
    images    uint8             the [H,W,3] inputs, concatenated;                      img_off  int64 [K+1]
    masks     uint8             np.packbits of the [N,H,W] 0 / 1 masks, concatenated;  mask_off int64 [K+1]
    boxes     float64 [sum N,4] (y1, x1, y2, x2), as handed to the reference;          box_off  int64 [K+1] (rows)
    colors    uint8 [sum N,3]   the palette the reference drew with (rows box_off)
    outputs   uint8             the rendered [H,W,3] images (offsets img_off)
    blend_table uint8 [256,256] Image.blend(pixel value p, colour value c, 0.2) at [p, c]
    pillow                      PIL.__version__
The kernel's tile is 256 x 16 pixels and a lane owns 16 pixels of a row: the seam case is cut to that.
"""
import os
import random
import sys
import types

import numpy as np

sys.dont_write_bytecode = True  # never drop __pycache__ into the reference tree
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MASKRCNN_REFERENCE", "/root/reference")

import torch  # noqa: E402


def load_reference_data():
    def placeholder(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    sk = placeholder("skimage")
    sk.io = placeholder("skimage.io")
    sk.color = placeholder("skimage.color")
    sk.measure = placeholder("skimage.measure", find_contours=None)
    tv = placeholder("torchvision")
    tv.datasets = placeholder("torchvision.datasets", CocoDetection=object)
    tv.transforms = placeholder("torchvision.transforms")
    import scipy
    if not hasattr(scipy, "misc"):
        scipy.misc = placeholder("scipy.misc")
    sys.path.insert(0, REF)
    import data as rdata
    return rdata


OUTSIDE = [-9.0, -9.0, -5.0, -5.0]      # a box no pixel of which is in the image


def ellipse(h, w, cy, cx, ry, rx):
    yy, xx = np.mgrid[:h, :w]
    return (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0).astype(np.uint8)


def noise(rng, h, w):
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    img.reshape(-1)[:2] = (0, 255)
    if img.size > 8:
        img.reshape(-1)[-2:] = (255, 0)
    return img


def points(h, w, pts):
    m = np.zeros((h, w), np.uint8)
    for y, x in pts:
        m[y, x] = 1
    return m


def cases():
    rng = np.random.default_rng(20251019)
    out = []   # (name, image, masks [N,H,W], boxes [N,4], seed)

    def add(name, image, masks, boxes, seed):
        masks = np.asarray(masks, np.uint8).reshape((-1,) + image.shape[:2])
        boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
        assert len(masks) == len(boxes), name
        out.append((name, image, masks, boxes, seed))

    add("n0_5x7", noise(rng, 5, 7), np.zeros((0, 5, 7)), np.zeros((0, 4)), 1)
    for h, w in ((1, 1), (2, 5), (5, 2), (3, 3), (17, 23)):
        img = noise(rng, h, w)
        add(f"full_{h}x{w}", img, [np.ones((h, w))], [[0, 0, h - 1, w - 1]], 2)          # the box equals the frame
        add(f"empty_{h}x{w}", img, [np.zeros((h, w))], [OUTSIDE], 3)
        add(f"random_{h}x{w}", img, rng.random((2, h, w)) < .4, [OUTSIDE, [0, 0, h // 2, w // 2]], 4)
    h, w = 17, 23
    img = noise(rng, h, w)
    for name, pts in (("corner", [(0, 0)]), ("corner_br", [(h - 1, w - 1)]), ("frame_top", [(0, 5)]), ("frame_left", [(6, 0)]),
                      ("next_to_frame", [(1, 1)]), ("next_to_frame_br", [(h - 2, w - 2)]), ("interior", [(8, 11)]),
                      ("diagonal", [(8, 11), (9, 12)]), ("antidiagonal", [(8, 11), (9, 10)])):
        add(f"pixel_{name}_17x23", img, [points(h, w, pts)], [OUTSIDE], 5)
    yy, xx = np.mgrid[:h, :w]
    add("checkerboard_17x23", img, [(yy + xx) % 2], [OUTSIDE], 6)
    add("checkerboard_odd_17x23", img, [(yy + xx + 1) % 2], [OUTSIDE], 6)
    # three overlapping instances: a later blend lands on an earlier outline and a later outline on an earlier blend
    three = [ellipse(h, w, 7, 8, 5, 6), ellipse(h, w, 9, 13, 5, 7), ellipse(h, w, 5, 11, 3.5, 9)]
    add("overlap3_17x23", img, three, [[2, 2, 12, 14], [4, 6, 14, 20], [1.5, 2.5, 8.5, 20.5]], 7)
    add("overlap3_reversed_17x23", img, three[::-1], [OUTSIDE] * 3, 8)
    # a width that is no multiple of 16, more than one lane run
    add("blobs_9x37", noise(rng, 9, 37), [ellipse(9, 37, 4, 16, 3, 6), ellipse(9, 37, 5, 33, 3.2, 5), rng.random((9, 37)) < .3],
        [[1, 10, 7, 22], [0, 30, 8, 36], OUTSIDE], 9)
    # larger than the 256 x 16 tile both ways: blobs across the tile seams (x = 256, 512; y = 16, 32) and the lane-run seams
    h, w = 40, 530
    seam = [ellipse(h, w, 16, 256, 6, 9), ellipse(h, w, 31.5, 511.5, 5, 7), ellipse(h, w, 8, 16, 5, 4), ellipse(h, w, 24, 271.5, 9, 3),
            ellipse(h, w, 20, 400, 19, 140), points(h, w, [(15, 255), (16, 256), (15, 257), (32, 511), (31, 512), (20, 15), (21, 16)]),
            rng.random((h, w)) < .08]
    add("seams_40x530", noise(rng, h, w), seam,
        [[10, 247, 22, 265], [26, 504, 37, 519], [3, 12, 13, 20], [15, 255, 16, 256], [1, 260, 39, 529], [15.9, 240.2, 32.1, 512.7],
         [-3, -3, 45, 600]], 10)
    # every pixel value under two colours, twice over
    grad = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (8, 256, 3)).copy()
    grad[4:] = 255 - grad[4:]
    gm = np.zeros((4, 8, 256), np.uint8)
    gm[0, 0:3] = 1; gm[1, 2:6] = 1; gm[2, 1:7, 40:200] = 1; gm[3, :, 100:256] = 1
    out.append(("gradient_8x256", grad, gm, np.array([OUTSIDE] * 4, np.float64),
                np.array([(0, 127, 255), (255, 0, 128), (255, 0, 128), (0, 127, 255)], np.uint8)))
    # boxes: no masks to speak of
    h, w = 17, 23
    img = noise(rng, h, w)
    kinds = [("inside", [3, 4, 10, 15]), ("cross_top", [-4, 4, 6, 12]), ("cross_left", [3, -5, 9, 7]), ("cross_bottom", [9, 3, 25, 11]),
             ("cross_right", [2, 15, 8, 40]), ("outside", OUTSIDE), ("outside_right", [2, 30, 8, 40]), ("outside_below", [20, 2, 28, 9]),
             ("flat", [6, 3, 6, 14]), ("flat_last_row", [16, 3, 16, 14]), ("flat_above", [-1, 3, -1, 14]), ("thin", [3, 9, 12, 9]),
             ("point", [7, 7, 7, 7]), ("point_corner", [16, 22, 16, 22]), ("frame", [0, 0, 16, 22]), ("beyond_frame", [-1, -1, 17, 23]),
             ("fractional", [2.7, 3.2, 9.9, 12.5]), ("negative_fractional", [-0.5, -0.9, 5.5, 6.5]),
             ("negative_fractional_flat", [-0.9, 2.2, -0.2, 8.8]), ("two_rows", [4, 5, 5, 16])]
    for name, b in kinds:
        add(f"box_{name}_17x23", img, [np.zeros((h, w))], [b], 11)
    add("box_order_17x23", img, np.zeros((3, h, w)), [[2, 2, 10, 12], [5, 6, 14, 18], [2, 6, 10, 18]], 12)
    add("box_all_17x23", img, np.zeros((len(kinds), h, w)), [b for _, b in kinds], 13)
    # 50 instances
    h, w = 24, 40
    p = rng.random((50, 6))
    many = [ellipse(h, w, p[i, 0] * h, p[i, 1] * w, 1 + 6 * p[i, 2], 1 + 9 * p[i, 3]) for i in range(50)]
    tl = np.stack([p[:, 0] * h - 8 * p[:, 4] - 1, p[:, 1] * w - 12 * p[:, 5] - 1], 1)
    add("n50_24x40", noise(rng, h, w), many, np.concatenate([tl, tl + 2 + 14 * rng.random((50, 2))], 1), 14)
    return out


def render(rdata, image, masks, boxes, seed):
    """→ (palette uint8 [N,3], output uint8 [H,W,3]) from the reference."""
    from PIL import Image
    pil = Image.fromarray(image.copy())
    if not isinstance(seed, int):                       # prescribed colours: blend_mask per instance, no boxes
        for m, c in zip(masks, seed):
            pil = rdata.blend_mask(pil, torch.from_numpy(m.copy()), tuple(int(v) for v in c))
        return np.asarray(seed, np.uint8), np.array(pil, dtype=np.uint8)
    n = len(boxes)
    random.seed(seed)
    palette = np.array(rdata.random_colors(n), dtype=np.uint8).reshape(-1, 3) if n else np.zeros((0, 3), np.uint8)
    random.seed(seed)
    got = rdata.blend_image(pil, None, torch.from_numpy(boxes.copy()), torch.from_numpy(masks.copy()))
    return palette, np.array(got, dtype=np.uint8)


def blend_table():
    from PIL import Image
    p = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None], (256, 256, 3)).copy()
    c = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (256, 256, 3)).copy()
    t = np.array(Image.blend(Image.fromarray(p), Image.fromarray(c), 0.2), dtype=np.uint8)
    assert (t[:, :, 0] == t[:, :, 1]).all() and (t[:, :, 0] == t[:, :, 2]).all()
    return t[:, :, 0].copy()


def main():
    import PIL
    rdata = load_reference_data()
    names, shapes, seeds, images, masks, boxes, colors, outputs = [], [], [], [], [], [], [], []
    for name, image, m, b, seed in cases():
        palette, got = render(rdata, image, m, b, seed)
        assert got.shape == image.shape and palette.shape == (len(b), 3), name
        names.append(name); shapes.append((len(b),) + image.shape[:2]); seeds.append(seed if isinstance(seed, int) else -1)
        images.append(image.reshape(-1)); masks.append(np.packbits(m.reshape(-1))); boxes.append(b); colors.append(palette)
        outputs.append(got.reshape(-1))
    off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    path = os.path.join(HERE, "blend.npz")
    np.savez_compressed(path, names=np.array(names), shapes=np.array(shapes, np.int32), seeds=np.array(seeds, np.int32),
                        images=np.concatenate(images), img_off=off(images), masks=np.concatenate(masks), mask_off=off(masks),
                        boxes=np.concatenate(boxes), box_off=off(boxes), colors=np.concatenate(colors),
                        outputs=np.concatenate(outputs), blend_table=blend_table(), pillow=np.array(PIL.__version__))
    print(f"{path}: {len(names)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
