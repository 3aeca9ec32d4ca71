"""The cases of tests/golden/targets.npz (made by tests/golden/make_golden_targets.py from the reference's data.rpn_samples), as
dense arrays, for test_targets_host.py and test_gpu_targets.py. Loaded once; nothing here is modified by a test."""
import functools

import numpy as np
import torch

from conftest import load_golden

PYRAMIDS = {"pyr64": (64, (8, 16, 32), (4, 8, 16)), "pyr128": (128, (8, 16, 32, 64, 128), (4, 8, 16, 32, 64)),
            "full": (1024, (32, 64, 128, 256, 512), (4, 8, 16, 32, 64))}


def hash_keys(seed: int, b: int, a: int, mode: int) -> np.ndarray:
    """The generator's formula: int32 [a], non-negative. mode 0: a multiplicative hash of the anchor index; 1: all equal; 2: the
    hash modulo 4."""
    h = ((np.arange(a, dtype=np.uint64) + np.uint64(1)) * np.uint64(2654435761) + np.uint64((seed + 977 * b) * 40503)) & np.uint64(0xffffffff)
    k = (h >> np.uint64(1)).astype(np.int64)
    if mode == 1:
        k[:] = 7
    elif mode == 2:
        k = (k >> 8) % 4
    return k.astype(np.int32)


def pyramid_config(name):
    from maskrcnn_amd.config import InferenceConfig
    side, scales, strides = PYRAMIDS[name]
    return InferenceConfig(image_height=side, image_width=side, backbone_strides=strides, rpn_anchor_scales=scales)


@functools.lru_cache(maxsize=None)
def anchor_set(name) -> np.ndarray:
    """float64 [A,4]: the reference's, from the fixture; the full-size set from anchors.py (the generator asserted equality)."""
    if name == "full":
        from maskrcnn_amd import anchors
        return anchors.pyramid_anchors(pyramid_config("full"), dtype=torch.float64).numpy()
    return load_golden("targets")["anchors_" + name]


@functools.lru_cache(maxsize=None)
def cases():
    z = load_golden("targets")
    out = []
    for i, name in enumerate(z["names"].tolist()):
        p = f"c{i}_"
        aset = str(z["sets"][i])
        anchors = anchor_set(aset)
        a, off = anchors.shape[0], z[p + "off"]
        b = len(off) - 1
        c = dict(name=name, set=aset, anchors=anchors, count=int(z["counts"][i]), boxes=z[p + "boxes"], ids=z[p + "ids"], off=off,
                 status=z[p + "status"], gt_argmax=z[p + "gt_argmax"], npos_all=z[p + "npos_all"], bbox_all=z[p + "bbox_all"],
                 bbox=z[p + "bbox"], batch=b, sparse=(p + "u_idx") in z.files,
                 keys=np.stack([hash_keys(int(z["seeds"][i]), k, a, int(z["key_modes"][i])) for k in range(b)]))
        if c["sparse"]:
            idx = z[p + "u_idx"].astype(np.int64)
            match_u, argmax, iou = np.full(b * a, -1, np.int32), None, None
            match_u[idx] = z[p + "u_val"]
            c.update(match_u=match_u.reshape(b, a), u_idx=idx, u_argmax=z[p + "u_argmax"].astype(np.int32), u_iou=z[p + "u_iou"])
            match = np.zeros(b * a, np.int32)
            match[z[p + "s_idx"].astype(np.int64)] = z[p + "s_val"]
            c["match"] = match.reshape(b, a)
        else:
            c.update(match_u=z[p + "match_u"].astype(np.int32), argmax=z[p + "argmax"].astype(np.int32), iou_max=z[p + "iou_max"],
                     match=z[p + "match"].astype(np.int32))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(c)
    return tuple(out)


def names(usable_only: bool = False):
    """Case names straight from the fixture (cheap: for parametrising at collection time)."""
    z = load_golden("targets")
    return [n for i, n in enumerate(z["names"].tolist()) if not (usable_only and z[f"c{i}_status"].any())]


def case(name):
    return next(c for c in cases() if c["name"] == name)


def images(c):
    """[(boxes [G,4], ids [G]), ...] of a case."""
    return [(c["boxes"][s:e], c["ids"][s:e]) for s, e in zip(c["off"][:-1], c["off"][1:])]


def usable(c) -> bool:
    """Every image has a kept row (rpn_targets takes the case)."""
    return not c["status"].any()


def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """|a - b| in fp32 units in the last place, for finite values of the same sign pattern (ordered-integer distance)."""
    ia, ib = a.astype(np.float32).view(np.int32).astype(np.int64), b.astype(np.float32).view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


@functools.lru_cache(maxsize=None)
def shared_geometry():
    """One geometry for BOTH matchers (csrc/target_match.hpp is their common rule): 100 boxes, every coordinate a multiple of 1/8
    in [0, 64], so the float64 anchors narrow exactly to the float32 RoIs; 2 images. Image 0: five rows — an ordinary one, a crowd,
    an id-0 row (dropped beside the crowd), another ordinary one and a duplicate of row 0 (an exact IoU tie for every box: row 0
    wins). Image 1: one row. Box 0 overlaps no row, boxes 1-6 are the rows themselves (IoU 1), box 7 overlaps rows 0 and 3 alike (IoU
    0.2 with each), the others are rows moved and resized by up to 2.5, or anywhere. → dict(boxes float64 [100,4], gt float32 [6,4], ids, off, keys)."""
    gt = np.array([[8, 8, 24, 24], [32, 32, 56, 56], [8, 40, 24, 56], [40, 8, 56, 24], [8, 8, 24, 24], [16, 16, 48, 48]], np.float32)
    ids = np.array([3, -1, 0, 5, 7, 2], np.int32)
    rng = np.random.default_rng(20261019)
    near = gt[rng.integers(0, 6, 62)] + rng.integers(-20, 21, (62, 4)) / 8.0
    y1, x1 = rng.integers(0, 8 * 48, 30) / 8.0, rng.integers(0, 8 * 48, 30) / 8.0
    far = np.stack([y1, x1, y1 + rng.integers(8, 8 * 16, 30) / 8.0, x1 + rng.integers(8, 8 * 16, 30) / 8.0], 1)
    boxes = np.concatenate([[[60, 60, 64, 64]], gt, [[16, 8, 48, 24]], near, far]).astype(np.float64)
    assert boxes.shape == (100, 4) and (boxes >= 0).all() and (boxes <= 64).all() and np.array_equal(boxes * 8, np.round(boxes * 8))
    assert (boxes[:, 2] > boxes[:, 0]).all() and (boxes[:, 3] > boxes[:, 1]).all()
    out = dict(boxes=boxes, gt=gt, ids=ids, off=np.array([0, 5, 6], np.int32), keys=np.stack([hash_keys(11, b, 100, 0) for b in range(2)]))
    for v in out.values():
        v.setflags(write=False)
    return out
