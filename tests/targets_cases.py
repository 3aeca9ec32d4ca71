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
