"""The cases of tests/golden/detection_targets.npz (made by tests/golden/make_golden_detection_targets.py from the reference's own
model.mrn_samples), for test_detection_targets_host.py and test_gpu_detection_targets.py, and the masks of those cases for the
generator and the tests alike: the fixture stores boxes and expected targets, never a ground-truth mask. Loaded once; nothing here
is modified by a test."""
import functools

import numpy as np

from conftest import load_golden
from targets_cases import hash_keys, ulp_distance  # noqa: F401  (re-exported for the tests)

STD_DEV = (0.1, 0.1, 0.2, 0.2)


def build_masks(kind: str, boxes: np.ndarray, height: int, width: int) -> np.ndarray:
    """[G,H,W] masks for the rows `boxes` (float32 [G,4], normalised (y1, x1, y2, x2): pixel (y, x) sits at (y / (H-1), x / (W-1))).
      rect     uint8: 1 inside the box.                    ellipse  uint8: 1 inside the box's inscribed ellipse.
      mixed    uint8: rect for even rows, ellipse for odd. bool     rect as numpy bool.
      ramp     float32: a grey ramp inside the box, 0 at its top-left corner to 1 at its bottom-right one; 0 outside.
      edge01   uint8: 1 where y >= 3, whatever the box (a tap midway between rows 2 and 3 reads 0.5).
      steps135 float32 of values 1 / 3 / 5, whatever the box: even rows 1 + 2 [y >= 3 and x >= 2] (a tap at (2.5, 1.5) reads
               1.5), odd rows 3 - 2 [y < 3 and x < 2] + 2 [y >= 5 and x >= 4] (2.5 at (2.5, 1.5), 3.5 at (4.5, 3.5))."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    ys = (np.arange(height, dtype=np.float64) / max(height - 1, 1))[:, None]
    xs = (np.arange(width, dtype=np.float64) / max(width - 1, 1))[None, :]
    yi, xi = np.arange(height)[:, None], np.arange(width)[None, :]
    out = np.zeros((len(boxes), height, width), np.float32 if kind in ("ramp", "steps135") else np.uint8)
    for g, (y1, x1, y2, x2) in enumerate(boxes.astype(np.float64)):
        rect = (ys >= y1) & (ys <= y2) & (xs >= x1) & (xs <= x2)
        cy, cx, ry, rx = (y1 + y2) / 2, (x1 + x2) / 2, max((y2 - y1) / 2, 1e-9), max((x2 - x1) / 2, 1e-9)
        ellipse = ((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1.0
        if kind in ("rect", "bool"):
            out[g] = rect
        elif kind == "ellipse":
            out[g] = ellipse
        elif kind == "mixed":
            out[g] = ellipse if g % 2 else rect
        elif kind == "ramp":
            t = ((ys - y1) / max(y2 - y1, 1e-9) + (xs - x1) / max(x2 - x1, 1e-9)) / 2
            out[g] = np.where(rect, t, 0.0).astype(np.float32)
        elif kind == "edge01":
            out[g] = np.broadcast_to(yi >= 3, (height, width))
        elif kind == "steps135":
            if g % 2 == 0:
                out[g] = 1 + 2 * ((yi >= 3) & (xi >= 2))
            else:
                out[g] = 3 - 2 * ((yi < 3) & (xi < 2)) + 2 * ((yi >= 5) & (xi >= 4))
        else:
            raise ValueError(kind)
    return out.astype(bool) if kind == "bool" else out


def case_masks(c) -> np.ndarray:
    """[M,H,W] for a case (a dict with mask_kind, boxes, mask_hw)."""
    return build_masks(c["mask_kind"], c["boxes"], int(c["mask_hw"][0]), int(c["mask_hw"][1]))


def case_keys(c) -> np.ndarray:
    """int32 [B,N]."""
    return np.stack([hash_keys(c["seed"], k, c["rois"].shape[1], c["key_mode"]) for k in range(c["batch"])])


@functools.lru_cache(maxsize=None)
def cases():
    z = load_golden("detection_targets")
    out = []
    for i, name in enumerate(z["names"].tolist()):
        p = f"c{i}_"
        off, count = z[p + "off"], int(z["counts"][i])
        mh, mw = (int(v) for v in z["mask_shapes"][i])
        b = len(off) - 1
        num_pos = z[p + "num_pos"]
        c = dict(name=name, batch=b, count=count, ratio=float(z["ratios"][i]), mask_shape=(mh, mw), mask_kind=str(z["mask_kinds"][i]),
                 mask_hw=tuple(int(v) for v in z["mask_hws"][i]), key_mode=int(z["key_modes"][i]), seed=int(z["seeds"][i]),
                 rois=z[p + "rois"], boxes=z[p + "boxes"], ids=z[p + "ids"], off=off, status=z[p + "status"], num_pos=num_pos,
                 num_neg=z[p + "num_neg"], roi_index=z[p + "roi_index"].astype(np.int32), gt_index=z[p + "gt_index"].astype(np.int32),
                 class_ids=z[p + "class_ids"].astype(np.int32), deltas=z[p + "deltas"])
        # the positives' mask targets, image after image: bits where the fixture holds 0 / 1 only, bytes otherwise
        total = int(num_pos.sum())
        if (p + "mask_bits") in z.files:
            flat = np.unpackbits(z[p + "mask_bits"])[:total * mh * mw]
        else:
            flat = z[p + "mask_bytes"]
        pos_masks = flat.reshape(total, mh, mw).astype(np.float32)
        mask = np.zeros((b, count, mh, mw), np.float32)
        at = 0
        for k in range(b):
            mask[k, :num_pos[k]] = pos_masks[at:at + num_pos[k]]
            at += int(num_pos[k])
        c["target_mask"] = mask
        rois_out = np.zeros((b, count, 4), np.float32)
        for k in range(b):
            n = int(num_pos[k] + c["num_neg"][k])
            rois_out[k, :n] = c["rois"][k][c["roi_index"][k, :n]]      # the generator asserted the reference's bits
        c["rois_out"] = rois_out
        c["keys"] = case_keys(c)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(c)
    return tuple(out)


def names(usable_only: bool = False):
    """Case names straight from the fixture (cheap: for parametrising at collection time)."""
    z = load_golden("detection_targets")
    return [n for i, n in enumerate(z["names"].tolist()) if not (usable_only and z[f"c{i}_status"].any())]


def case(name):
    return next(c for c in cases() if c["name"] == name)


def images(c):
    """[(boxes [G,4], ids [G]), ...] of a case."""
    return [(c["boxes"][s:e], c["ids"][s:e]) for s, e in zip(c["off"][:-1], c["off"][1:])]


def usable(c) -> bool:
    """Every image has a kept row (the front end takes the case)."""
    return not c["status"].any()


EXPECTED = ("rois_out", "class_ids", "deltas", "roi_index", "gt_index", "num_pos", "num_neg", "status", "target_mask")


def compare(c, got: dict, exact_log: bool = False):
    """Asserts the issue's bars for one case: every integer output, rois_out, dy, dx and every mask target bit for bit; dh / dw
    within 2 fp32 ulps (torch's fp32 CPU log may be one ulp from the correctly rounded value, and one correctly rounded division
    by std_dev can carry that to two). `got`: name -> array, the names of EXPECTED. → (values of dh / dw that differ at all, the
    largest distance in ulps)."""
    for k in ("class_ids", "roi_index", "gt_index", "num_pos", "num_neg", "status"):
        np.testing.assert_array_equal(np.asarray(got[k]).astype(np.int64), c[k].astype(np.int64), err_msg=f"{c['name']}: {k}")
    for k in ("rois_out", "target_mask"):
        a, e = np.ascontiguousarray(got[k], np.float32), np.ascontiguousarray(c[k], np.float32)
        assert a.shape == e.shape and np.array_equal(a.view(np.uint32), e.view(np.uint32)), f"{c['name']}: {k} differs"
    a, e = np.ascontiguousarray(got["deltas"], np.float32), c["deltas"]
    assert a.shape == e.shape
    assert np.array_equal(a[..., :2].copy().view(np.uint32), e[..., :2].copy().view(np.uint32)), f"{c['name']}: dy / dx differ"
    d = ulp_distance(a[..., 2:], e[..., 2:])
    differing, worst = int((d != 0).sum()), int(d.max()) if d.size else 0
    print(f"{c['name']}: dh / dw values differing from the fixture: {differing} of {d.size}, largest distance {worst} ulp")
    assert worst <= (0 if exact_log else 2), f"{c['name']}: dh / dw {worst} ulps from the fixture"
    return differing, worst
