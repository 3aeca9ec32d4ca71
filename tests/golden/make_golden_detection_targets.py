#!/usr/bin/env python3
"""Regenerates tests/golden/detection_targets.npz from the reference's own model.mrn_samples.

    python tests/golden/make_golden_detection_targets.py      (reference tree: $MASKRCNN_REFERENCE, as for make_golden.py)

Loads the reference through make_golden.load_reference() (its model.py / data.py with its compiled CPU extension behind the
`maskrcnn` shim) and records what model.mrn_samples returns, image after image of every case, with GPU_COUNT = 0. For the call
  * torch.randperm is replaced by the key rule: torch.randperm(n) is not told its candidates, so torch.nonzero is wrapped to
    remember its last [n,1] result `cand`, and randperm returns lexsort((cand, keys[cand])) — the candidates with the smallest
    (key, roi index) come first, in that order;
  * data.boxes_deltas is wrapped to record the positive RoIs and their matched boxes.
roi_index comes from the recorded orders, gt_index from the reference's boxes_overlaps + torch.max(dim=1) on the chosen RoIs; the
generator asserts that the reference's own rois, class ids and matched boxes are the rows those indices name, that no IoU is NaN,
and that the reference raised wherever status is 1 (an image without a kept row; the fixture then holds what the library
defines: all slots empty).

DATA only; ground-truth masks are NOT stored: tests/detection_targets_cases.py builds them from the boxes for the generator and
the tests alike, and the keys come from hash_keys. Per case i (names[i], counts[i], ratios[i], mask_shapes[i], mask_kinds[i],
mask_hws[i], key_modes[i], seeds[i]):
    c<i>_rois float32 [B,N,4], c<i>_boxes float32 [M,4], c<i>_ids int32 [M], c<i>_off int32 [B+1],
    c<i>_status / _num_pos / _num_neg int32 [B], c<i>_roi_index / _gt_index int16 [B,count] (-1: empty slot; gt_index -1 for a
    negative), c<i>_class_ids int32 [B,count], c<i>_deltas float32 [B,count,4],
    c<i>_mask_bits: np.packbits of the positives' mask targets [sum num_pos, mh, mw] where they are 0 / 1, else c<i>_mask_bytes uint8.
"""
import importlib.util
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import detection_targets_cases as dtc  # noqa: E402

STD_DEV = [0.1, 0.1, 0.2, 0.2]
f32 = lambda v: np.asarray(v, np.float32).reshape(-1, 4)
i32 = lambda v: np.asarray(v, np.int32).reshape(-1)


def random_gt(rng, g, lo=0.12, hi=0.5):
    y1, x1 = rng.uniform(0, 0.8, g), rng.uniform(0, 0.8, g)
    h, w = rng.uniform(lo, hi, g), rng.uniform(lo, hi, g)
    return np.stack([y1, x1, np.minimum(y1 + h, 1.0), np.minimum(x1 + w, 1.0)], 1).astype(np.float32)


def jittered(rng, boxes, n, jitter=0.08):
    """n RoIs around rows of `boxes`, corners moved by up to `jitter` of the side: most reach IoU 0.5."""
    pick = boxes[rng.integers(0, len(boxes), n)].astype(np.float64)
    h, w = pick[:, 2] - pick[:, 0], pick[:, 3] - pick[:, 1]
    d = rng.uniform(-jitter, jitter, (n, 4)) * np.stack([h, w, h, w], 1)
    return (pick + d).astype(np.float32)


def rois_for(rng, boxes, n, near, zeros=0, jitter=0.08, clip=True):
    r = np.concatenate([jittered(rng, boxes, near, jitter), random_gt(rng, n - near - zeros, 0.05, 0.4), np.zeros((zeros, 4), np.float32)])
    r[:n - zeros] = r[rng.permutation(n - zeros)]
    return np.clip(r, 0, 1) if clip else r


def cases():
    """[dict(name, rois [B,N,4], images [(boxes, ids)], count, ratio, mask_shape, mask_kind, mask_hw, key_mode, seed)]"""
    rng = np.random.default_rng(20261020)
    out = []

    def add(name, rois, images, count=100, ratio=0.33, mask_shape=(28, 28), mask_kind="mixed", mask_hw=(32, 40), key_mode=0):
        out.append(dict(name=name, rois=np.stack([np.asarray(r, np.float32) for r in rois]), images=images, count=count, ratio=ratio,
                        mask_shape=mask_shape, mask_kind=mask_kind, mask_hw=mask_hw, key_mode=key_mode, seed=31 + len(out)))

    # the basic batch: fewer positives than the limit, negatives cut by neg_limit
    gts = [(random_gt(rng, 4), i32([3, 1, 7, 80])), (random_gt(rng, 3), i32([5, 5, 9])), (random_gt(rng, 1), i32([2]))]
    basic = [rois_for(rng, b, 64, 12) for b, _ in gts]
    add("basic_b3", basic, gts)
    add("basic_b3_count8", basic, gts, count=8)
    add("basic_b3_count8_equal_keys", basic, gts, count=8, key_mode=1)
    add("basic_b3_count8_mod4_keys", basic, gts, count=8, key_mode=2)
    add("basic_b3_mask1x1", basic, gts, mask_shape=(1, 1))
    add("basic_b3_ramp", basic, gts, mask_kind="ramp")
    add("basic_b3_mask8x8", basic, gts, mask_hw=(8, 8), mask_kind="rect")
    # sizes
    one = random_gt(rng, 1)
    add("n1", [jittered(rng, one, 1, 0.02), f32([0.0, 0.0, 0.05, 0.05])], [(one, i32([4])), (f32([0.5, 0.5, 0.9, 0.9]), i32([6]))])
    for n in (63, 65):
        g = random_gt(rng, 5)
        add(f"n{n}", [rois_for(rng, g, n, 20)], [(g, rng.integers(1, 81, 5).astype(np.int32))])
    g = random_gt(rng, 50)
    add("n4096_rows50", [rois_for(rng, g, 4096, 600)], [(g, rng.integers(1, 81, 50).astype(np.int32))])
    g = random_gt(rng, 1024)
    add("rows1024_n64", [rois_for(rng, g, 64, 24, jitter=0.04)], [(g, rng.integers(1, 81, 1024).astype(np.int32))], mask_kind="rect")
    # both limits reached: 33 + 67 (the num_pos = 33 -> 67 entry), 25 + 75, 50 + 50
    g = random_gt(rng, 6)
    both = [rois_for(rng, g, 200, 90, jitter=0.05)]
    for ratio in (0.33, 0.25, 0.5):
        add(f"both_limits_ratio{ratio}", both, [(g, i32([1, 2, 3, 4, 5, 6]))], ratio=ratio)
    # no positive although negatives exist; only positives
    add("no_positives", [f32([[0, 0, 0.1, 0.1], [0.05, 0.05, 0.2, 0.3], [0, 0.5, 0.2, 0.9]])], [(f32([0.6, 0.6, 0.9, 0.9]), i32([3]))])
    g = random_gt(rng, 2, 0.3, 0.5)
    add("only_positives", [jittered(rng, g, 16, 0.02)], [(g, i32([8, 9]))])
    # thresholds: IoU exactly 0.5 is positive, one ulp narrower is negative
    add("thresholds", [f32([[0, 0, 1, 0.5], [0, 0, 1, np.nextafter(np.float32(0.5), np.float32(0))]])], [(f32([0, 0, 1, 1]), i32([7]))])
    # duplicate rows with different ids: the first wins
    g = random_gt(rng, 2)
    add("row_ties", [rois_for(rng, g, 32, 16)], [(np.concatenate([g[:1], g[:1], g[1:], g[1:]]), i32([11, 12, 13, 14]))])
    # crowds: crowd row + id-0 row (dropped) + kept rows, with RoIs inside the crowd; an id-0 row without a crowd (kept: class-0
    # positives); an all-crowd image between two good ones
    k3, k2 = random_gt(rng, 3), random_gt(rng, 2)
    crowd_a = (np.concatenate([f32([0.0, 0.0, 0.45, 0.45]), f32([0.5, 0.5, 0.8, 0.8]), k3]), i32([-1, 0, 4, 4, 6]))
    crowd_b = (np.concatenate([f32([0.1, 0.1, 0.5, 0.6]), k2]), i32([0, 2, 6]))
    rois_a = np.concatenate([rois_for(rng, crowd_a[0][1:], 40, 20), f32([[0.05, 0.05, 0.2, 0.2], [0.1, 0.2, 0.4, 0.44], [0.0, 0.0, 0.45, 0.45]]),
                             rois_for(rng, k3, 5, 0)])
    rois_b = rois_for(rng, crowd_b[0], 48, 24)
    add("crowds", [rois_a, rois_b], [crowd_a, crowd_b])
    add("all_crowd_between", [rois_a, rois_b, rois_b], [crowd_b, (random_gt(rng, 2), i32([-1, -3])), crowd_b])
    # zero-padded RoIs are ordinary RoIs: sampled as negatives
    g = random_gt(rng, 3)
    add("zero_padded", [rois_for(rng, g, 32, 10, zeros=5, jitter=0.03)], [(g, i32([1, 2, 3]))])
    # masks: RoIs reaching outside [0, 1] (extrapolation 0)
    g = f32([[0.0, 0.0, 0.4, 0.5], [0.55, 0.5, 1.0, 1.0], [0.2, 0.6, 0.7, 1.0]])
    outside = [rois_for(rng, g, 48, 30, jitter=0.1, clip=False)]
    add("masks_outside", outside, [(g, i32([1, 2, 3]))])
    add("masks_outside_14x28", outside, [(g, i32([1, 2, 3]))], mask_shape=(14, 28), mask_kind="ellipse")
    # taps exactly midway between pixels of a 9 x 17 mask: rows 2.5, 4.5 and columns 1.5, 3.5, 5.5
    mid = f32([0.3125, 0.09375, 0.5625, 0.34375])
    far = f32([0.8, 0.8, 0.95, 0.95])
    add("midpoints_u8", [np.concatenate([mid, far])], [(mid, i32([5]))], mask_shape=(2, 3), mask_kind="edge01", mask_hw=(9, 17))
    add("midpoints_f32", [np.concatenate([mid, far]), np.concatenate([far, mid])], [(mid, i32([5])), (mid, i32([4]))],
        mask_shape=(2, 3), mask_kind="steps135", mask_hw=(9, 17))
    # one full-size image with 2 rows
    g = f32([[0.1, 0.2, 0.6, 0.7], [0.5, 0.05, 0.95, 0.5]])
    add("mask1024", [rois_for(rng, g, 24, 12)], [(g, i32([17, 18]))], mask_hw=(1024, 1024), mask_kind="mixed")
    return out


def one_image(rmodel, rdata, rois, boxes, ids, masks, c, keys):
    """The reference's outputs for one image, as the library lays them out."""
    count, (mh, mw) = c["count"], c["mask_shape"]
    cfg = types.SimpleNamespace(GPU_COUNT=0, TRAIN_ROIS_PER_IMAGE=count, ROI_POSITIVE_RATIO=c["ratio"], BBOX_STD_DEV=STD_DEV,
                                MASK_SHAPE=[mh, mw])
    crowd = np.where(ids < 0)[0]
    kept = np.where(ids > 0)[0] if crowd.size else np.arange(ids.size)
    res = dict(status=0, num_pos=0, num_neg=0, roi_index=np.full(count, -1, np.int32), gt_index=np.full(count, -1, np.int32),
               class_ids=np.zeros(count, np.int32), deltas=np.zeros((count, 4), np.float32), masks=np.zeros((0, mh, mw), np.float32))
    args = (torch.from_numpy(rois)[None], torch.from_numpy(ids)[None], torch.from_numpy(boxes)[None], torch.from_numpy(masks)[None], cfg)
    log = dict(last=None, orders=[], deltas=[])
    real_nonzero, real_randperm, real_deltas = torch.nonzero, torch.randperm, rdata.boxes_deltas

    def nonzero(x, *a, **k):
        r = real_nonzero(x, *a, **k)
        if r.dim() == 2 and r.size(1) == 1:
            log["last"] = r[:, 0].numpy().copy()
        return r

    def randperm(n, *a, **k):
        cand = log["last"]
        assert cand is not None and len(cand) == n
        perm = np.lexsort((cand, keys[cand]))
        log["orders"].append(cand[perm])
        return torch.from_numpy(perm)

    def boxes_deltas(b, g):
        log["deltas"].append((b.numpy().copy(), g.numpy().copy()))
        return real_deltas(b, g)

    torch.nonzero, torch.randperm, rdata.boxes_deltas = nonzero, randperm, boxes_deltas
    try:
        if kept.size == 0:
            try:
                rmodel.mrn_samples(*args)
            except Exception:
                res["status"] = 1
                return res
            raise AssertionError("the reference accepted an image without a kept row")
        r_rois, r_ids, r_deltas, r_masks = rmodel.mrn_samples(*args)
    finally:
        torch.nonzero, torch.randperm, rdata.boxes_deltas = real_nonzero, real_randperm, real_deltas
    n = r_rois.size(0) if r_rois.dim() == 2 else 0
    if n == 0:
        return res
    pos_rois, pos_boxes = log["deltas"][0]
    p = len(pos_rois)
    q = n - p
    assert p >= 1 and n <= count and len(log["deltas"]) == 1 and len(log["orders"]) >= (2 if q else 1)
    idx = np.concatenate([log["orders"][0][:p], log["orders"][1][:q] if q else np.zeros(0, np.int64)]).astype(np.int32)
    bits = lambda v: np.ascontiguousarray(v, np.float32).view(np.uint32)
    assert np.array_equal(bits(r_rois.numpy()), bits(rois[idx])), "the reference's rois are not rois[roi_index]"
    ov = rdata.boxes_overlaps(torch.from_numpy(rois[idx[:p]]), torch.from_numpy(boxes[kept]))
    assert not torch.isnan(rdata.boxes_overlaps(torch.from_numpy(rois), torch.from_numpy(boxes))).any(), "NaN IoU"
    gt = kept[torch.max(ov, dim=1)[1].numpy()].astype(np.int32)
    assert np.array_equal(bits(pos_boxes), bits(boxes[gt])) and np.array_equal(bits(pos_rois), bits(rois[idx[:p]]))
    assert np.array_equal(r_ids.numpy()[:p], ids[gt]) and not r_ids.numpy()[p:].any() and r_ids.dtype == torch.int32
    assert r_deltas.dtype == torch.float32 and not r_deltas.numpy()[p:].any() and not r_masks.numpy()[p:].any()
    assert tuple(r_masks.shape) == (n, mh, mw) and r_masks.dtype == torch.float32
    res.update(num_pos=p, num_neg=q, masks=r_masks.numpy()[:p].copy())
    res["roi_index"][:n] = idx
    res["gt_index"][:p] = gt
    res["class_ids"][:n] = r_ids.numpy()
    res["deltas"][:n] = r_deltas.numpy()
    return res


def main():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    refc, rconfig, rutils, rdata, rmodel = mg.load_reference()
    assert rconfig.Config.BBOX_STD_DEV == STD_DEV and rconfig.Config.TRAIN_ROIS_PER_IMAGE == 100
    assert rconfig.Config.ROI_POSITIVE_RATIO == 0.33 and rconfig.Config.MASK_SHAPE == [28, 28]
    assert torch.max(torch.tensor([[.5, .5, .2]]), dim=1)[1].item() == 0            # the first maximum
    assert [int(1.0 / 0.33 * p - p) for p in (0, 1, 2, 31, 32, 33)] == [0, 2, 4, 62, 64, 67]
    arrays, meta = {}, {k: [] for k in ("names", "counts", "ratios", "mask_shapes", "mask_kinds", "mask_hws", "key_modes", "seeds")}
    for i, c in enumerate(cases()):
        images = c["images"]
        boxes = np.concatenate([b for b, _ in images]).astype(np.float32)
        ids = np.concatenate([k for _, k in images]).astype(np.int32)
        off = np.concatenate([[0], np.cumsum([len(k) for _, k in images])]).astype(np.int32)
        masks = dtc.build_masks(c["mask_kind"], boxes, *c["mask_hw"])
        n = c["rois"].shape[1]
        res = [one_image(rmodel, rdata, c["rois"][k], boxes[s:e], ids[s:e], masks[s:e], c, dtc.hash_keys(c["seed"], k, n, c["key_mode"]))
               for k, (s, e) in enumerate(zip(off[:-1], off[1:]))]
        for k, v in (("names", c["name"]), ("counts", c["count"]), ("ratios", c["ratio"]), ("mask_shapes", c["mask_shape"]),
                     ("mask_kinds", c["mask_kind"]), ("mask_hws", c["mask_hw"]), ("key_modes", c["key_mode"]), ("seeds", c["seed"])):
            meta[k].append(v)
        p = f"c{i}_"
        arrays[p + "rois"], arrays[p + "boxes"], arrays[p + "ids"], arrays[p + "off"] = c["rois"], boxes, ids, off
        for k in ("status", "num_pos", "num_neg"):
            arrays[p + k] = np.array([r[k] for r in res], np.int32)
        for k, dt in (("roi_index", np.int16), ("gt_index", np.int16), ("class_ids", np.int32), ("deltas", np.float32)):
            arrays[p + k] = np.stack([r[k] for r in res]).astype(dt)
        pos_masks = np.concatenate([r["masks"] for r in res])
        assert np.array_equal(pos_masks, np.round(pos_masks)) and pos_masks.min(initial=0) >= 0 and pos_masks.max(initial=0) <= 255
        if pos_masks.max(initial=0) <= 1:
            arrays[p + "mask_bits"] = np.packbits(pos_masks.astype(np.uint8).ravel())
        else:
            arrays[p + "mask_bytes"] = pos_masks.astype(np.uint8).ravel()
        print(f"{c['name']}: N={n} G={[len(k) for _, k in images]} count={c['count']} ratio={c['ratio']}: "
              f"+{[r['num_pos'] for r in res]} -{[r['num_neg'] for r in res]} status={[r['status'] for r in res]} "
              f"mask values {sorted(set(np.unique(pos_masks).tolist()))}")
    path = os.path.join(HERE, "detection_targets.npz")
    np.savez_compressed(path, names=np.array(meta["names"]), counts=np.array(meta["counts"], np.int32),
                        ratios=np.array(meta["ratios"], np.float64), mask_shapes=np.array(meta["mask_shapes"], np.int32),
                        mask_kinds=np.array(meta["mask_kinds"]), mask_hws=np.array(meta["mask_hws"], np.int32),
                        key_modes=np.array(meta["key_modes"], np.int32), seeds=np.array(meta["seeds"], np.int32),
                        numpy_version=np.array(np.__version__), torch_version=np.array(torch.__version__), **arrays)
    print(f"{path}: {len(meta['names'])} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
