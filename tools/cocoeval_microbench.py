#!/usr/bin/env python3
"""Times the COCO evaluation kernels and maskrcnn_amd.cocoeval.evaluate. Recorded, not asserted: there is no earlier
implementation here to regress against, and the reference's C codec is not available where the GPU is.

    python tools/cocoeval_microbench.py [--out profiles/cocoeval_microbench.jsonl] [--reps 9] [--images 500]

  (a) 100 x 30 blob masks at 1200 x 1920 (the case of tests/test_gpu_cocoeval.py), one group:
      ops.rle_iou (grouped form) and ops.coco_match, HIP events around each call after a warm-up; their sum per repetition
  (b) the same arithmetic by the numpy restatement of tests/test_cocoeval_host.py (rle_iou_ref + evaluate_img_ref for the four
      area ranges), wall clock, same process, same inputs — labelled "numpy_restatement": it is this repository's own test
      oracle, NOT the reference's C / Cython code
  (c) cocoeval.evaluate(iou_type="segm" and "bbox") on a seeded synthetic data set of --images images of 240 x 320 (about 7 ground
      truths and 9 detections each, four categories, RLE made by ops.rle_encode): wall clock of the whole call (host grouping,
      table building, the two grouped launches, accumulate, summarize), and inside it the device time of the two calls
  (d) the restatement's IoU + matching on (c)'s groups, wall clock, labelled as in (b)
One JSON line per measurement (median, min, max over the repetitions, in ms). Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def blob_masks(torch, n, h, w, seed, rmin, rmax):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: (torch.rand(n, generator=g) * (hi - lo) + lo).to(dev).view(n, 1, 1)
    cy, cx, r, p1, p2 = u(0.1 * h, 0.9 * h), u(0.1 * w, 0.9 * w), u(rmin, rmax), u(0, 6), u(0, 6)
    k1, k2 = torch.randint(2, 5, (n,), generator=g).to(dev).view(n, 1, 1), torch.randint(5, 9, (n,), generator=g).to(dev).view(n, 1, 1)
    yy, xx = torch.arange(h, device=dev).view(1, h, 1).float(), torch.arange(w, device=dev).view(1, 1, w).float()
    out = torch.empty(n, h, w, dtype=torch.uint8, device=dev)
    for i in range(0, n, 8):
        s = slice(i, i + 8)
        ang = torch.atan2(yy - cy[s], xx - cx[s])
        rad = r[s] * (1 + 0.25 * torch.sin(k1[s] * ang + p1[s]) + 0.12 * torch.cos(k2[s] * ang + p2[s]))
        out[s] = torch.hypot(yy - cy[s], xx - cx[s]) <= rad
    return out


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def synthetic_dataset(torch, image, n_images, seed=11):
    """→ (COCO data set dict, result records): per image 7 blobs as ground truth (a crowd among them in one image of eight);
    the detections are copies of most of them plus 9 unrelated blobs; masks are encoded by ops.rle_encode."""
    import numpy as np
    rng = np.random.default_rng(seed)
    h, w, cats = 240, 320, [1, 2, 3, 4]
    images, anns, results = [], [], []
    per = 16
    for i0 in range(0, n_images, 32):
        ids = list(range(i0 + 1, min(i0 + 32, n_images) + 1))
        masks = blob_masks(torch, per * len(ids), h, w, seed + i0, 5, 70)
        enc = image.rle_masks(masks)
        rles, areas, boxes = enc.to_coco(), enc.areas.cpu().numpy(), enc.bboxes.cpu().numpy()
        for j, img in enumerate(ids):
            images.append({"id": img, "height": h, "width": w})
            for k in range(per):
                m = j * per + k
                seg = {"size": rles[m]["size"], "counts": rles[m]["counts"].decode("ascii")}
                cat = cats[int(rng.integers(0, 4))]
                if k < 7:       # a ground truth, and four times in five a detection of it
                    anns.append({"id": len(anns) + 1, "image_id": img, "category_id": cat, "segmentation": seg,
                                 "iscrowd": int(k == 6 and img % 8 == 0), "area": float(areas[m]), "bbox": [float(v) for v in boxes[m]]})
                    if rng.uniform() < 0.8:
                        results.append({"image_id": img, "category_id": cat, "segmentation": seg, "bbox": [float(v) for v in boxes[m]],
                                        "score": float(np.round(rng.uniform(0.3, 1.0), 3))})
                else:           # an unrelated blob: a false positive unless it happens to overlap a ground truth enough
                    results.append({"image_id": img, "category_id": cat, "segmentation": seg, "bbox": [float(v) for v in boxes[m]],
                                    "score": float(np.round(rng.uniform(0.0, 0.7), 3))})
    return {"images": images, "annotations": anns, "categories": [{"id": c, "name": str(c)} for c in cats]}, results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cocoeval_microbench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--images", type=int, default=500)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cocoeval_microbench.py needs a GPU")
    from maskrcnn_amd import cocoeval, image, ops
    import test_cocoeval_host as ref
    dev = torch.device("cuda:0")
    rows = []
    to_dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(dev)

    # (a) one group of 100 x 30 at 1200 x 1920
    h, w = 1200, 1920
    dt, gt = image.rle_masks(blob_masks(torch, 100, h, w, 1, 60, 320)), image.rle_masks(blob_masks(torch, 30, h, w, 2, 80, 400))
    crowd = (np.arange(30) % 4 == 1).astype(np.uint8)
    offs = (to_dev([0, 100], np.int32), to_dev([0, 30], np.int32), to_dev([0, 3000], np.int64))
    areas = (dt.areas.double(), gt.areas.double(), to_dev(crowd, np.uint8), to_dev(ref.AREA_RNG, np.float64), to_dev(ref.IOU_THRS, np.float64))
    iou = lambda: ops.rle_iou(dt, gt, to_dev(crowd, np.uint8), *offs, out_len=3000)
    flat = iou()
    match = lambda: ops.coco_match(flat, *offs, *areas)
    match()
    torch.cuda.synchronize()
    t_iou, t_match = [], []
    for _ in range(args.reps):
        t_iou.append(event_ms(torch, iou)[0])
        t_match.append(event_ms(torch, match)[0])
    case = dict(case="100x30 blob masks at 1200x1920, one group", device=torch.cuda.get_device_name(0),
                dt_runs=int(dt.num_runs.sum()), gt_runs=int(gt.num_runs.sum()))
    rows.append(dict(case, what="ops.rle_iou (grouped), HIP events", **spread(t_iou)))
    rows.append(dict(case, what="ops.coco_match (4 area ranges x 10 thresholds), HIP events", **spread(t_match)))
    rows.append(dict(case, what="ops.rle_iou + ops.coco_match, HIP events", **spread([a + b for a, b in zip(t_iou, t_match)])))

    # (b) the numpy restatement on the same inputs
    nr, c = dt.num_runs.cpu().numpy(), dt.counts.cpu().numpy().view(np.uint32)
    rows_d = [c[i, :nr[i]] for i in range(len(nr))]
    nr, c = gt.num_runs.cpu().numpy(), gt.counts.cpu().numpy().view(np.uint32)
    rows_g = [c[i, :nr[i]] for i in range(len(nr))]
    ad, ag = dt.areas.double().cpu().numpy(), gt.areas.double().cpu().numpy()
    t_ref = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = ref.rle_iou_ref(rows_d, rows_g, crowd)
        for rng in ref.AREA_RNG:
            ref.evaluate_img_ref(want, ad, ag, crowd, rng, ref.IOU_THRS)
        t_ref.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(flat.cpu().numpy().reshape(30, 100).T, want)
    rows.append(dict(case, what="numpy_restatement (tests/test_cocoeval_host.py: rle_iou_ref + evaluate_img_ref), wall clock, host",
                     **spread(t_ref)))

    # (c) evaluate() on a synthetic data set
    data, results = synthetic_dataset(torch, image, args.images)
    case = dict(case=f"synthetic evaluation: {len(data['images'])} images 240x320, {len(data['annotations'])} ground truths, "
                     f"{len(results)} detections, 4 categories", device=torch.cuda.get_device_name(0))
    for iou_type in ("segm", "bbox"):
        ev = cocoeval.evaluate(data, results, iou_type)          # warm-up
        wall, device = [], []
        for _ in range(max(3, args.reps // 3)):
            ops.CONV_PROFILE = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev = cocoeval.evaluate(data, results, iou_type)
            wall.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            device.append(sum(r[0].elapsed_time(r[1]) for r in ops.CONV_PROFILE if r[5] in ("rle_iou", "bbox_iou", "coco_match")))
            ops.CONV_PROFILE = None
        groups = sum(1 for v in ev.ious.values() if len(v))
        rows.append(dict(case, what=f"cocoeval.evaluate(iou_type={iou_type!r}), wall clock of the whole call", groups_with_pairs=groups,
                         ap=round(float(ev.stats[0]), 4), **spread(wall)))
        rows.append(dict(case, what=f"  of which the grouped IoU call + the grouped matching call ({iou_type}), HIP events", **spread(device)))

    # (d) the restatement's IoU + matching over the same groups (segm)
    t0 = time.perf_counter()
    by_key = {}
    for a in data["annotations"]:
        by_key.setdefault((a["image_id"], a["category_id"]), ([], []))[1].append(a)
    for i, r in enumerate(results):
        by_key.setdefault((r["image_id"], r["category_id"]), ([], []))[0].append(dict(r, area=r["bbox"][2] * r["bbox"][3]))
    for key, (d, g) in by_key.items():
        d = [d[i] for i in np.argsort([-x["score"] for x in d], kind="mergesort")][:100]
        crowd = [x["iscrowd"] for x in g]
        ious = ref.rle_iou_ref([image.rle_counts(x["segmentation"]) for x in d], [image.rle_counts(x["segmentation"]) for x in g], crowd) \
            if d and g else []
        for rng in ref.AREA_RNG:
            ref.evaluate_img_ref(ious, [x["area"] for x in d], [x["area"] for x in g], crowd, rng, ref.IOU_THRS)
    rows.append(dict(case, what="numpy_restatement of the IoU + matching over the same groups (segm; string decoding included), wall "
                                "clock, host", **spread([(time.perf_counter() - t0) * 1e3])))

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
