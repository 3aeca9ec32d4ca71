#!/usr/bin/env python3
"""Times the training ground truth made on the GPU — ops.rle_resample (csrc/gt_masks.hip) alone and ground_truth.load_batch end
to end — and, in the same process, what the parent commit offers for the same job: per image size ops.rle_decode +
ops.resize_bilinear_u8 + a pad copy. Recorded, not asserted.

    python tools/gt_masks_microbench.py [--out profiles/gt_masks_microbench.jsonl] [--reps 9] [--masks 20]

The workload is synthetic and seeded: 8 and 16 images of COCO-like sizes (480 x 640 and its neighbours, mixed, every image of a
batch another size), --masks blobs each (the union of two ellipses), to a 1024 x 1024 canvas (IMAGE_MIN_DIM 800, IMAGE_MAX_DIM
1024), every other image mirrored. Three of four annotations reach load_batch as polygons (the blob's outline as a 24-gon, as a
stock instances_*.json would have them), the fourth as a compressed string.
  rle_resample   ONE call over all rows of the batch, the table and the geometry on the device.
  composition    the same masks from the same table: per image rle_decode, torch.flip where mirrored, resize_bilinear_u8, a copy
                 into the zeroed canvas. Its output is compared with rle_resample's (equal bytes).
  load_batch     ground_truth.load_batch(gt, ids, 800, 1024, hflip=...) on the device, from the dict to the GroundTruth: host
                 work, copies and its one synchronisation included.
HIP events around each, the median of --reps after a warm-up call. One JSON line per measurement. Needs the GPU."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(480, 640), (640, 480), (427, 640), (375, 500), (640, 426), (333, 500), (612, 612), (480, 639), (500, 375), (428, 640),
         (640, 427), (360, 640), (478, 640), (640, 512), (500, 333), (426, 640)]


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def timed(torch, fn, reps):
    fn()                                                        # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def blob_params(torch, n, gen):
    return torch.rand(n, 2, 4, generator=gen)


def blobs(torch, p, h, w, dev):
    """Seeded blobs [n,h,w] uint8 on the device: the union of two ellipses."""
    p = p.to(dev)
    yy = torch.arange(h, device=dev, dtype=torch.float32)[None, :, None]
    xx = torch.arange(w, device=dev, dtype=torch.float32)[None, None, :]
    out = torch.zeros(p.size(0), h, w, dtype=torch.bool, device=dev)
    for k in range(2):
        cy, cx = p[:, k, 0, None, None] * h, p[:, k, 1, None, None] * w
        ry, rx = (0.03 + 0.2 * p[:, k, 2, None, None]) * h, (0.03 + 0.2 * p[:, k, 3, None, None]) * w
        out |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return out.view(torch.uint8)


def polygon_parts(p, h, w):
    """The two ellipses of one blob as 24-gons (two parts of one annotation)."""
    parts = []
    for k in range(2):
        cy, cx, ry, rx = float(p[k, 0]) * h, float(p[k, 1]) * w, (0.03 + 0.2 * float(p[k, 2])) * h, (0.03 + 0.2 * float(p[k, 3])) * w
        parts.append([round(v, 2) for t in range(24) for v in (cx + rx * math.cos(t * math.pi / 12), cy + ry * math.sin(t * math.pi / 12))])
    return parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_masks_microbench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--masks", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    from maskrcnn_amd import ground_truth, image, ops
    dev = torch.device("cuda:0")
    min_dim, max_dim = 800, 1024
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()

    def emit(row):
        with open(args.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
        print(json.dumps(row), flush=True)

    for batch in (8, 16):
        gen = torch.Generator().manual_seed(20260120 + batch)
        sizes, flips = SIZES[:batch], [bool(i % 2) for i in range(batch)]
        plans = [ground_truth._plan(h, w, min_dim, max_dim) for h, w in sizes]
        gt = dict(images=[dict(id=i + 1, height=h, width=w) for i, (h, w) in enumerate(sizes)], categories=[dict(id=1, name="blob")],
                  annotations=[])
        parts = []
        for i, (h, w) in enumerate(sizes):
            p = blob_params(torch, args.masks, gen)
            enc = image.rle_masks(blobs(torch, p, h, w, dev))
            parts.append((np.arange(i * args.masks, (i + 1) * args.masks), enc.num_runs, enc.counts))
            for k, seg in enumerate(enc.to_coco()):
                seg = polygon_parts(p[k], h, w) if k % 4 else {"size": seg["size"], "counts": seg["counts"].decode("ascii")}
                gt["annotations"].append(dict(id=len(gt["annotations"]) + 1, image_id=i + 1, category_id=1, iscrowd=0, segmentation=seg))
        n = batch * args.masks
        num_runs, counts = image._merge_tables(n, parts, dev)
        per_row = lambda f: torch.tensor([f(i) for i in range(batch) for _ in range(args.masks)], dtype=torch.int32).to(dev)
        hs, ws = per_row(lambda i: sizes[i][0]), per_row(lambda i: sizes[i][1])
        geom = per_row(lambda i: [plans[i].new_h, plans[i].new_w, plans[i].top, plans[i].left, int(flips[i])])
        out = torch.empty(n, max_dim, max_dim, dtype=torch.uint8, device=dev)
        common = dict(images=batch, masks_per_image=args.masks, canvas=[max_dim, max_dim], sizes=sizes, runs=int(num_runs.sum()),
                      capacity=int(counts.size(1)), bytes_written=int(out.numel()), device=torch.cuda.get_device_name(0))

        def resample():
            return ops.rle_resample(num_runs, counts, hs, ws, geom, max_dim, max_dim, out=out)

        emit(dict(what="rle_resample", **spread(timed(torch, resample, args.reps)), launches=2, **common))
        _, status = resample()
        assert not status.any().item()

        other = torch.empty_like(out)

        def composition():
            other.zero_()
            for i, (p, (h, w)) in enumerate(zip(plans, sizes)):
                rows = slice(i * args.masks, (i + 1) * args.masks)
                m = ops.rle_decode(num_runs[rows], counts[rows], h, w)
                if flips[i]:
                    m = torch.flip(m, dims=[2])
                if (p.new_h, p.new_w) != (h, w):
                    m = ops.resize_bilinear_u8(m, p.new_h, p.new_w)
                other[rows, p.top:p.top + p.new_h, p.left:p.left + p.new_w] = m
            return other

        emit(dict(what="composition_decode_resize_pad", **spread(timed(torch, composition, args.reps)), **common))
        assert torch.equal(composition(), out)

        ids = [i + 1 for i in range(batch)]
        load = lambda: ground_truth.load_batch(gt, ids, min_dim, max_dim, hflip=flips, device=dev)
        emit(dict(what="load_batch", **spread(timed(torch, load, args.reps)), polygons=sum(isinstance(a["segmentation"], list) for a in gt["annotations"]),
                  strings=sum(isinstance(a["segmentation"], dict) for a in gt["annotations"]), **common))
        got = load()
        assert got.gt_masks.shape == out.shape and got.gt_off.tolist() == [i * args.masks for i in range(batch + 1)]
        strings = torch.arange(0, n, 4, device=dev)                 # the rows load_batch read from the same compressed strings
        assert torch.equal(got.gt_masks[strings], out[strings])


if __name__ == "__main__":
    main()
