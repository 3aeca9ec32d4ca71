#!/usr/bin/env python3
"""Times the COCO RLE path against the copy it replaces, on the 400-mask 1200 x 1920 case: 50 masks pasted by ops.paste_masks
from seeded 28 x 28 masks and boxes (the case of tests/test_gpu_rle.py), tiled to 400 = eight images of 50 detections
(921 MB of dense masks).

    python tools/rle_probe.py [--out profiles/rle_encode_microbench.jsonl] [--reps 9] [--masks 400]

  (a) ops.rle_encode                    HIP events around the call, after a warm-up; GB/s against the n*h*w bytes it must read
  (b) RleMasks.to_coco()                wall clock from a synchronised device to the list of dicts (its device-to-host copy included)
  (c) masks.cpu()                       wall clock of the dense copy a caller without the encoder needs, same process
One JSON line per measurement (median, min, max of the repetitions, in ms) and one with the ratio (a + b) / c. Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pasted_masks(ops, torch, n=50, height=1200, width=1920, seed=3):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, 28), torch.linspace(-1, 1, 28), indexing="ij")
    blobs = []
    for _ in range(n):
        a, b, c = (torch.rand(3, generator=g) * 0.8 + 0.3).tolist()
        field = 1.0 - (xx / a) ** 2 - (yy / b) ** 2 + c * 0.3 * torch.sin(5 * xx) * torch.cos(4 * yy)
        blobs.append(torch.sigmoid(4 * field + 0.5 * torch.randn(28, 28, generator=g)))
    m28 = torch.stack(blobs)[:, :, :, None].contiguous()
    y1 = torch.rand(n, generator=g) * (height - 80)
    x1 = torch.rand(n, generator=g) * (width - 80)
    y2 = torch.minimum(y1 + 40 + torch.rand(n, generator=g) * 700, torch.tensor(float(height)))
    x2 = torch.minimum(x1 + 40 + torch.rand(n, generator=g) * 900, torch.tensor(float(width)))
    boxes = torch.stack([y1, x1, y2, x2], 1)
    return ops.paste_masks(m28.cuda(), torch.zeros(n, dtype=torch.int64, device="cuda"), boxes.cuda(), height, width,
                           channels_last=True)


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_encode_microbench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--masks", type=int, default=400)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rle_probe.py needs a GPU")
    from maskrcnn_amd import image as imagelib, ops
    assert args.reps >= 5 and args.masks % 50 == 0
    masks = pasted_masks(ops, torch).repeat(args.masks // 50, 1, 1)
    n, h, w = masks.shape
    nbytes = n * h * w
    case = dict(masks=n, height=h, width=w, dense_bytes=nbytes, device=torch.cuda.get_device_name(0))

    for _ in range(3):                                       # warm-up of all three paths (code objects, allocator, pinned staging)
        enc = ops.rle_encode(masks)
        imagelib.RleMasks((h, w), *enc).to_coco()
    masks[:50].cpu()
    torch.cuda.synchronize()
    a_ms, b_ms, c_ms = [], [], []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        enc = ops.rle_encode(masks)
        e1.record()
        torch.cuda.synchronize()
        a_ms.append(e0.elapsed_time(e1))
        rle = imagelib.RleMasks((h, w), *enc)
        t = time.perf_counter()
        coco = rle.to_coco()
        b_ms.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        host = masks.cpu()
        c_ms.append((time.perf_counter() - t) * 1e3)
        del host
    runs = enc[0].cpu()
    rows = [dict(case, what="a_rle_encode", **spread(a_ms), gb_per_s=round(nbytes / statistics.median(a_ms) / 1e6, 1),
                 capacity=int(enc[1].size(1)), max_runs=int(runs.max())),
            dict(case, what="b_to_coco", **spread(b_ms), string_bytes=sum(len(c["counts"]) for c in coco)),
            dict(case, what="c_dense_masks_cpu_copy", **spread(c_ms), gb_per_s=round(nbytes / statistics.median(c_ms) / 1e6, 1)),
            dict(case, what="ratio_a_plus_b_over_c",
                 value=round((statistics.median(a_ms) + statistics.median(b_ms)) / statistics.median(c_ms), 5))]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            line = json.dumps(r)
            print(line)
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
