#!/usr/bin/env python3
"""Times the RLE codec kernels on tables — ops.rle_from_string, ops.rle_area_bbox, ops.rle_to_string, ops.rle_decode
(csrc/codec.hip) — and cocoeval.evaluate with and without the device route for compressed strings. Recorded, not asserted.

    python tools/codec_microbench.py [--out profiles/codec_microbench.jsonl] [--reps 9] [--masks 100000] [--images 5000]

The workload is synthetic and seeded (no fixture is involved):
  result masks   --masks blobs (the union of two ellipses) on 480 x 640, made and encoded on the GPU in batches; their compressed
                 strings are what a result file holds. The lines carry the total characters and runs.
  rle_from_string / rle_area_bbox / rle_to_string   ONE call each over all of them, the arguments on the device and the sizes
                 given, so no call synchronises; HIP events around the call, the median of --reps after a warm-up call.
  rle_from_string_long   the wave-per-string kernel's worst case: 1 and 64 strings of 20 000 runs (~50 000 characters) each.
  rle_decode     400 blobs of 1200 x 1920 (the README's encode workload in reverse), likewise.
  evaluate       wall clock of cocoeval.evaluate(gt, results, "segm") on --images images x 20 detections (the first images*20
                 masks as records without a bbox, every fourth one also a ground truth, three categories), once with
                 compressed strings decoded on the device and once on the host — the per-character numpy route that is still
                 in the tree — in this one process. The stats of the two runs are compared.
  rle_counts_cpu for context only: image.rle_counts over a 2 000-string sample, wall clock on the CPU named in the line.
One JSON line per measurement. Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def timed(torch, fn, reps):
    fn()                                                        # warm-up
    torch.cuda.synchronize()
    return [event_ms(torch, fn)[0] for _ in range(reps)]


def blobs(torch, n, h, w, gen, dev):
    """n seeded blobs [n,h,w] uint8 on the device: the union of two ellipses."""
    p = torch.rand(n, 2, 4, generator=gen).to(dev)
    yy = torch.arange(h, device=dev, dtype=torch.float32)[None, :, None]
    xx = torch.arange(w, device=dev, dtype=torch.float32)[None, None, :]
    out = torch.zeros(n, h, w, dtype=torch.bool, device=dev)
    for k in range(2):
        cy, cx = p[:, k, 0, None, None] * h, p[:, k, 1, None, None] * w
        ry, rx = (0.03 + 0.2 * p[:, k, 2, None, None]) * h, (0.03 + 0.2 * p[:, k, 3, None, None]) * w
        out |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return out.view(torch.uint8)


def cpu_name():
    try:
        return next(l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name"))
    except (OSError, StopIteration):
        import platform
        return platform.processor() or platform.machine()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_microbench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--masks", type=int, default=100000)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--decode-masks", type=int, default=400)
    args = ap.parse_args()
    import numpy as np
    import torch
    from maskrcnn_amd import cocoeval, image, ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(20250801)
    h, w = 480, 640
    rows, done = [], 0

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()

    def emit(row):                                              # written line by line: a long run that is cut short keeps its lines
        rows.append(row)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
        print(json.dumps(row), flush=True)

    # the result strings, as a file would hold them
    strings = []
    while done < args.masks:
        n = min(1000, args.masks - done)
        strings += [d["counts"] for d in image.rle_masks(blobs(torch, n, h, w, gen, dev)).to_coco()]
        done += n
    data = np.frombuffer(b"".join(strings), dtype=np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)
    tokens = ops.rle_string_tokens(data, off)
    cap = int(tokens.max())
    sizes = dict(masks=args.masks, image=[h, w], characters=int(data.size), runs=int(tokens.sum()), capacity=cap,
                 device=torch.cuda.get_device_name(0))
    d_data, d_off = torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev)
    d_h = torch.full((args.masks,), h, dtype=torch.int32, device=dev)
    d_w = torch.full((args.masks,), w, dtype=torch.int32, device=dev)
    frs = lambda: ops.rle_from_string(d_data, d_off, d_h, d_w, capacity=cap)
    emit(dict(what="rle_from_string", **spread(timed(torch, frs, args.reps)), **sizes))
    num_runs, counts, status = frs()
    assert not status.any().item() and torch.equal(num_runs.cpu(), torch.from_numpy(tokens.astype(np.int32)))
    # the worst case of the wave-per-string kernel: long strings, read serially by one wave each (20 000 runs, ~50 000 characters)
    lrng = np.random.default_rng(5)
    mags = (1 << lrng.choice([4, 9, 14, 19], 20000)) - 1
    long_counts = np.where(np.arange(20000) % 4 < 2, 1 + mags, 1).astype(np.uint32)     # alternating large and small: long differences
    lt = torch.from_numpy(long_counts.view(np.int32))[None].to(dev)
    lbytes, loff = ops.rle_to_string(torch.tensor([20000], dtype=torch.int32, device=dev), lt)
    for copies in (1, 64):
        cb = lbytes.repeat(copies)
        co = (torch.arange(copies + 1, device=dev, dtype=torch.int64) * lbytes.numel())
        ch = torch.ones(copies, dtype=torch.int32, device=dev)
        fl = lambda: ops.rle_from_string(cb, co, ch, ch, capacity=20000)
        emit(dict(what="rle_from_string_long", **spread(timed(torch, fl, args.reps)), strings=copies, runs_each=20000,
                  characters_each=int(lbytes.numel()), device=torch.cuda.get_device_name(0)))
        got = fl()
        assert got[0].tolist() == [20000] * copies and torch.equal(got[1][copies - 1], lt[0])
    ab = lambda: ops.rle_area_bbox(num_runs, counts, d_h, d_w)
    emit(dict(what="rle_area_bbox", **spread(timed(torch, ab, args.reps)), **sizes))
    ts = lambda: ops.rle_to_string(num_runs, counts, total_bytes=int(data.size))
    emit(dict(what="rle_to_string", **spread(timed(torch, ts, args.reps)), **sizes))
    back, back_off = ts()
    assert torch.equal(back, d_data) and torch.equal(back_off, d_off)
    areas, bboxes = (t.cpu().numpy() for t in ab())

    # the per-character host reader, for context
    t0 = time.perf_counter()
    for s in strings[:2000]:
        image.rle_counts(s)
    emit(dict(what="rle_counts_cpu", wall_ms=round((time.perf_counter() - t0) * 1e3, 2), strings=min(2000, len(strings)),
              characters=int(off[min(2000, len(strings))]), cpu=cpu_name(), threads=1,
              note="image.rle_counts, the per-character Python loop, on the CPU named here; context only"))

    # evaluate, both routes in one process
    n_img = min(args.images, args.masks // 20)
    gt = dict(images=[dict(id=i + 1, height=h, width=w) for i in range(n_img)], categories=[dict(id=c) for c in (1, 2, 3)],
              annotations=[])
    results = []
    rng = np.random.default_rng(7)
    score = rng.random(n_img * 20)
    for k in range(n_img * 20):
        seg = {"size": [h, w], "counts": strings[k].decode("ascii")}
        results.append(dict(image_id=k // 20 + 1, category_id=k % 3 + 1, score=float(score[k]), segmentation=seg))
        if k % 4 == 0:
            j = (k + 4) % (n_img * 20) if k % 8 else k          # half of the ground truths are another image's mask
            gt["annotations"].append(dict(id=len(gt["annotations"]) + 1, image_id=k // 20 + 1, category_id=k % 3 + 1, iscrowd=0,
                                          segmentation={"size": [h, w], "counts": strings[j].decode("ascii")},
                                          area=float(areas[j]), bbox=[float(v) for v in bboxes[j]]))
    small = dict(gt, images=gt["images"][:20], annotations=[a for a in gt["annotations"] if a["image_id"] <= 20])
    cocoeval.evaluate(small, [r for r in results if r["image_id"] <= 20], "segm", dev)       # warm-up
    stats = {}
    for codec in ("device", "host"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats[codec] = cocoeval._evaluate(gt, results, "segm", dev, "error", codec).stats
        emit(dict(what=f"evaluate_{codec}_route", wall_ms=round((time.perf_counter() - t0) * 1e3, 1), images=n_img,
                  detections=len(results), ground_truths=len(gt["annotations"]), image=[h, w], cpu=cpu_name(),
                  device=torch.cuda.get_device_name(0)))
    assert np.array_equal(stats["device"], stats["host"])

    # decode: the encode workload in reverse
    big = image.rle_masks(blobs(torch, args.decode_masks, 1200, 1920, gen, dev))
    out = torch.empty(args.decode_masks, 1200, 1920, dtype=torch.uint8, device=dev)
    dec = lambda: ops.rle_decode(big.num_runs, big.counts, 1200, 1920, out=out)
    emit(dict(what="rle_decode", **spread(timed(torch, dec, args.reps)), masks=args.decode_masks, image=[1200, 1920],
              runs=int(big.num_runs.sum()), capacity=big.capacity, bytes_written=int(out.numel()),
              device=torch.cuda.get_device_name(0)))


if __name__ == "__main__":
    main()
