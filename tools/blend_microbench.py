#!/usr/bin/env python3
"""Times ops.blend_instances (csrc/overlay.hip): data.blend_image's masks, outlines and boxes in one launch. Recorded, not asserted.

    python tools/blend_microbench.py [--out profiles/blend_microbench.jsonl] [--reps 9] [--masks 50] [--height 1200] [--width 1920]

The workload is synthetic and seeded (no fixture is involved): --masks blobs (the union of two ellipses, as tools/codec_microbench.py
makes them) of --height x --width with their bounding boxes, a random image, the palette of image.random_colors.
  blend_instances  HIP events around the call, the median of --reps after a warm-up call; floor_bytes = N*H*W + 6*H*W (every mask
                   byte and the image read once, the output written once) and the rate that makes of the median. An event pair
                   around ONE call on an idle GPU also holds the host's way to the launch (the binding's checks, the launch
                   itself), which for a kernel this short is most of it; queued_ms_per_call is the kernel alone: --queued calls
                   enqueued behind some milliseconds of device copies, so the host is ahead of the GPU, one event pair around
                   them all, divided by their number (median of --reps such bursts).
  device_copy      a plain device-to-device copy of floor_bytes / 2 bytes (it reads and writes: floor_bytes of traffic) in the same
                   process, timed both ways: blend_over_copy is the ratio of the two queued times, the inverse of the fraction
                   of copy rate the kernel reaches.
  pillow_cpu       when Pillow imports: the same composite by the PIL calls of data.blend_mask / blend_image (Image.blend, two
                   Image.composite, ImageFilter.CONTOUR, ImageDraw.rectangle) on one thread of the CPU named in the line, wall
                   clock, masks already on the host; its output is compared with the kernel's. Context only.
One JSON line per measurement. Needs the GPU."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from codec_microbench import blobs, cpu_name, spread, timed  # noqa: E402


def pillow_composite(image, masks, colors, boxes):
    """The composite with Pillow's own full-frame operations, the way data.blend_image gets it (per instance a blend at 0.2, an
    inverted 3 x 3 CONTOUR without the frame, two composites; then the rectangles), without the labels."""
    from PIL import Image, ImageChops, ImageDraw, ImageFilter
    fusion = Image.fromarray(image)
    inner = Image.new("L", fusion.size, 0)
    if fusion.width > 2 and fusion.height > 2:
        inner.paste(255, (1, 1, fusion.width - 1, fusion.height - 1))
    for m, c in zip(masks, colors):
        solid = Image.new("RGB", fusion.size, c)
        on = Image.fromarray(m * 255)
        outline = ImageChops.multiply(ImageChops.invert(on.filter(ImageFilter.CONTOUR)), inner)
        fusion = Image.composite(solid, Image.composite(Image.blend(fusion, solid, 0.2), fusion, on), outline)
    draw = ImageDraw.Draw(fusion)
    for (y1, x1, y2, x2), c in zip(boxes, colors):
        draw.rectangle((x1, y1, x2, y2), None, c)
    return fusion


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blend_microbench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--masks", type=int, default=50)
    ap.add_argument("--queued", type=int, default=20)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1920)
    args = ap.parse_args()
    import numpy as np
    import torch
    from maskrcnn_amd import image, ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(20251019)
    n, h, w = args.masks, args.height, args.width
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()

    def emit(row):
        with open(args.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
        print(json.dumps(row), flush=True)

    masks = blobs(torch, n, h, w, gen, dev)
    img = torch.randint(0, 256, (h, w, 3), generator=gen, dtype=torch.uint8).to(dev)
    ys, xs = masks.any(2), masks.any(1)
    first = lambda t: t.to(torch.uint8).argmax(1)
    last = lambda t: t.size(1) - 1 - t.flip(1).to(torch.uint8).argmax(1)
    boxes = torch.stack([first(ys), first(xs), last(ys), last(xs)], 1).to(torch.int32)
    random.seed(1)
    palette = image.random_colors(n)
    colors = torch.tensor(palette, dtype=torch.uint8, device=dev)
    out = torch.empty_like(img)
    run = lambda: ops.blend_instances(img, masks, colors, boxes, 0, out)
    floor = n * h * w + 6 * h * w
    sizes = dict(masks=n, image=[h, w], on_fraction=round(float(masks.float().mean()), 4), floor_bytes=floor,
                 device=torch.cuda.get_device_name(0))
    src = torch.empty(floor // 2, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)
    ballast = torch.empty(1 << 30, dtype=torch.uint8, device=dev)

    def queued(fn):
        """ms per call of --queued calls enqueued while the GPU is still busy with 2 GiB of copies."""
        ballast[:1 << 29].copy_(ballast[1 << 29:])
        ballast[1 << 29:].copy_(ballast[:1 << 29])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.queued):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.queued

    t = spread(timed(torch, run, args.reps))
    q = sorted(queued(run) for _ in range(args.reps))[args.reps // 2]
    emit(dict(what="blend_instances", **t, queued_ms_per_call=round(q, 4), floor_gb_per_s=round(floor / q / 1e6, 1), **sizes))
    tc = spread(timed(torch, lambda: dst.copy_(src), args.reps))
    qc = sorted(queued(lambda: dst.copy_(src)) for _ in range(args.reps))[args.reps // 2]
    emit(dict(what="device_copy", **tc, queued_ms_per_call=round(qc, 4), bytes_copied=floor // 2, traffic_bytes=2 * (floor // 2),
              traffic_gb_per_s=round(2 * (floor // 2) / qc / 1e6, 1), blend_over_copy=round(q / qc, 2),
              device=torch.cuda.get_device_name(0)))
    try:
        import PIL
    except ImportError:
        return
    got = run().cpu().numpy()
    h_img, h_masks, h_boxes = img.cpu().numpy(), masks.cpu().numpy(), boxes.cpu().tolist()
    t0 = time.perf_counter()
    want = np.array(pillow_composite(h_img, h_masks, palette, h_boxes))
    emit(dict(what="pillow_cpu", wall_ms=round((time.perf_counter() - t0) * 1e3, 1), masks=n, image=[h, w], cpu=cpu_name(), threads=1,
              pillow=PIL.__version__, equal_to_kernel=bool(np.array_equal(got, want)),
              note="data.blend_image's PIL calls without the labels, masks already on the host; context only"))


if __name__ == "__main__":
    main()
