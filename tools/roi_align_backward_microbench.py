#!/usr/bin/env python3
"""Times the backward of the pyramid RoIAlign (ops.roi_align_pyramid_backward, csrc/roi_align_backward.hip) at a training step's
shapes. Recorded, not asserted: no ratio is promised.

    python tools/roi_align_backward_microbench.py [--out profiles/roi_align_backward_microbench.jsonl] [--reps 9] [--inner 5]
        [--label key=value ...]   extra fields for every line: what tells two builds apart (MRCNN_LIB=<variant> ... --label threads=256)

The workload is synthetic and seeded: 8 images of 1024 x 1024, C = 256, maps 256^2 .. 32^2 (P2 .. P5), RoIs with log-uniform sides
(0.03 .. 0.6 of the image, so all four levels occur), 200 per image at pool 7 (the classifier head) and 66 per image at pool 14 (the
mask head). Everything is on the device before the clock starts. HIP events go around --inner back-to-back calls after a warm-up
of every shape, the time of one call is the quotient, and the median of --reps such windows is reported with the minimum and the
maximum; the measurements alternate inside a repetition. Per head:
  roi_align_pyramid_backward   the new op, `out=` preallocated: two launches, every byte of the four gradients written
  atomic_route                 what the library offered before for the same gradients, composed here per level, as the reference goes about
                               it (model.py:323-374): the levels from torch ops, per level `torch.nonzero` (a host read-back), the
                               rows' gradients turned NCHW (ops.nhwc_to_nchw), torch.ops.maskrcnn.crop_backward (memset + fp32
                               atomics) on an NCHW buffer, and ops.nchw_to_nhwc of the result. Its sums have no fixed order; the
                               largest difference from the new op's result is recorded (max_abs_diff), not bounded.
  fill                         a plain device fill of the four gradient buffers: the floor, since every byte must be written
One JSON line per measurement and head. Needs the GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BATCH, CHANNELS, IMAGE = 8, 256, 1024
MAP_SIZES = [(256, 256), (128, 128), (64, 64), (32, 32)]
HEADS = (("classifier", 200, 7), ("mask", 66, 14))


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def make_rois(np, per_image, seed):
    rng = np.random.default_rng(seed)
    n = BATCH * per_image
    side = np.exp(rng.uniform(np.log(0.03), np.log(0.6), (n, 2)))
    centre = rng.uniform(0.0, 1.0, (n, 2))
    return np.clip(np.concatenate([centre - side / 2, centre + side / 2], 1), 0.0, 1.0).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_align_backward_microbench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--label", action="append", default=[], metavar="key=value")
    args = ap.parse_args()
    labels = {k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in (item.split("=", 1) for item in args.label)}
    import numpy as np
    import torch
    from maskrcnn_amd import ops
    assert torch.cuda.is_available(), "roi_align_backward_microbench needs the GPU"
    dev = torch.device("cuda:0")
    area = float(IMAGE * IMAGE)

    def window_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.inner

    out = [torch.empty(BATCH, h, w, CHANNELS, device=dev) for h, w in MAP_SIZES]
    nchw = [torch.empty(BATCH, CHANNELS, h, w, device=dev) for h, w in MAP_SIZES]
    rows = []
    for head, per_image, pool in HEADS:
        rois = torch.from_numpy(make_rois(np, per_image, 20261020 + pool)).to(dev)
        n = rois.size(0)
        g = torch.Generator(device="cpu").manual_seed(pool)
        grad = torch.randn(n, pool, pool, CHANNELS, generator=g).to(dev)
        image = torch.arange(n, device=dev, dtype=torch.int32) // per_image
        image_area = torch.tensor([area], device=dev)

        def ours():
            return ops.roi_align_pyramid_backward(grad, rois, pool, area, BATCH, MAP_SIZES, rois_per_image=per_image, out=out)

        def atomic_route():
            # equation 1 of the FPN paper on normalised boxes, in a few small torch launches: k = 4 + log2(sqrt(box area * image
            # area) / 224), nearest level, 2 .. 5 (a box on a boundary may go the other way than in the kernel: this is a timing)
            box_area = (rois[:, 2] - rois[:, 0]) * (rois[:, 3] - rois[:, 1])
            level = torch.floor(4.5 + 0.5 * torch.log2(box_area * image_area / (224.0 * 224.0))).clamp(2, 5)
            result = []
            for i, lv in enumerate(range(2, 6)):
                ix = torch.nonzero(level == lv)[:, 0]                             # a host read-back per level
                if ix.numel():
                    torch.ops.maskrcnn.crop_backward(ops.nhwc_to_nchw(grad[ix]), rois[ix], image[ix], nchw[i])
                else:
                    nchw[i].zero_()
                result.append(ops.nchw_to_nhwc(nchw[i]))
            return result

        def fill():
            for t in out:
                t.zero_()

        theirs = atomic_route()
        mine = [t.clone() for t in ours()]
        torch.cuda.synchronize()
        diff = max(float((a - b).abs().max()) for a, b in zip(mine, theirs))
        scale = max(float(a.abs().max()) for a in mine)
        del theirs, mine
        timed = {"roi_align_pyramid_backward": ours, "atomic_route": atomic_route, "fill": fill}
        for fn in timed.values():                                                     # warm-up of every shape
            window_ms(fn)
        torch.cuda.synchronize()
        t = {k: [] for k in timed}
        for _ in range(args.reps):
            for k, fn in timed.items():
                t[k].append(window_ms(fn))
        sizes = dict(head=head, batch=BATCH, channels=CHANNELS, map_sizes=MAP_SIZES, rois_per_image=per_image, pool=pool,
                     gradient_bytes=4 * CHANNELS * BATCH * sum(h * w for h, w in MAP_SIZES), inner=args.inner,
                     max_abs_diff=diff, max_abs_gradient=scale, device=torch.cuda.get_device_name(0))
        rows += [dict(what=k, **labels, **spread(v), **sizes) for k, v in t.items()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
