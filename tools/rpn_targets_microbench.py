#!/usr/bin/env python3
"""Times the RPN training-target kernels: ops.anchor_match, ops.sample_by_key, ops.rpn_deltas (csrc/targets.hip) and the front
end targets.rpn_targets. Recorded, not asserted: there is no earlier implementation here to regress against, and the reference
does not exist where the GPU is, so no ratio is claimed.

    python tools/rpn_targets_microbench.py [--out profiles/rpn_targets_microbench.jsonl] [--reps 9] [--batches 8,16] [--boxes 20]

The workload is synthetic and seeded (no fixture is involved): the 261 888 pyramid anchors of the 1024 x 1024 config, B images
with --boxes whole-pixel boxes each, count = 128, hashed keys. Everything is on the device before the clock starts, HIP events
go around each call after a warm-up call, and the median of --reps runs is reported with the minimum and the maximum:
  anchor_match / sample_by_key / rpn_deltas   one call each, fed with the call before's output
  rpn_targets                                 the front end on packed device tensors with given keys (the three calls)
  rpn_targets_drawn_keys                      the same with keys=None: torch.randint on the device is inside the clock
One JSON line per measurement and batch size. Needs the GPU.

    python tools/rpn_targets_microbench.py --reference-source <reference tree> [--out ...]

For context only, and without a GPU: imports data.py of that tree (third-party modules it does not need here replaced by empty
placeholders), runs its rpn_samples on the SAME inputs image after image as its data feed does, and APPENDS one line per batch
size, what = "reference_rpn_samples_cpu", wall clock, labelled with the CPU it ran on. It is a different machine from the GPU
lines' unless the file says otherwise; no ratio is claimed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COUNT = 128


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def workload(np, batch, boxes, seed=20261019, side=1024):
    """→ (gt_boxes float32 [batch*boxes,4], ids int32, off int32 [batch+1], keys int32 [batch,261888])"""
    rng = np.random.default_rng(seed + batch)
    n = batch * boxes
    y1, x1 = rng.uniform(0, side - 16, n), rng.uniform(0, side - 16, n)
    h, w = rng.uniform(16, 500, n), rng.uniform(16, 500, n)
    b = np.round(np.stack([y1, x1, np.minimum(y1 + h, side), np.minimum(x1 + w, side)], 1)).astype(np.float32)
    ids = rng.integers(1, 81, n).astype(np.int32)
    a = 261888
    keys = ((np.arange(batch * a, dtype=np.uint64) + np.uint64(1)) * np.uint64(2654435761) & np.uint64(0xffffffff)) >> np.uint64(1)
    return b, ids, (np.arange(batch + 1) * boxes).astype(np.int32), keys.astype(np.int32).reshape(batch, a)


def full_anchors(torch):
    from maskrcnn_amd import anchors
    from maskrcnn_amd.config import InferenceConfig
    return anchors.pyramid_anchors(InferenceConfig(), dtype=torch.float64)


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def reference_cpu(args):
    import platform
    import time
    import types
    import numpy as np
    import torch

    def placeholder(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    sys.dont_write_bytecode = True
    sk = placeholder("skimage")
    sk.io, sk.color = placeholder("skimage.io"), placeholder("skimage.color")
    sk.measure, sk.transform = placeholder("skimage.measure", find_contours=None), placeholder("skimage.transform")
    tv = placeholder("torchvision")
    tv.datasets, tv.transforms = placeholder("torchvision.datasets", CocoDetection=object), placeholder("torchvision.transforms")
    import scipy
    if not hasattr(scipy, "misc"):
        scipy.misc = placeholder("scipy.misc")
    sys.path.insert(0, os.path.abspath(args.reference_source))
    import data as rdata
    cfg = types.SimpleNamespace(RPN_TRAIN_ANCHORS_PER_IMAGE=COUNT, RPN_BBOX_STD_DEV=[0.1, 0.1, 0.2, 0.2])
    anchors = full_anchors(torch).numpy()
    cpu = platform.processor() or platform.machine()
    try:
        cpu = next(l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name"))
    except (OSError, StopIteration):
        pass
    for batch in args.batches:
        boxes, ids, off, _ = workload(np, batch, args.boxes)
        times = []
        for _ in range(max(1, min(args.reps, 3))):
            np.random.seed(0)
            t0 = time.perf_counter()
            for i in range(batch):
                rdata.rpn_samples(anchors, ids[off[i]:off[i + 1]], boxes[off[i]:off[i + 1]], cfg)
            times.append((time.perf_counter() - t0) * 1e3)
        row = dict(what="reference_rpn_samples_cpu", **spread(times), batch=batch, boxes_per_image=args.boxes, anchors=int(anchors.shape[0]),
                   count=COUNT, cpu=cpu, torch_threads=torch.get_num_threads(),
                   note="the reference's data.rpn_samples image after image on the CPU named here: NOT the machine of the GPU lines; "
                        "context only")
        with open(args.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
        print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rpn_targets_microbench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batches", type=lambda s: [int(v) for v in s.split(",")], default=[8, 16])
    ap.add_argument("--boxes", type=int, default=20)
    ap.add_argument("--reference-source", default=None, help="the reference tree: time its rpn_samples on this CPU instead (no GPU needed)")
    args = ap.parse_args()
    if args.reference_source:
        return reference_cpu(args)
    import numpy as np
    import torch
    from maskrcnn_amd import ops, targets
    dev = torch.device("cuda:0")
    anchors = full_anchors(torch).to(dev)
    rows = []
    for batch in args.batches:
        boxes, ids, off, keys = (torch.from_numpy(v).to(dev) for v in workload(np, batch, args.boxes))
        match_fn = lambda: ops.anchor_match(anchors, boxes, ids, off)
        matched = match_fn()                                                   # warm-up
        sample_fn = lambda: ops.sample_by_key(matched[0], keys, COUNT)
        sampled = sample_fn()
        delta_fn = lambda: ops.rpn_deltas(anchors, boxes, off, sampled, matched[1], COUNT)
        delta_fn()
        front_fn = lambda: targets.rpn_targets(anchors, boxes, ids, COUNT, keys=keys, device=dev, gt_off=off)
        drawn_fn = lambda: targets.rpn_targets(anchors, boxes, ids, COUNT, device=dev, gt_off=off)
        front_fn(), drawn_fn()
        torch.cuda.synchronize()
        assert not matched[4].any() and int((sampled != 0).sum()) == batch * COUNT
        t = {k: [] for k in ("anchor_match", "sample_by_key", "rpn_deltas", "rpn_targets", "rpn_targets_drawn_keys")}
        for _ in range(args.reps):
            for k, fn in zip(t, (match_fn, sample_fn, delta_fn, front_fn, drawn_fn)):
                t[k].append(event_ms(torch, fn)[0])
        sizes = dict(batch=batch, boxes_per_image=args.boxes, anchors=int(anchors.size(0)), count=COUNT,
                     positives=int((matched[0] == 1).sum()), negatives=int((matched[0] == -1).sum()),
                     device=torch.cuda.get_device_name(0))
        rows += [dict(what=k, **spread(v), **sizes) for k, v in t.items()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
