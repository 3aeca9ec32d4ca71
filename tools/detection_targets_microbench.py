#!/usr/bin/env python3
"""Times the detection-target kernels: ops.detection_targets and ops.mask_targets (csrc/detection_targets.hip) and the front end
targets.detection_targets. Recorded, not asserted: there is no earlier implementation here to regress against, and the reference
does not exist where the GPU is, so no ratio is claimed.

    python tools/detection_targets_microbench.py [--out profiles/detection_targets_microbench.jsonl] [--reps 9] [--batches 1,8,16]

The workload is synthetic and seeded (no fixture is involved): B images with N = 2000 RoIs (a third of them near a box), 20 boxes
and 20 rectangle masks of 1024 x 1024 bytes each, count = 100, positive_ratio 0.33, 28 x 28 targets, hashed keys. Everything is on
the device before the clock starts, HIP events go around each call after a warm-up call, and the median of --reps runs is
reported with the minimum and the maximum:
  detection_targets / mask_targets        one call each, the second fed with the first's output
  front_end                               targets.detection_targets on packed device tensors with given keys (the two calls)
  front_end_drawn_keys                    the same with keys=None: torch.randint on the device is inside the clock
One JSON line per measurement and batch size. Needs the GPU.

    python tools/detection_targets_microbench.py --reference-source <reference tree> [--out ...]

For context only, and without a GPU: loads that tree's model.py as tests/golden/make_golden.py does (with its CPU extension),
runs its mrn_samples on the SAME inputs image after image (it takes batch size 1), and APPENDS one line per batch size, what =
"reference_mrn_samples_cpu", wall clock, labelled with the CPU it ran on. It is a different machine from the GPU lines' unless the
file says otherwise; no ratio is claimed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COUNT, RATIO, ROIS, BOXES, SIDE, MASK_SHAPE = 100, 0.33, 2000, 20, 1024, (28, 28)


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def workload(np, batch, seed=20261020):
    """→ (rois float32 [batch,ROIS,4], gt_boxes float32 [batch*BOXES,4], ids int32, off int32 [batch+1], keys int32 [batch,ROIS]),
    normalised coordinates."""
    rng = np.random.default_rng(seed + batch)

    def boxes(n, lo, hi):
        y1, x1 = rng.uniform(0, 0.85, n), rng.uniform(0, 0.85, n)
        h, w = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
        return np.stack([y1, x1, np.minimum(y1 + h, 1.0), np.minimum(x1 + w, 1.0)], 1)

    gt = boxes(batch * BOXES, 0.05, 0.5)
    rois = np.zeros((batch, ROIS, 4))
    near = ROIS // 3
    for b in range(batch):
        pick = gt[b * BOXES + rng.integers(0, BOXES, near)]
        size = np.stack([pick[:, 2] - pick[:, 0], pick[:, 3] - pick[:, 1]] * 2, 1)
        rois[b, :near] = np.clip(pick + rng.uniform(-0.1, 0.1, (near, 4)) * size, 0, 1)
        rois[b, near:] = boxes(ROIS - near, 0.03, 0.4)
        rois[b] = rois[b][rng.permutation(ROIS)]
    ids = rng.integers(1, 81, batch * BOXES).astype(np.int32)
    keys = ((np.arange(batch * ROIS, dtype=np.uint64) + np.uint64(1)) * np.uint64(2654435761) & np.uint64(0xffffffff)) >> np.uint64(1)
    return (rois.astype(np.float32), gt.astype(np.float32), ids, (np.arange(batch + 1) * BOXES).astype(np.int32),
            keys.astype(np.int32).reshape(batch, ROIS))


def rectangle_masks(torch, gt, device):
    """uint8 [M,SIDE,SIDE]: 1 inside the box (pixel (y, x) sits at (y, x) / (SIDE - 1))."""
    t = torch.arange(SIDE, device=device, dtype=torch.float32) / (SIDE - 1)
    g = torch.as_tensor(gt, device=device)
    rows = (t[None, :] >= g[:, 0:1]) & (t[None, :] <= g[:, 2:3])
    cols = (t[None, :] >= g[:, 1:2]) & (t[None, :] <= g[:, 3:4])
    return (rows[:, :, None] & cols[:, None, :]).to(torch.uint8)


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def reference_cpu(args):
    import importlib.util
    import platform
    import time
    import types
    import numpy as np
    import torch
    sys.dont_write_bytecode = True
    os.environ["MASKRCNN_REFERENCE"] = os.path.abspath(args.reference_source)
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    rmodel = mg.load_reference()[4]
    cfg = types.SimpleNamespace(GPU_COUNT=0, TRAIN_ROIS_PER_IMAGE=COUNT, ROI_POSITIVE_RATIO=RATIO, BBOX_STD_DEV=[0.1, 0.1, 0.2, 0.2],
                                MASK_SHAPE=list(MASK_SHAPE))
    cpu = platform.processor() or platform.machine()
    try:
        cpu = next(l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name"))
    except (OSError, StopIteration):
        pass
    for batch in args.batches:
        rois, gt, ids, off, _ = workload(np, batch)
        masks = rectangle_masks(torch, gt, "cpu")
        t = [torch.from_numpy(v) for v in (rois, ids, gt)]
        times = []
        for _ in range(max(1, min(args.reps, 3))):
            torch.manual_seed(0)
            t0 = time.perf_counter()
            for i in range(batch):
                s, e = off[i], off[i + 1]
                rmodel.mrn_samples(t[0][i:i + 1], t[1][None, s:e], t[2][None, s:e], masks[None, s:e], cfg)
            times.append((time.perf_counter() - t0) * 1e3)
        row = dict(what="reference_mrn_samples_cpu", **spread(times), batch=batch, rois=ROIS, boxes_per_image=BOXES, mask_side=SIDE,
                   count=COUNT, cpu=cpu, torch_threads=torch.get_num_threads(),
                   note="the reference's model.mrn_samples image after image on the CPU named here: NOT the machine of the GPU lines; "
                        "context only")
        with open(args.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
        print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detection_targets_microbench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batches", type=lambda s: [int(v) for v in s.split(",")], default=[1, 8, 16])
    ap.add_argument("--reference-source", default=None, help="the reference tree: time its mrn_samples on this CPU instead (no GPU needed)")
    args = ap.parse_args()
    if args.reference_source:
        return reference_cpu(args)
    import numpy as np
    import torch
    from maskrcnn_amd import ops, targets
    dev = torch.device("cuda:0")
    rows = []
    for batch in args.batches:
        host = workload(np, batch)
        rois, boxes, ids, off, keys = (torch.from_numpy(v).to(dev) for v in host)
        masks = rectangle_masks(torch, host[1], dev)
        targets_fn = lambda: ops.detection_targets(rois, boxes, ids, off, keys, COUNT, RATIO)
        out = targets_fn()                                                     # warm-up
        masks_fn = lambda: ops.mask_targets(masks, off, out[0], out[4], out[5], MASK_SHAPE)
        masks_fn()
        front_fn = lambda: targets.detection_targets(rois, boxes, ids, masks, COUNT, RATIO, keys=keys, device=dev, gt_off=off)
        drawn_fn = lambda: targets.detection_targets(rois, boxes, ids, masks, COUNT, RATIO, device=dev, gt_off=off)
        front_fn(), drawn_fn()
        torch.cuda.synchronize()
        assert not out[7].any()
        t = {k: [] for k in ("detection_targets", "mask_targets", "front_end", "front_end_drawn_keys")}
        for _ in range(args.reps):
            for k, fn in zip(t, (targets_fn, masks_fn, front_fn, drawn_fn)):
                t[k].append(event_ms(torch, fn)[0])
        sizes = dict(batch=batch, rois=ROIS, boxes_per_image=BOXES, mask_side=SIDE, count=COUNT, positive_ratio=RATIO,
                     num_pos=out[5].tolist(), num_neg=out[6].tolist(), device=torch.cuda.get_device_name(0))
        rows += [dict(what=k, **spread(v), **sizes) for k, v in t.items()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
