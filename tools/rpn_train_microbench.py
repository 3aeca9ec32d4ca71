#!/usr/bin/env python3
"""Times the RPN's training branch on the sampled anchors (csrc/rpn_train.hip, maskrcnn_amd/rpn_train.py) beside the dense route it
replaces, at a training step's shapes. Recorded, not asserted: no ratio is promised.

    python tools/rpn_train_microbench.py [--out profiles/rpn_train_microbench.jsonl] [--reps 9] [--inner 3] [--batches 2,8]
        [--label key=value ...]   extra fields for every line: what tells two builds apart

The workload is synthetic and seeded: images of 1024 x 1024, C = 256, maps 256^2 .. 16^2 (P2 .. P6), 261 888 anchors per image, of
which 64 carry rpn_match = 1 and 64 rpn_match = -1 at random places (count = 128). Everything is on the device before the clock
starts. HIP events go around --inner back-to-back calls after a warm-up of every shape, the time of one call is the quotient, and the
median of --reps such windows is reported with the minimum and the maximum; the measurements alternate inside a repetition. Per batch:
  anchor_compact, pyramid_patch_gather, pyramid_patch_scatter   the three kernels, outputs preallocated where the binding takes them
  sampled_losses_backward   TrainableRPN.losses(...) with .backward(): gradients into the five maps and the six parameters
  dense_losses_backward     the same losses and gradients by the dense route, in the same process: layers.conv_bn_act over the whole
                            maps of all five levels (shared conv + ReLU, fused heads), losses.rpn_losses on every anchor, .backward()
  fill                      a plain device fill of the five gradient maps: the scatter's floor, since every byte must be written
The peak of torch's allocator over one call (beyond what was allocated before it) stands beside the two routes as peak_bytes.
One JSON line per measurement and batch. Needs the GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CHANNELS, HIDDEN, APL, COUNT = 256, 512, 3, 128
MAP_SIZES = [(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)]


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rpn_train_microbench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--batches", default="2,8")
    ap.add_argument("--label", action="append", default=[], metavar="key=value")
    args = ap.parse_args()
    labels = {k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in (item.split("=", 1) for item in args.label)}
    import torch
    from maskrcnn_amd import layers, losses, ops
    from maskrcnn_amd.rpn_train import TrainableRPN
    assert torch.cuda.is_available(), "rpn_train_microbench needs the GPU"
    dev = torch.device("cuda:0")
    anchors = APL * sum(h * w for h, w in MAP_SIZES)

    def window_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.inner

    def peak_bytes(fn):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    g = torch.Generator(device="cpu").manual_seed(20261021)
    rpn = TrainableRPN(CHANNELS, APL, HIDDEN)
    with torch.no_grad():
        for p in rpn.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.02 if p.dim() > 1 else 0.1))
    rpn.to(dev)
    parameters = list(rpn.parameters())
    rows = []
    for batch in [int(v) for v in args.batches.split(",")]:
        fms = [torch.randn(batch, h, w, CHANNELS, generator=g).to(dev).requires_grad_(True) for h, w in MAP_SIZES]
        match = torch.zeros(batch, anchors, dtype=torch.int32)
        for b in range(batch):
            where = torch.randperm(anchors, generator=g)[:COUNT]
            match[b, where[:COUNT // 2]] = 1
            match[b, where[COUNT // 2:]] = -1
        match = match.to(dev)
        target = (torch.randn(batch, COUNT, 4, generator=g) * 0.5).to(dev)
        index, num, _ = ops.anchor_compact(match, COUNT)
        plain = [f.detach() for f in fms]
        patches = torch.empty(batch * COUNT, 9 * CHANNELS, device=dev)
        dpatch = torch.randn(batch * COUNT, 9 * CHANNELS, generator=g).to(dev)
        grads = [torch.empty_like(f) for f in plain]

        def clear():
            for t in (*fms, *parameters):
                t.grad = None

        def sampled():
            clear()
            out = rpn.losses(fms, match, target)
            (out.rpn_class_loss + out.rpn_bbox_loss).backward()

        def dense():
            clear()
            w_shared = rpn.conv_shared.weight.permute(0, 2, 3, 1).contiguous()
            w_head = torch.cat([rpn.conv_class.weight, rpn.conv_bbox.weight], 0).permute(0, 2, 3, 1).contiguous()
            b_head = torch.cat([rpn.conv_class.bias, rpn.conv_bbox.bias])
            logits, bbox = [], []
            for f in fms:
                h = layers.conv_bn_act(f, w_shared, None, rpn.conv_shared.bias, (1, 1, 1, 1), 1)
                o = layers.conv_bn_act(h, w_head, None, b_head)
                logits.append(o[..., :2 * APL].reshape(batch, -1, 2))
                bbox.append(o[..., 2 * APL:].reshape(batch, -1, 4))
            out = losses.rpn_losses(match, torch.cat(logits, 1), torch.cat(bbox, 1), target)
            (out.rpn_class_loss + out.rpn_bbox_loss).backward()

        def fill():
            for t in grads:
                t.zero_()

        timed = {
            "anchor_compact": lambda: ops.anchor_compact(match, COUNT),
            "pyramid_patch_gather": lambda: ops.pyramid_patch_gather(plain, index, num, APL, out=patches),
            "pyramid_patch_scatter": lambda: ops.pyramid_patch_scatter(dpatch, index, num, MAP_SIZES, CHANNELS, APL, out=grads),
            "fill": fill,
            "sampled_losses_backward": sampled,
            "dense_losses_backward": dense,
        }
        peaks = {k: peak_bytes(timed[k]) for k in ("sampled_losses_backward", "dense_losses_backward")}    # also the warm-up
        for fn in timed.values():
            window_ms(fn)
        torch.cuda.synchronize()
        t = {k: [] for k in timed}
        for _ in range(args.reps):
            for k, fn in timed.items():
                t[k].append(window_ms(fn))
        clear()
        sizes = dict(batch=batch, channels=CHANNELS, hidden=HIDDEN, map_sizes=MAP_SIZES, anchors_per_image=anchors, count=COUNT,
                     gradient_map_bytes=4 * CHANNELS * batch * sum(h * w for h, w in MAP_SIZES), inner=args.inner,
                     device=torch.cuda.get_device_name(0))
        rows += [dict(what=k, **labels, **spread(v), **({"peak_bytes": peaks[k]} if k in peaks else {}), **sizes) for k, v in t.items()]
        del fms, plain, grads, patches, dpatch
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
