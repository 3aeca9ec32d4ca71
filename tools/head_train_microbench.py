#!/usr/bin/env python3
"""Times the heads' training mode (csrc/mask_train.hip, maskrcnn_amd/head_train.py) beside the dense route it replaces, at a training
step's shapes. Recorded, not asserted: no ratio is promised.

    python tools/head_train_microbench.py [--out profiles/head_train_microbench.jsonl] [--reps 9] [--inner 3] [--batches 2,8]
        [--label key=value ...]   extra fields for every line: what tells two builds apart

The workload is synthetic and seeded: images of 1024 x 1024, maps 256^2 .. 32^2 x 256 (P2 .. P5), count = 100 slots per image of which 33
are positives of random classes among 81 and 67 negatives, P = 33 plane slots, 28 x 28 planes. Everything is on the device before the
clock starts. HIP events go around --inner back-to-back calls after a warm-up of every shape, the time of one call is the quotient, and the
median of --reps such windows is reported with the minimum and the maximum; the measurements alternate inside a repetition. Per batch:
  class_plane_conv, class_plane_conv_backward, mask_plane_loss, mask_plane_loss_backward   the four ops, outputs preallocated where the
                         binding takes them
  copy_x, copy_x_dx      a plain device copy of the traffic of the conv's forward (x once: half of x copied) and backward (x read, dx
                         written: all of x copied): their floor
  mask_losses_backward   TrainableMask.losses(...) with .backward()
  heads_losses_backward  TrainableHeads.losses(...) with .backward(): gradients into the four maps and every head parameter
  dense_losses_backward  the same three losses by the dense route the tests use, in the same process: RoIAlign and layers over all count
                         slots, conv5 to all 81 planes, losses.head_losses, .backward()
The peak of torch's allocator over one call (beyond what was allocated before it) stands beside the three routes as peak_bytes.
One JSON line per measurement and batch. Needs the GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEPTH, HIDDEN, CLASSES, COUNT, SLOTS, SIDE = 256, 1024, 81, 100, 33, 28
MAP_SIZES = [(256, 256), (128, 128), (64, 64), (32, 32)]
AREA = 1024.0 * 1024.0


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_train_microbench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--batches", default="2,8")
    ap.add_argument("--label", action="append", default=[], metavar="key=value")
    args = ap.parse_args()
    labels = {k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in (item.split("=", 1) for item in args.label)}
    import torch
    from maskrcnn_amd import layers, losses, modules, ops
    from maskrcnn_amd.head_train import TrainableClassifier, TrainableHeads, TrainableMask
    from maskrcnn_amd.targets import DetectionTargets
    assert torch.cuda.is_available(), "head_train_microbench needs the GPU"
    dev = torch.device("cuda:0")

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
    heads = TrainableHeads(TrainableClassifier(DEPTH, 7, CLASSES, HIDDEN, AREA), TrainableMask(DEPTH, 14, CLASSES, AREA, SLOTS))
    with torch.no_grad():
        for n, p in heads.named_parameters():
            if ".bn" not in n:
                p.copy_(torch.randn(p.shape, generator=g) * (0.02 if p.dim() > 1 else 0.1))
    heads.to(dev)
    cls, mask = heads.classifier, heads.mask
    parameters = [p for p in heads.parameters() if p.requires_grad]
    ohwi = lambda w: w.permute(0, 2, 3, 1).contiguous()
    rows = []
    for batch in [int(v) for v in args.batches.split(",")]:
        fms = [torch.randn(batch, h, w, DEPTH, generator=g).to(dev).requires_grad_(True) for h, w in MAP_SIZES]
        side = 0.03 + 0.4 * torch.rand(batch, COUNT, 1, generator=g)
        centre = 0.25 + 0.5 * torch.rand(batch, COUNT, 2, generator=g)
        rois = torch.cat([centre - side / 2, centre + side / 2], 2)
        ids = torch.zeros(batch, COUNT, dtype=torch.int32)
        ids[:, :SLOTS] = torch.randint(1, CLASSES, (batch, SLOTS), generator=g).to(torch.int32)
        target_mask = torch.zeros(batch, COUNT, SIDE, SIDE)
        target_mask[:, :SLOTS] = (torch.rand(batch, SLOTS, SIDE, SIDE, generator=g) < 0.5).float()
        minus = torch.full((batch, COUNT), -1, dtype=torch.int32)
        t = DetectionTargets(*[v.to(dev) for v in (rois, ids, torch.randn(batch, COUNT, 4, generator=g) * 0.5, target_mask, minus, minus,
                                                   torch.full((batch,), SLOTS, dtype=torch.int32), torch.full((batch,), COUNT - SLOTS, dtype=torch.int32),
                                                   torch.zeros(batch, dtype=torch.int32))])
        num = t.num_pos + t.num_neg
        s = batch * SLOTS
        x = torch.randn(s, SIDE, SIDE, DEPTH, generator=g).to(dev)
        w5 = mask.conv5.weight.detach().view(CLASSES, DEPTH).contiguous()
        b5 = mask.conv5.bias.detach()
        y = torch.empty(s, SIDE, SIDE, device=dev)
        p, _ = ops.class_plane_conv(x, w5, b5, t.target_class_ids, num, 2)
        dy = torch.randn(s, SIDE, SIDE, generator=g).to(dev)
        outs = (torch.empty_like(x), torch.empty_like(w5), torch.empty_like(b5))
        planes = p.view(batch, SLOTS, SIDE, SIDE)
        _, counts, _ = ops.mask_plane_loss(planes, t.target_mask, t.target_class_ids, num, CLASSES)
        one = torch.ones(1, device=dev)
        grad_p = torch.empty_like(planes)
        x_copy = torch.empty_like(x)

        def clear():
            for v in (*fms, *parameters):
                v.grad = None

        def mask_route():
            clear()
            loss, _ = mask.losses(fms, t)
            loss.backward()

        def heads_route():
            clear()
            out = heads.losses(fms, t)
            (out.class_loss + out.bbox_loss + out.mask_loss).backward()

        def dense_route():
            clear()
            sd = {**{"classifier." + n: v for n, v in cls._state().items()}, **{"mask." + n: v for n, v in mask._state().items()}}
            r = batch * COUNT
            flat = t.rois.reshape(r, 4)
            pooled = ops.roi_align_pyramid(fms, flat, 7, AREA, rois_per_image=COUNT)
            s1, t1 = modules.fold_bn(sd, "classifier.conv1", "classifier.bn1", dev)
            s2, t2 = modules.fold_bn(sd, "classifier.conv2", "classifier.bn2", dev)
            h = layers.conv_bn_act(pooled.reshape(r, 1, 1, -1), ohwi(cls.conv1.weight).reshape(HIDDEN, 1, 1, -1), s1, t1, act=1)
            h = layers.conv_bn_act(h, ohwi(cls.conv2.weight), s2, t2, act=1)
            w_fc = torch.cat([cls.linear_class.weight, cls.linear_bbox.weight], 0).view(5 * CLASSES, 1, 1, HIDDEN)
            out = layers.conv_bn_act(h, w_fc, None, torch.cat([cls.linear_class.bias, cls.linear_bbox.bias])).view(r, 5 * CLASSES)
            v = ops.roi_align_pyramid(fms, flat, 14, AREA, rois_per_image=COUNT)
            for i in (1, 2, 3, 4):
                sc, sh = modules.fold_bn(sd, f"mask.conv{i}", f"mask.bn{i}", dev)
                v = layers.conv_bn_act(v, ohwi(getattr(mask, f"conv{i}").weight), sc, sh, (1, 1, 1, 1), 1)
            w4 = mask.deconv.weight.permute(2, 3, 1, 0).reshape(4 * DEPTH, 1, 1, DEPTH).contiguous()
            v = layers.deconv2x2(v, w4, mask.deconv.bias.repeat(4), 1)
            m = layers.conv_bn_act(v, ohwi(mask.conv5.weight), None, mask.conv5.bias, act=2)
            masks = m.permute(0, 3, 1, 2).reshape(batch, COUNT, CLASSES, SIDE, SIDE)
            got = losses.head_losses(t, out[:, :CLASSES].reshape(batch, COUNT, CLASSES), out[:, CLASSES:].reshape(batch, COUNT, CLASSES, 4), masks)
            (got.class_loss + got.bbox_loss + got.mask_loss).backward()

        def copy_x_dx():
            outs[0].copy_(x)

        timed = {
            "class_plane_conv": lambda: ops.class_plane_conv(x, w5, b5, t.target_class_ids, num, 2, out=y),
            "copy_x": lambda: x_copy[:s // 2].copy_(x[:s // 2]),   # half of x read, as much written: the bytes of one read of x
            "class_plane_conv_backward": lambda: ops.class_plane_conv_backward(dy, p, x, w5, t.target_class_ids, num, 2, out=outs),
            "copy_x_dx": copy_x_dx,
            "mask_plane_loss": lambda: ops.mask_plane_loss(planes, t.target_mask, t.target_class_ids, num, CLASSES),
            "mask_plane_loss_backward": lambda: ops.mask_plane_loss_backward(planes, t.target_mask, t.target_class_ids, num, CLASSES, counts, one,
                                                                             out=grad_p),
            "mask_losses_backward": mask_route,
            "heads_losses_backward": heads_route,
            "dense_losses_backward": dense_route,
        }
        routes = ("mask_losses_backward", "heads_losses_backward", "dense_losses_backward")
        peaks = {}
        for k in routes:                                      # also the warm-up; the gradients of the route before are freed first
            clear()
            peaks[k] = peak_bytes(timed[k])
        for fn in timed.values():
            window_ms(fn)
        torch.cuda.synchronize()
        ms = {k: [] for k in timed}
        for _ in range(args.reps):
            for k, fn in timed.items():
                ms[k].append(window_ms(fn))
        clear()
        sizes = dict(batch=batch, depth=DEPTH, classes=CLASSES, count=COUNT, plane_slots=SLOTS, positives_per_image=SLOTS, plane_side=SIDE,
                     map_sizes=MAP_SIZES, x_bytes=4 * x.numel(), inner=args.inner, device=torch.cuda.get_device_name(0))
        rows += [dict(what=k, **labels, **spread(v), **({"peak_bytes": peaks[k]} if k in peaks else {}), **sizes) for k, v in ms.items()]
        del fms, x, x_copy, outs, p, planes, grad_p, dy, y
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
