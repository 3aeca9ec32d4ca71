#!/usr/bin/env python3
"""Times the training-loss kernels (csrc/losses.hip): ops.rpn_loss / ops.rpn_loss_backward, ops.head_loss / ops.head_loss_backward and
the front ends losses.rpn_losses / losses.head_losses with .backward(). Recorded, not asserted: no ratio is promised.

    python tools/losses_microbench.py [--out profiles/losses_microbench.jsonl] [--reps 9] [--inner 10] [--batches 1,8,16]

The workload is synthetic and seeded: B images of 261 888 anchors with 64 positives and 64 negatives each and 128 target rows; 100
slots per image, all of them sampled, 33 positive, 81 classes, 28 x 28 masks. Everything is on the device before the clock starts.
HIP events go around --inner back-to-back calls after a warm-up, the time of one call is the quotient, and the median of --reps such
windows is reported with the minimum and the maximum. Per family (rpn, head) and batch size:
  <family>_forward / <family>_backward      the two ops, the second fed with the first's counts and an upstream gradient of ones
  <family>_forward_backward                 the front end and .backward() on leaf predictions: autograd's bookkeeping and the
                                            fp64 quotient on the device are inside the clock
  torch_<family>_forward / _backward / _forward_backward
                                            for context, in the same process on the same GPU: the same losses composed from stock
                                            torch ops the way the reference composes them — torch.nonzero (a host read-back),
                                            advanced-index gathers, F.cross_entropy / F.smooth_l1_loss / F.binary_cross_entropy on
                                            the concatenation of the images — and autograd's backward of that. It is float32
                                            arithmetic, so its values agree with the kernels' to float32 rounding only (asserted
                                            loosely before timing).
One JSON line per measurement and batch size. Needs the GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ANCHORS, RPN_COUNT, POSITIVES, NEGATIVES = 261888, 128, 64, 64
COUNT, CLASSES, MASK, HEAD_POSITIVES = 100, 81, (28, 28), 33


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def workload(np, torch, batch, dev, seed=20261021):
    rng = np.random.default_rng(seed + batch)
    f32 = lambda lo, hi, *shape: torch.from_numpy((lo + (hi - lo) * rng.random(shape, dtype=np.float32)).astype(np.float32)).to(dev)
    match = np.zeros((batch, ANCHORS), np.int32)
    ids = np.zeros((batch, COUNT), np.int32)
    for b in range(batch):
        pick = rng.permutation(ANCHORS)[:POSITIVES + NEGATIVES]
        match[b, pick[:POSITIVES]], match[b, pick[POSITIVES:]] = 1, -1
        ids[b, :HEAD_POSITIVES] = rng.integers(1, CLASSES, HEAD_POSITIVES)
    rpn = (torch.from_numpy(match).to(dev), f32(-8, 8, batch, ANCHORS, 2), f32(-8, 8, batch, ANCHORS, 4), f32(-8, 8, batch, RPN_COUNT, 4))
    rpn[3][:, POSITIVES:] = 0
    head = (torch.from_numpy(ids).to(dev), torch.full((batch,), COUNT, dtype=torch.int32, device=dev), f32(-8, 8, batch, COUNT, 4),
            (f32(0, 1, batch, COUNT, *MASK) < 0.5).float(), f32(-8, 8, batch, COUNT, CLASSES), f32(-8, 8, batch, COUNT, CLASSES, 4),
            f32(0.01, 0.99, batch, COUNT, CLASSES, *MASK))
    return rpn, head


def torch_rpn(torch, F, match, logits, pred, target):
    """The two RPN losses from stock ops, over the concatenation of the images."""
    idx = torch.nonzero(match != 0)
    cls = F.cross_entropy(logits[idx[:, 0], idx[:, 1]], (match[idx[:, 0], idx[:, 1]] == 1).long())
    pos = torch.nonzero(match == 1)
    rank = torch.cumsum(match == 1, dim=1)[pos[:, 0], pos[:, 1]] - 1                 # the k-th positive of its image
    keep = rank < target.size(1)
    pos, rank = pos[keep], rank[keep]
    return cls, F.smooth_l1_loss(pred[pos[:, 0], pos[:, 1]], target[pos[:, 0], rank])


def torch_head(torch, F, ids, num_rois, deltas, mask, logits, pred_bbox, pred_masks):
    """The three head losses from stock ops, over the concatenation of the images' sampled slots."""
    valid = torch.arange(ids.size(1), device=ids.device)[None, :] < num_rois[:, None]
    use = torch.nonzero(valid)
    cls = F.cross_entropy(logits[use[:, 0], use[:, 1]], ids[use[:, 0], use[:, 1]].long())
    pos = torch.nonzero(valid & (ids > 0))
    c = ids[pos[:, 0], pos[:, 1]].long()
    box = F.smooth_l1_loss(pred_bbox[pos[:, 0], pos[:, 1], c], deltas[pos[:, 0], pos[:, 1]])
    return cls, box, F.binary_cross_entropy(pred_masks[pos[:, 0], pos[:, 1], c], mask[pos[:, 0], pos[:, 1]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "losses_microbench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batches", type=lambda s: [int(v) for v in s.split(",")], default=[1, 8, 16])
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from maskrcnn_amd import losses, ops
    assert torch.cuda.is_available(), "losses_microbench needs the GPU"
    dev = torch.device("cuda:0")

    def window_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.inner

    rows = []
    for batch in args.batches:
        rpn, head = workload(np, torch, batch, dev)
        families = {}
        for family, inputs, n_pred, forward, backward, front, stock in (
                ("rpn", rpn, 2, ops.rpn_loss, ops.rpn_loss_backward,
                 lambda m, t, *preds: losses.rpn_losses(m, *preds, t)[:2], lambda m, t, *preds: torch_rpn(torch, F, m, *preds, t)),
                ("head", head, 3, ops.head_loss, ops.head_loss_backward,
                 lambda *a: losses.head_losses(*a)[:3], lambda *a: torch_head(torch, F, *a))):
            if family == "rpn":
                targets, preds = (inputs[0], inputs[3]), [inputs[1], inputs[2]]
            else:
                targets, preds = inputs[:4], list(inputs[4:])
            first = forward(*inputs)
            grad_out = torch.ones(n_pred, dtype=torch.float32, device=dev)
            leaves = [p.clone().requires_grad_(True) for p in preds]

            def both(compose):
                for p in leaves:
                    p.grad = None
                sum(compose(*targets, *leaves)).backward()

            def backward_only(compose):
                """.backward() alone: the graph is rebuilt outside the window (the window then holds `inner` backward calls)."""
                totals = [sum(compose(*targets, *leaves)) for _ in range(args.inner)]
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for t in totals:
                    for p in leaves:
                        p.grad = None
                    t.backward()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / args.inner

            with torch.no_grad():
                ours, theirs = front(*targets, *preds), stock(*targets, *preds)
            for a, b in zip(ours, theirs):
                assert abs(float(a) - float(b)) <= 1e-4 * max(1.0, abs(float(b))), (family, float(a), float(b))
            timed = {
                f"{family}_forward": lambda: window_ms(lambda: forward(*inputs)),
                f"{family}_backward": lambda: window_ms(lambda: backward(*inputs, *first[3:], first[1], grad_out)),
                f"{family}_forward_backward": lambda: window_ms(lambda: both(front)),
                f"torch_{family}_forward": lambda: window_ms(lambda: stock(*targets, *preds)),
                f"torch_{family}_backward": lambda: backward_only(stock),
                f"torch_{family}_forward_backward": lambda: window_ms(lambda: both(stock)),
            }
            for fn in timed.values():                                                   # warm-up of every shape
                fn()
            torch.cuda.synchronize()
            t = {k: [] for k in timed}
            for _ in range(args.reps):
                for k, fn in timed.items():
                    t[k].append(fn())
            families.update(t)
        sizes = dict(batch=batch, anchors=ANCHORS, rpn_count=RPN_COUNT, positives=POSITIVES, negatives=NEGATIVES, count=COUNT,
                     classes=CLASSES, mask_shape=list(MASK), head_positives=HEAD_POSITIVES, inner=args.inner,
                     device=torch.cuda.get_device_name(0))
        rows += [dict(what=k, **spread(v), **sizes) for k, v in families.items()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
