#!/usr/bin/env python3
"""Times the clipped SGD (csrc/optim.hip through maskrcnn_amd.optim.ClippedSGD) on the parameters the reference's first schedule
trains. Recorded, not asserted: no ratio is promised.

    python tools/optim_microbench.py [--out profiles/optim_microbench.jsonl] [--reps 9] [--inner 10]

The workload: the parameters of the reference's state-dict layout for ResNet-50-FPN with 81 classes (modules.reference_schema) whose
names the "heads" regex of train_model (model.py:1512) matches in full, in the reference's two groups (model.py:1542-1557): weight
decay 1e-4 on the names without 'bn', none on the others; lr 0.001, momentum 0.9, max_norm 5; seeded gradients of unit scale.
Everything is on the device before the clock starts. HIP events go around --inner back-to-back calls after a warm-up, the time of one
call is the quotient (the gradients are refilled before each window, outside the clock, so that every call clips), and the median
of --reps such windows is reported with the minimum and the maximum:
  clip / step / step_zero      ClippedSGD.clip_(), .step() and .step(zero_grad=True): the pointer check of the front end and the three
                               launches (clip: two and one that writes the gradients) are inside the clock
  torch_default / torch_fused  for context, in the same process on copies of the same tensors: clip_grad_norm_(params, 5) +
                               torch.optim.SGD(the two groups).step() + zero_grad(set_to_none=False), with torch's default
                               implementation and with fused=True (recorded as absent where this torch refuses fused=True)
  torch_clip                   clip_grad_norm_ alone
  copy_28B                     a device-to-device copy of 28 bytes per element (14 read, 14 written): the traffic of step_zero's floor
                               (g read twice, p and b read, p, b and g written) as one plain copy
One JSON line per measurement. Needs the GPU."""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HEADS = r"(fpn.P5\_.*)|(fpn.P4\_.*)|(fpn.P3\_.*)|(fpn.P2\_.*)|(rpn.*)|(classifier.*)|(mask.*)"      # model.py:1512
LR, MOMENTUM, WEIGHT_DECAY, MAX_NORM = 0.001, 0.9, 1e-4, 5.0


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def heads_parameters(torch, dev, seed=20261020):
    """[(name, Parameter with a gradient)] of the heads schedule on dev, and the two groups' index lists."""
    from maskrcnn_amd import modules
    gen = torch.Generator().manual_seed(seed)
    named = [(n, p) for n, p in modules.reference_schema("resnet50").named_parameters() if re.fullmatch(HEADS, n)]
    out = []
    for name, p in named:
        q = torch.nn.Parameter(torch.randn(p.shape, generator=gen).mul_(0.05).to(dev))
        q.grad = torch.randn(p.shape, generator=gen).to(dev)
        out.append((name, q))
    return out


def groups(named, params):
    return [{"params": [q for (n, _), q in zip(named, params) if "bn" not in n], "weight_decay": WEIGHT_DECAY},
            {"params": [q for (n, _), q in zip(named, params) if "bn" in n]}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_microbench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    import torch
    from maskrcnn_amd import optim
    assert torch.cuda.is_available(), "optim_microbench needs the GPU"
    dev = torch.device("cuda:0")
    named = heads_parameters(torch, dev)
    elements = sum(q.numel() for _, q in named)

    def copies():
        ps = []
        for _, q in named:
            c = torch.nn.Parameter(q.detach().clone())
            c.grad = q.grad.clone()
            ps.append(c)
        return ps

    def window_ms(fn):
        refill()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.inner

    ours_p = copies()
    saved = [q.grad.clone() for q in ours_p]

    def refill():
        """The gradients of the ClippedSGD copy as they were, before every window and outside the clock: a window that zeroed them
        would leave the next one c == 1, whose store of the unchanged gradient is left out. (Within a window the clipped norm stays
        a hair under max_norm, and norm + 1e-6 above it: c < 1 in every call.)"""
        torch._foreach_copy_([q.grad for q in ours_p], saved)

    ours = optim.ClippedSGD(groups(named, ours_p), lr=LR, momentum=MOMENTUM, max_norm=MAX_NORM)
    timed = {"clip": ours.clip_, "step": ours.step, "step_zero": lambda: ours.step(zero_grad=True)}
    notes = {}
    for tag, extra in (("torch_default", {}), ("torch_fused", {"fused": True})):
        ps = copies()
        try:
            sgd = torch.optim.SGD(groups(named, ps), lr=LR, momentum=MOMENTUM, **extra)
        except (RuntimeError, ValueError, TypeError) as e:
            notes[tag] = f"refused: {e}"
            continue

        def stock(ps=ps, sgd=sgd):
            torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
            sgd.step()
            sgd.zero_grad(set_to_none=False)

        timed[tag] = stock
    clip_p = copies()
    timed["torch_clip"] = lambda: torch.nn.utils.clip_grad_norm_(clip_p, MAX_NORM)
    src, dst = torch.empty(14 * elements, dtype=torch.uint8, device=dev), torch.empty(14 * elements, dtype=torch.uint8, device=dev)
    timed["copy_28B"] = lambda: dst.copy_(src)

    for fn in timed.values():                                                   # warm-up: the table upload, torch's own caches
        window_ms(fn)
    torch.cuda.synchronize()
    t = {k: [] for k in timed}
    for _ in range(args.reps):
        for k, fn in timed.items():
            t[k].append(window_ms(fn))
    assert ours.status.tolist() == [0]
    sizes = dict(tensors=len(named), elements=elements, tiles=ours._device_table[3], tile=optim.TILE,
                 decay_tensors=len(groups(named, ours_p)[0]["params"]), inner=args.inner, torch=torch.__version__,
                 device=torch.cuda.get_device_name(0))
    rows = [dict(what=k, **spread(v), **sizes) for k, v in t.items()] + [dict(what=k, note=v, **sizes) for k, v in notes.items()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
