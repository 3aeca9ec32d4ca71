#!/usr/bin/env python3
"""Times the backbone's backward (layers.bottleneck, ops.conv_bn_act_backward with a stride, ops.dilate2_sum, ops.maxpool_backward;
csrc/conv_backward.hip, csrc/pool_backward.hip) at the shapes of a 1024 x 1024 image, batch 2. Recorded, not asserted: no ratio is
promised.

    python tools/backbone_backward_microbench.py [--out profiles/backbone_backward_microbench.jsonl] [--reps 9] [--inner 3]
        [--cases a,b] [--label key=value ...]

The cases (synthetic standard-normal operands, everything on the device before the clock starts):
  c3_first / c3_mid   Bottleneck planes 128: [2,256,256,256] at stride 2 with a downsample, and [2,128,128,512]
  c4_first / c4_mid   planes 256: [2,128,128,512] at stride 2, and [2,64,64,1024]
  c5_first / c5_mid   planes 512: [2,64,64,1024] at stride 2, and [2,32,32,2048]
  stem                the weight gradient of the 7x7 stride-2 conv, [2,1024,1024,4] -> 64, and the backward of SamePad2d(3,2) +
                      MaxPool2d(3,2) on [2,512,512,64]
  p6                  the backward of MaxPool2d(1,2) on P5 [2,32,32,256]: ops.dilate2_sum
HIP events go around --inner back-to-back calls after a warm-up, the time of one call is the quotient, and the median of --reps such
windows is reported with the minimum and the maximum; the measurements alternate inside a repetition. Per block:
  backward            the whole block's backward through autograd (dx, four dw, four dshift), the graph retained
  <entry point>       its pieces apart, from the events ops.CONV_PROFILE puts around each launch group, summed over the block's
                      convs at either stride (conv_act_backward, conv_backward_data, conv_backward_weights, dilate2_sum)
  forward             the same block's forward through layers.bottleneck
  aten_convolution_backward   torch.ops.aten.convolution_backward (input, weight and bias gradients) of the block's three or four
                      convs back to back on the same shapes, NCHW, in the same process; a failure is recorded as its reason
For the stem and P6: the op, aten's counterpart (convolution_backward for the weight alone, max_pool2d_with_indices_backward), and
for every dilate2_sum its floor, device_fill: a plain fill of dx. One JSON line per measurement and case. Needs the GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name: (x shape NHWC, planes, stride, downsample)
BLOCKS = {
    "c3_first": ((2, 256, 256, 256), 128, 2, True), "c3_mid": ((2, 128, 128, 512), 128, 1, False),
    "c4_first": ((2, 128, 128, 512), 256, 2, True), "c4_mid": ((2, 64, 64, 1024), 256, 1, False),
    "c5_first": ((2, 64, 64, 1024), 512, 2, True), "c5_mid": ((2, 32, 32, 2048), 512, 1, False),
}
CASES = (*BLOCKS, "stem", "p6")


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backbone_backward_microbench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--label", action="append", default=[], metavar="key=value")
    args = ap.parse_args()
    labels = {k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in (item.split("=", 1) for item in args.label)}
    import torch
    from maskrcnn_amd import layers, ops
    assert torch.cuda.is_available(), "backbone_backward_microbench needs the GPU"
    dev = torch.device("cuda:0")
    device = torch.cuda.get_device_name(0)
    gen = torch.Generator(device="cpu").manual_seed(0)
    randn = lambda *shape: torch.randn(*shape, generator=gen).to(dev)

    def window_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.inner

    def measure(timed, profiled=None):
        """{name: [ms]} of every function in `timed`, alternating inside a repetition; `profiled` is run once more per repetition
        under ops.CONV_PROFILE and its launch groups are summed by tag."""
        usable, errors = {}, {}
        for name, fn in timed.items():
            try:
                window_ms(fn)                                                        # warm-up of every shape
                usable[name] = fn
            except Exception as e:                                                   # recorded: aten's column is a by-product
                if not name.startswith("aten_"):
                    raise
                errors[name] = f"{type(e).__name__}: {e}"[:300]
        torch.cuda.synchronize()
        t = {name: [] for name in usable}
        apart = {}
        for _ in range(args.reps):
            for name, fn in usable.items():
                t[name].append(window_ms(fn))
            if profiled is not None:
                ops.CONV_PROFILE = []
                profiled()
                torch.cuda.synchronize()
                once = {}
                for e0, e1, *booked in ops.CONV_PROFILE:
                    once[booked[3]] = once.get(booked[3], 0.0) + e0.elapsed_time(e1)
                ops.CONV_PROFILE = None
                for tag, ms in once.items():
                    apart.setdefault(tag, []).append(ms)
        t.update(apart)
        return t, errors

    rows = []

    def record(case, sizes, t, errors):
        first = len(rows)
        for what, v in t.items():
            rows.append(dict(case=case, what=what, **labels, **spread(v), **sizes, inner=args.inner, device=device))
        for what, why in errors.items():
            rows.append(dict(case=case, what=what, error=why, **labels, **sizes, device=device))
        for r in rows[first:]:
            print(json.dumps(r), flush=True)

    def aten_conv_backward(x, w, dy, stride, pad, mask):
        xn, wn, dyn = [v.permute(0, 3, 1, 2).contiguous() for v in (x, w, dy)]
        return lambda: torch.ops.aten.convolution_backward(dyn, xn, wn, [w.size(0)], [stride, stride], [pad, pad], [1, 1], False,
                                                           [0, 0], 1, mask)

    for case in args.cases.split(","):
        if case in BLOCKS:
            (b, h, w, cin), planes, stride, down = BLOCKS[case]
            c4 = 4 * planes
            weight = lambda co, k, ci: (randn(co, k, k, ci) * (k * k * ci) ** -0.5).requires_grad_(True)
            affine = lambda c: ((torch.rand(c, generator=gen) + 0.5).to(dev), randn(c).requires_grad_(True))
            x = randn(b, h, w, cin).requires_grad_(True)
            w1, w2, w3 = weight(planes, 1, cin), weight(planes, 3, planes), weight(c4, 1, planes)
            (s1, t1), (s2, t2), (s3, t3) = affine(planes), affine(planes), affine(c4)
            wd, (sd, td) = (weight(c4, 1, cin), affine(c4)) if down else (None, (None, None))
            params = (w1, s1, t1, w2, s2, t2, w3, s3, t3, wd, sd, td)

            def forward():
                return layers.bottleneck(x, *params, stride=stride)

            y = forward()
            dy = randn(*y.shape)
            wanted = [v for v in (x, w1, t1, w2, t2, w3, t3, wd, td) if v is not None]

            def backward():
                return torch.autograd.grad(y, wanted, dy, retain_graph=True)

            oh, ow = y.size(1), y.size(2)
            h1, h2 = randn(b, oh, ow, planes), randn(b, oh, ow, planes)
            every = [True, True, True]
            convs = [aten_conv_backward(h2, w3.detach(), dy, 1, 0, every), aten_conv_backward(h1, w2.detach(), h2, 1, 1, every),
                     aten_conv_backward(x.detach(), w1.detach(), h1, stride, 0, every)]
            if down:
                convs.append(aten_conv_backward(x.detach(), wd.detach(), dy, stride, 0, every))
            timed = {"backward": backward, "forward": forward, "aten_convolution_backward": lambda: [f() for f in convs]}
            if stride == 2:
                full = torch.empty(b, h, w, cin, device=dev)
                a, a2 = randn(b, oh, ow, cin), randn(b, oh, ow, cin)
                timed["dilate2_sum_two_operands"] = lambda: ops.dilate2_sum(a, a2, h, w, out=full)
                timed["device_fill"] = lambda: full.fill_(0.0)
            t, errors = measure(timed, backward)
            flops = 2.0 * b * oh * ow * (planes * cin + 9 * planes * planes + c4 * planes + (c4 * cin if down else 0))
            sizes = dict(x_shape=[b, h, w, cin], planes=planes, stride=stride, downsample=down, forward_gflop=round(flops / 1e9, 3),
                         chunk_conv1=ops.conv_backward_chunk(b, h, w, cin, planes, 1, 1, stride=stride))
            record(case, sizes, t, errors)
            del x, y, dy, params, wanted, convs, timed, h1, h2
        elif case == "stem":
            b, h, w = 2, 1024, 1024
            x, wt = randn(b, h, w, 4), randn(64, 7, 7, 4) * 196 ** -0.5
            scale, shift = (torch.rand(64, generator=gen) + 0.5).to(dev), randn(64)
            pad = (3, 3, 3, 3)
            y = ops.conv_bn_act(x, wt, scale, shift, 2, pad, True)
            dy = randn(*y.shape)
            timed = {"conv_backward_dw_dshift": lambda: ops.conv_bn_act_backward(dy, x, wt, y, scale, pad, 1, needs=(False, True, True, False),
                                                                                  stride=2),
                     "forward": lambda: ops.conv_bn_act(x, wt, scale, shift, 2, pad, True),
                     "aten_convolution_backward": aten_conv_backward(x, wt, dy, 2, 3, [False, True, True])}
            t, errors = measure(timed, timed["conv_backward_dw_dshift"])
            chunk = ops.conv_backward_chunk(b, h, w, 4, 64, 7, 7, pad, stride=2)
            record("stem_conv", dict(x_shape=[b, h, w, 4], cout=64, kernel=7, stride=2, chunk=chunk,
                                     chunks=-(-y.numel() // 64 // chunk)), t, errors)
            ppad = ops.same_pad(y.size(1), y.size(2), 3, 2)
            pooled = ops.maxpool(y, 3, 2, ppad)
            dp = randn(*pooled.shape)
            yn = torch.nn.functional.pad(y.permute(0, 3, 1, 2), (ppad[1], ppad[3], ppad[0], ppad[2])).contiguous()
            _, idx = torch.nn.functional.max_pool2d(yn, 3, 2, return_indices=True)
            dpn = dp.permute(0, 3, 1, 2).contiguous()
            timed = {"maxpool_backward": lambda: ops.maxpool_backward(dp, y, 3, 2, ppad),
                     "forward": lambda: ops.maxpool(y, 3, 2, ppad),
                     "aten_max_pool2d_with_indices_backward": lambda: torch.ops.aten.max_pool2d_with_indices_backward(
                         dpn, yn, [3, 3], [2, 2], [0, 0], [1, 1], False, idx)}
            t, errors = measure(timed)
            record("stem_pool", dict(x_shape=list(y.shape), kernel=3, stride=2, pad=list(ppad)), t, errors)
            del x, y, dy, yn, idx, dpn, pooled, dp, timed
        elif case == "p6":
            b, h, w, c = 2, 32, 32, 256
            p5, dp = randn(b, h, w, c), randn(b, h // 2, w // 2, c)
            full = torch.empty(b, h, w, c, device=dev)
            p5n, dpn = p5.permute(0, 3, 1, 2).contiguous(), dp.permute(0, 3, 1, 2).contiguous()
            _, idx = torch.nn.functional.max_pool2d(p5n, 1, 2, return_indices=True)
            timed = {"dilate2_sum": lambda: ops.dilate2_sum(dp, None, h, w, out=full), "device_fill": lambda: full.fill_(0.0),
                     "forward": lambda: ops.maxpool(p5, 1, 2),
                     "aten_max_pool2d_with_indices_backward": lambda: torch.ops.aten.max_pool2d_with_indices_backward(
                         dpn, p5n, [1, 1], [2, 2], [0, 0], [1, 1], False, idx)}
            t, errors = measure(timed)
            record("p6", dict(x_shape=[b, h, w, c], kernel=1, stride=2), t, errors)
        else:
            raise SystemExit(f"unknown case {case!r}: one of {', '.join(CASES)}")
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
