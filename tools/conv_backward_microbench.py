#!/usr/bin/env python3
"""Times the conv backward (ops.conv_bn_act_backward, csrc/conv_backward.hip) on four head layers of a training step. Recorded, not
asserted: no ratio is promised.

    python tools/conv_backward_microbench.py [--out profiles/conv_backward_microbench.jsonl] [--reps 9] [--inner 3] [--layers a,b]
        [--label key=value ...]   extra fields for every line: what tells two builds apart (MRCNN_LIB=<variant> ... --label tile=64)

The layers (synthetic standard-normal operands, everything on the device before the clock starts):
  mask_conv1        3x3 SAME, 256 -> 256 on [800,14,14], BN affine + ReLU
  rpn_shared        3x3 SAME, 256 -> 512 on [2,256,256], bias + ReLU
  classifier_conv1  the 7x7 conv as a GEMM: [800,1,1,12544] -> 1024, BN affine + ReLU
  fc_405            the joined linear_class + linear_bbox: [800,1,1,1024] -> 405
HIP events go around --inner back-to-back calls after a warm-up, the time of one call is the quotient, and the median of --reps such
windows is reported with the minimum and the maximum; the measurements alternate inside a repetition. Per layer:
  backward            the whole op (dx, dw, dshift): six launches
  conv_act_backward / conv_backward_data / conv_backward_weights
                      the three entry points apart, from the events ops.CONV_PROFILE puts around each (their own --reps runs)
  forward             the same layer's forward by ops.conv_bn_act: the same flops as the weight gradient and as the data gradient,
                      so this is the yardstick for conv_backward_weights
  aten_convolution_backward   torch.ops.aten.convolution_backward (input, weight and bias gradients) on the same shapes, NCHW, in
                      the same process; a failure is recorded as its reason
tflops and mfma_peak_share are the algorithmic 2 * M * K * Cout against the time and the 157.3 TF fp32-MFMA peak. One JSON line
per measurement and layer. Needs the GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_TFLOPS = 157.3
# name: (x shape NHWC, Cout, kernel, pad, act, scale?)
LAYERS = {
    "mask_conv1": ((800, 14, 14, 256), 256, 3, 1, 1, True),
    "rpn_shared": ((2, 256, 256, 256), 512, 3, 1, 1, False),
    "classifier_conv1": ((800, 1, 1, 12544), 1024, 1, 0, 1, True),
    "fc_405": ((800, 1, 1, 1024), 405, 1, 0, 0, False),
}


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_backward_microbench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--layers", default=",".join(LAYERS))
    ap.add_argument("--label", action="append", default=[], metavar="key=value")
    args = ap.parse_args()
    labels = {k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in (item.split("=", 1) for item in args.label)}
    import torch
    from maskrcnn_amd import ops
    assert torch.cuda.is_available(), "conv_backward_microbench needs the GPU"
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
    for name in args.layers.split(","):
        (b, h, w, cin), cout, k, p, act, with_scale = LAYERS[name]
        pad = (p, p, p, p)
        g = torch.Generator(device="cpu").manual_seed(len(name))
        x = torch.randn(b, h, w, cin, generator=g).to(dev)
        wt = (torch.randn(cout, k, k, cin, generator=g) * (k * k * cin) ** -0.5).to(dev)
        scale = (torch.rand(cout, generator=g) + 0.5).to(dev) if with_scale else None
        shift = torch.randn(cout, generator=g).to(dev)
        y = ops.conv_bn_act(x, wt, scale, shift, 1, pad, act)
        dy = torch.randn(y.shape, generator=g).to(dev)
        m, kk = y.numel() // cout, k * k * cin
        flops = 2.0 * m * kk * cout
        chunk = ops.conv_backward_chunk(b, h, w, cin, cout, k, k, pad)

        def backward():
            return ops.conv_bn_act_backward(dy, x, wt, y, scale, pad, act, needs=(True, True, True, False))

        def forward():
            return ops.conv_bn_act(x, wt, scale, shift, 1, pad, act)

        timed = {"backward": backward, "forward": forward}
        aten_error = None
        try:
            xn, wn = x.permute(0, 3, 1, 2).contiguous(), wt.permute(0, 3, 1, 2).contiguous()
            dyn = dy.permute(0, 3, 1, 2).contiguous()

            def aten():
                return torch.ops.aten.convolution_backward(dyn, xn, wn, [cout], [1, 1], [p, p], [1, 1], False, [0, 0], 1,
                                                           [True, True, True])
            aten()
            torch.cuda.synchronize()
            timed["aten_convolution_backward"] = aten
        except Exception as e:   # recorded: the comparison is a by-product
            aten_error = f"{type(e).__name__}: {e}"[:300]
        for fn in timed.values():                                                     # warm-up of every shape
            window_ms(fn)
        torch.cuda.synchronize()
        t = {k_: [] for k_ in timed}
        apart = {}
        for _ in range(args.reps):
            for k_, fn in timed.items():
                t[k_].append(window_ms(fn))
            ops.CONV_PROFILE = []
            backward()
            torch.cuda.synchronize()
            for e0, e1, *booked in ops.CONV_PROFILE:
                apart.setdefault(booked[3], []).append(e0.elapsed_time(e1))
            ops.CONV_PROFILE = None
        t.update(apart)
        sizes = dict(layer=name, x_shape=[b, h, w, cin], cout=cout, kernel=k, pad=p, activation=act, scale=with_scale, pixels=m,
                     gemm_k=kk, chunk=chunk, chunks=-(-m // chunk), algorithmic_gflop=round(flops / 1e9, 3), inner=args.inner,
                     device=torch.cuda.get_device_name(0))
        for k_, v in t.items():
            row = dict(what=k_, **labels, **spread(v), **sizes)
            units = {"backward": 2, "aten_convolution_backward": 2, "conv_act_backward": 0}.get(k_, 1)   # GEMMs of `flops` each
            if units:
                row["tflops"] = round(units * flops / (row["median_ms"] * 1e-3) / 1e12, 2)
                row["mfma_peak_share"] = round(row["tflops"] / PEAK_TFLOPS, 4)
            rows.append(row)
        if aten_error:
            rows.append(dict(what="aten_convolution_backward", error=aten_error, **labels, **sizes))
        del x, wt, y, dy
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
