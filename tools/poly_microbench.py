#!/usr/bin/env python3
"""Times the polygon rasterisation kernels, ops.rle_from_poly and ops.rle_merge (csrc/poly.hip). Recorded, not asserted: there is
no earlier implementation here to regress against, and the reference's C codec is not available where the GPU is, so no ratio is
claimed.

    python tools/poly_microbench.py [--out profiles/poly_microbench.jsonl] [--reps 9] [--annotations 40000]

The workload is synthetic and seeded (no fixture is involved): --annotations annotations on 480 x 640 images, 1-4 polygon parts
each, 10-60 vertices per part (star-shaped rings of radius 5-120 pixels around a centre inside the image, coordinates with two
decimals). The arguments are on the device before the clock starts and the capacities are given, so neither call synchronises:
  rle_from_poly   all parts in ONE call                          HIP events around the call, after a warm-up call
  rle_merge       all annotations in ONE call on its output      likewise
  both            their sum per repetition
One JSON line per measurement (median, min, max over the repetitions, in ms) with the sizes of the workload. Needs the GPU.

    python tools/poly_microbench.py --codec-source <cocoapi>/common/maskApi.c [--out ...]

For context only, and without a GPU: compiles that C file (cc -O2) into a temporary directory, runs rleFrPoly on every part and
rleMerge on every annotation of the SAME workload through ctypes, one after the other as COCO.annToRLE does, and APPENDS one line,
what = "reference_codec_cpu", wall clock of the whole loop (the ctypes call overhead included), labelled with the CPU it ran on.
It is a different machine from the GPU lines' unless the file says otherwise; no ratio is claimed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def workload(np, annotations, seed=20250715, h=480, w=640):
    rng = np.random.default_rng(seed)
    parts_per = rng.integers(1, 5, annotations)
    n = int(parts_per.sum())
    ks = rng.integers(10, 61, n)
    off = np.concatenate([[0], np.cumsum(ks)])
    part = np.repeat(np.arange(n), ks)
    ang = rng.uniform(0, 2 * np.pi, int(off[-1]))
    ang = ang[np.lexsort((ang, part))]                         # sorted within each part: a star-shaped ring
    r = (rng.uniform(5, 120, n)[part]) * rng.uniform(0.6, 1.0, int(off[-1]))
    cx, cy = rng.uniform(0, w, n)[part], rng.uniform(0, h, n)[part]
    xy = np.round(np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1), 2)
    group_off = np.concatenate([[0], np.cumsum(parts_per)])
    return xy, off, np.full(n, h), np.full(n, w), group_off


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def codec_cpu(args):
    import ctypes
    import platform
    import subprocess
    import tempfile
    import time
    import numpy as np

    class RLE(ctypes.Structure):   # typedef struct { siz h, w, m; uint *cnts; } RLE
        _fields_ = [("h", ctypes.c_ulong), ("w", ctypes.c_ulong), ("m", ctypes.c_ulong), ("cnts", ctypes.POINTER(ctypes.c_uint))]

    xy, off, hs, ws, group_off = workload(np, args.annotations)
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libmaskapi.so")
        src = os.path.abspath(args.codec_source)
        subprocess.run(["cc", "-O2", "-std=c99", "-shared", "-fPIC", "-I" + os.path.dirname(src), src, "-lm", "-o", so], check=True)
        dll = ctypes.CDLL(so)
        P, UL = ctypes.POINTER, ctypes.c_ulong
        dll.rleFrPoly.argtypes, dll.rleFrPoly.restype = [P(RLE), ctypes.c_void_p, UL, UL, UL], None
        dll.rleMerge.argtypes, dll.rleMerge.restype = [P(RLE), P(RLE), UL, ctypes.c_int], None
        dll.rleFree.argtypes, dll.rleFree.restype = [P(RLE)], None
        n, base = len(hs), xy.ctypes.data
        ks = np.diff(off).tolist()
        addr = (base + 16 * off[:-1]).tolist()
        times, runs = [], 0
        for _ in range(max(1, min(args.reps, 3))):
            rs, ms = (RLE * n)(), (RLE * (len(group_off) - 1))()
            t0 = time.perf_counter()
            for i in range(n):
                dll.rleFrPoly(ctypes.byref(rs[i]), addr[i], ks[i], 480, 640)
            t1 = time.perf_counter()
            for g in range(len(group_off) - 1):
                dll.rleMerge(ctypes.byref(rs[int(group_off[g])]), ctypes.byref(ms[g]),
                             int(group_off[g + 1] - group_off[g]), 0)
            t2 = time.perf_counter()
            times.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
            runs = sum(int(m.m) for m in ms)
            for r in list(rs) + list(ms):
                dll.rleFree(ctypes.byref(r))
    cpu = platform.processor() or platform.machine()
    try:
        cpu = next(l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name"))
    except (OSError, StopIteration):
        pass
    row = dict(what="reference_codec_cpu", rle_from_poly=spread([a for a, _ in times]), rle_merge=spread([b for _, b in times]),
               **spread([a + b for a, b in times]), annotations=args.annotations, parts=n, vertices=int(off[-1]), merged_runs=runs,
               cpu=cpu, threads=1, note="maskApi.c -O2 through ctypes on the CPU named here: NOT the machine of the GPU lines; context only")
    with open(args.out, "a") as fh:
        fh.write(json.dumps(row) + "\n")
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_microbench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--annotations", type=int, default=40000)
    ap.add_argument("--codec-source", default=None, help="maskApi.c of the COCO API: time it on this CPU instead (no GPU needed)")
    args = ap.parse_args()
    if args.codec_source:
        return codec_cpu(args)
    import numpy as np
    import torch
    from maskrcnn_amd import ops
    dev = torch.device("cuda:0")
    xy, off, hs, ws, group_off = workload(np, args.annotations)
    bounds = ops.poly_host_bounds(xy, off, hs, ws)
    cap = int(bounds.max()) + 1
    run_bound = np.concatenate([[0], np.cumsum(bounds + 1)])
    merged_cap = int((run_bound[group_off[1:]] - run_bound[group_off[:-1]]).max())
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(dev)
    d_xy, d_off, d_h, d_w, d_goff = to(xy, np.float64), to(off, np.int32), to(hs, np.int32), to(ws, np.int32), to(group_off, np.int32)
    poly = lambda: ops.rle_from_poly(d_xy, d_off, d_h, d_w, capacity=cap)
    table = poly()                                             # warm-up
    merge = lambda: ops.rle_merge(table[0], table[1], d_goff, capacity=merged_cap)
    merged = merge()
    torch.cuda.synchronize()
    t_poly, t_merge = [], []
    for _ in range(args.reps):
        t_poly.append(event_ms(torch, poly)[0])
        t_merge.append(event_ms(torch, merge)[0])
    nr, nk, mr = table[0].cpu().numpy(), table[2].cpu().numpy(), merged[0].cpu().numpy()
    assert (nr >= 1).all() and (nr <= cap).all() and (mr >= 1).all() and (mr <= merged_cap).all()
    sizes = dict(annotations=args.annotations, parts=int(len(hs)), vertices=int(off[-1]), image=[480, 640], keys=int(nk.sum()),
                 part_runs=int(nr.sum()), merged_runs=int(mr.sum()), capacity=cap, merged_capacity=merged_cap,
                 device=torch.cuda.get_device_name(0))
    rows = [dict(what="rle_from_poly", **spread(t_poly), **sizes), dict(what="rle_merge", **spread(t_merge), **sizes),
            dict(what="both", **spread([a + b for a, b in zip(t_poly, t_merge)]), **sizes)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
