"""crop_forward_nchw on the BASELINE configs[1] shapes (256 RoIs x 256 ch x 14x14 on P2..P5), staged kernel vs gather kernel
(MRCNN_CROP_STAGED), channels per wave (MRCNN_CROP_CPW; honoured by a -DMRCNN_TUNING build loaded through MRCNN_LIB only).
Usage: python tools/crop_probe.py [cpw ...]

The library reads its switches ONCE per process, so every setting runs in a child process of its own, one after the other, with
the variables in its environment from the start; each child reports what the launcher says it launched (ops.crop_plan), the
time, and a digest of the result's bits, which the parent compares with the gather kernel's."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timeit(fn, iters=20, reps=5):
    """Device time per call: the calls are captured in a hipGraph (the Python + ctypes cost of a call, ~20 us, would
    otherwise bound a 20 us kernel) and the graph is replayed."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / iters * 1e3)
    return best


def levels():
    return [int(v) for v in os.environ.get("CROP_LEVELS", "256,128,64,32").split(",")]


def child():
    """One setting (this process's environment), every level: a JSON line per level."""
    import torch
    from maskrcnn_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1234)
    for hl in levels():
        fm = torch.randn(1, 256, hl, hl, generator=g).to(dev)
        c = torch.rand(256, 2, generator=g)
        hw = torch.rand(256, 2, generator=g) * 0.10 + 0.02
        boxes = torch.cat([c - hw / 2, c + hw / 2], 1).clamp(0, 1).to(dev)
        ind = torch.zeros(256, dtype=torch.int32, device=dev)
        us = timeit(lambda: ops.crop(fm, boxes, ind, 0.0, 14, 14))
        got = ops.crop(fm, boxes, ind, 0.0, 14, 14)
        plan = ops.crop_plan(256, hl, hl, 256, 14, 14, fm, got)
        print("PROBE " + json.dumps({"level_hw": hl, "us": us, "plan": plan._asdict(),
                                     "digest": hashlib.sha1(got.cpu().numpy().tobytes()).hexdigest()}), flush=True)


def run_setting(staged, cpw):
    env = dict(os.environ, MRCNN_CROP_STAGED="1" if staged else "0")
    env.pop("MRCNN_CROP_CPW", None)
    if cpw:
        env["MRCNN_CROP_CPW"] = str(cpw)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"crop_probe child (staged={staged}, cpw={cpw}) failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    rows = [json.loads(l[6:]) for l in r.stdout.splitlines() if l.startswith("PROBE ")]
    return {row["level_hw"]: row for row in rows}


def main():
    cpws = [int(a) for a in sys.argv[1:]] or [0]
    gather = run_setting(False, 0)
    staged = {cpw: run_setting(True, cpw) for cpw in cpws}
    for hl in levels():
        algo = 256 * 256 * 14 * 14 * 4 + 256 * hl * hl * 4 + 256 * 20
        ref = gather[hl]
        if ref["plan"]["route"] != "gather":
            raise RuntimeError(f"MRCNN_CROP_STAGED=0 did not reach the gather kernel: {ref['plan']}")
        row = {"level_hw": hl, "algorithmic_MB": round(algo / 1e6, 2), "gather_us": round(ref["us"], 2)}
        for cpw in cpws:
            s = staged[cpw][hl]
            if s["plan"]["route"] != "staged" or (cpw and s["plan"]["cpw"] != cpw):
                raise RuntimeError(f"cpw {cpw} asked, the launcher answers {s['plan']} (MRCNN_CROP_CPW needs a -DMRCNN_TUNING "
                                   "build: build.py --variant tuning -DMRCNN_TUNING, loaded through MRCNN_LIB)")
            row[f"staged_cpw{cpw}_us"] = round(s["us"], 2)
            row[f"staged_cpw{cpw}_plan_cpw"] = s["plan"]["cpw"]
            row[f"staged_cpw{cpw}_frac_of_8TBps"] = round(algo / s["us"] / 1e3 / 8000.0, 4)
            row[f"staged_cpw{cpw}_equal"] = s["digest"] == ref["digest"]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
