"""Shared by tests/test_optim_host.py and tests/test_gpu_optim.py: the tensor table both run, the reference and the bars.

The reference's optimiser is stock torch (model.py:1542-1557, 1632-1637), so the expected values are its own composition in float64
on the CPU: clip_grad_norm_(params, max_norm), then torch.optim.SGD with the decay group and the no-decay group. reference() always
runs ONE step from the fp32 state widened to float64, with the momentum buffer injected into optimizer.state.

Bars (derived, not fitted):
  p', b', g': |got - want| <= 1 fp32 ulp of want + 1e-14. The rule is a correctly rounded fp64 evaluation narrowed once (<= 0.5 ulp
    from the exact fp64 value), and torch's float64 kernels differ from it by a few fp64 roundings (<< 0.5 fp32 ulp; 1e-14 covers
    them next to 0, where an ulp of the result says nothing about the operands' size).
  norm: S is a sum of non-negative exact products, so every addition's relative error 2^-53 reaches the total at most once per
    level an element passes through: the thread's chain (TILE / 256 additions), the wave tree (6), the waves (4), and the same
    again in the finishing pass with a chain of ceil(tiles / 256). The yardstick is math.fsum of the products, which is exact; the
    square root halves the relative error and adds its own rounding and the yardstick's. norm_bound() returns that; it may not
    exceed 1e-12, and at these sizes one missing or doubled element of unit scale moves S by >= 1e-6 relative.
"""
import math

import numpy as np
import torch

THREADS, TREE, WAVES = 256, 6, 4


def sizes(t0):
    """Vector tails, tile edges, one tensor with more tiles than the finishing workgroup has threads, and 300 one-element
    tensors (more entries than a workgroup is wide for the binary search)."""
    return [1, 3, 4, 5, t0 - 1, t0, t0 + 1, 2 * t0 + 3, 257 * t0 + 1] + [1] * 300


class Case:
    """fp32 CPU state of one table: p, g (None: no gradient), b per tensor, decay[i] (which of the two groups), and the indices
    of the parameter stored one element into its storage (view), its aligned twin (twin), the tensor without a gradient (nograd)
    and the empty one (empty)."""

    def __init__(self, t0, seed=0, gscale=1.0, cancel=False, integers=False):
        gen = torch.Generator().manual_seed(seed)
        ns = sizes(t0)
        self.view, self.twin, self.nograd, self.empty = len(ns), len(ns) + 1, len(ns) + 2, len(ns) + 3
        ns = ns + [2 * t0 + 5, 2 * t0 + 5, 7, 0]
        if integers:
            draw = lambda n, hi: torch.randint(-hi, hi + 1, (n,), generator=gen).float()
            self.p, self.g, self.b = [draw(n, 64) for n in ns], [draw(n, 8) for n in ns], [draw(n, 16) for n in ns]
        else:
            self.p = [torch.randn(n, generator=gen) for n in ns]
            self.g = [torch.randn(n, generator=gen) * gscale for n in ns]
            self.b = [torch.randn(n, generator=gen) * gscale for n in ns]
            if cancel:      # a momentum term that all but cancels the gradient: B is the small difference of two large numbers
                self.b = [-(g / 0.9) for g in self.g]
        for name in ("p", "g", "b"):
            getattr(self, name)[self.twin] = getattr(self, name)[self.view].clone()
        self.g[self.nograd] = None
        self.decay = [i % 2 == 0 for i in range(len(ns))]
        self.decay[self.twin] = self.decay[self.view]

    def params(self, device):
        """→ the Parameters with their gradients, in the case's order. The view parameter lies one element into its storage;
        everything else is its own allocation."""
        ps = []
        for i, (p, g) in enumerate(zip(self.p, self.g)):
            if i == self.view:
                store = torch.zeros(p.numel() + 1, device=device)
                q = torch.nn.Parameter(store[1:])
                with torch.no_grad():
                    q.copy_(p)
            else:
                q = torch.nn.Parameter(p.clone().to(device))
            q.grad = None if g is None else g.clone().to(device)
            ps.append(q)
        return ps

    def groups(self, ps, wd):
        """The reference's two groups: weight decay on the first only."""
        return [{"params": [q for q, d in zip(ps, self.decay) if d], "weight_decay": wd},
                {"params": [q for q, d in zip(ps, self.decay) if not d]}]

    def load_buffers(self, opt, ps):
        for q, b in zip(ps, self.b):
            opt.state[q]["momentum_buffer"].copy_(b)


class Snapshot:
    """The fp32 state of live parameters as reference() reads a Case: what the code under test is about to step from."""

    def __init__(self, opt, ps, decay):
        host = lambda t: None if t is None else t.detach().cpu().clone()
        self.p, self.g, self.b = [host(q) for q in ps], [host(q.grad) for q in ps], [host(opt.state[q]["momentum_buffer"]) for q in ps]
        self.decay = list(decay)


def run_case(optim, case, hyper, mode, device):
    """The code under test on `case`: → (optimiser, parameters, returned norm)."""
    ps = case.params(device)
    opt = optim.ClippedSGD(case.groups(ps, hyper["wd"]), lr=hyper["lr"], momentum=hyper["momentum"], max_norm=hyper["max_norm"])
    case.load_buffers(opt, ps)
    norm = opt.clip_() if mode == "clip" else opt.step(zero_grad=mode == "step_zero")
    return opt, ps, norm


def compare(case, opt, ps, norm, want, t0):
    """Every bar of the module docstring on one finished step; returns the worst ulp figure and the norm's relative error."""
    worst = 0.0
    for i, q in enumerate(ps):
        b = opt.state[q]["momentum_buffer"]
        if case.g[i] is None:       # skipped entirely: no decay, no momentum update
            assert q.grad is None and torch.equal(bits(q), bits(case.p[i])) and torch.equal(bits(b), bits(case.b[i])), i
            continue
        for name, got, exp in (("p", q, want["p"][i]), ("b", b, want["b"][i]), ("g", q.grad, want["g"][i])):
            e = ulp_excess(got, exp)
            worst = max(worst, e)
            assert e <= 1.0, f"tensor {i} ({q.numel()} elements) {name}: {e:.3f} ulp"
    # the scalar path (a parameter one element into its storage) and the 16-byte path: same bits
    for name in ("p", "b", "g") if hasattr(case, "view") else ():
        pick = lambda i: {"p": ps[i], "b": opt.state[ps[i]]["momentum_buffer"], "g": ps[i].grad}[name]
        assert torch.equal(bits(pick(case.view)), bits(pick(case.twin))), name
    rel = 0.0
    if norm is not None:
        rel = abs(float(norm) - want["norm"]) / want["norm"]
        assert norm.dtype == torch.float64 and norm.dim() == 0
        assert rel <= norm_bound(t0, tiles_of(case, t0)), rel
        assert abs(want["norm_torch"] - want["norm"]) / want["norm"] <= 1e-12
    assert opt.status.dtype == torch.int32 and opt.status.tolist() == [0]
    return worst, rel


def reference(case, lr, momentum, wd, max_norm, mode):
    """One step of the reference's composition in float64 → dict(p, b, g: lists of float64 tensors (g None where there is no
    gradient), norm_torch: clip_grad_norm_'s return, norm: sqrt of the exactly summed squares, clipped: norm > max_norm)."""
    ps = [torch.nn.Parameter(p.double()) for p in case.p]
    for q, g in zip(ps, case.g):
        q.grad = None if g is None else g.double().clone()
    squares = [float(v) for g in case.g if g is not None for v in (g.double() * g.double()).reshape(-1).tolist()]
    out = {"norm": math.sqrt(math.fsum(squares)), "norm_torch": None}
    if max_norm is not None:
        out["norm_torch"] = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    out["clipped"] = max_norm is not None and out["norm"] > max_norm
    bs = [b.double().clone() for b in case.b]
    if mode != "clip":
        opt = torch.optim.SGD([{"params": [q for q, d in zip(ps, case.decay) if d], "weight_decay": wd},
                               {"params": [q for q, d in zip(ps, case.decay) if not d]}], lr=lr, momentum=momentum)
        if momentum != 0:
            for q, b in zip(ps, bs):
                opt.state[q]["momentum_buffer"] = b
        else:       # torch keeps no buffer then; the rule's B = 0 * b + d = d is what the buffer receives
            bs = [b if q.grad is None else q.grad + (wd if d else 0.0) * q.detach() for q, b, d in zip(ps, bs, case.decay)]
        opt.step()
    out["p"] = [q.detach() for q in ps]
    out["b"] = bs
    out["g"] = [None if q.grad is None else (torch.zeros_like(q.grad) if mode == "step_zero" else q.grad) for q in ps]
    return out


def ulp_excess(got, want):
    """max over the elements of (|got - want| - 1e-14) in fp32 ulps of want: <= 1 passes. got fp32, want float64."""
    got, want = got.detach().cpu().double().reshape(-1).numpy(), want.reshape(-1).numpy()
    if got.size == 0:
        return 0.0
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return float(np.max((np.abs(got - want) - 1e-14) / ulp))


def norm_bound(t0, tiles):
    depth = (t0 // THREADS + TREE + WAVES) + (-(-tiles // THREADS) + TREE + WAVES)
    bound = (0.5 * depth + 2.0) * 2.0 ** -53 * 1.01
    assert bound <= 1e-12, bound
    return bound


def tiles_of(case, t0):
    return sum(-(-p.numel() // t0) for p in case.p)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# name -> (Case keywords, dict(lr, momentum, wd, max_norm), mode)
H = dict(lr=0.01, momentum=0.9, wd=1e-4, max_norm=5.0)
CONFIGS = {
    "clipped step": ({}, H, "step"),
    "clipped step_zero": ({}, H, "step_zero"),
    "clipped clip": ({}, H, "clip"),
    "unclipped step": ({"gscale": 1e-4}, H, "step"),
    "large gradients": ({"gscale": 100.0}, H, "step_zero"),
    "momentum 0": ({}, dict(H, momentum=0.0), "step"),
    "lr 0": ({}, dict(H, lr=0.0), "step"),
    "no max_norm": ({}, dict(H, max_norm=None), "step"),
    "cancelling momentum": ({"cancel": True}, dict(H, max_norm=1e9, wd=0.0), "step"),
}
# integers for g, p and b; lr, momentum and wd powers of two; max_norm above the norm (c = 1): every operation is exact in fp32
# and fp64 alike, so the result equals float64's and torch fp32's bit for bit
EXACT = ({"integers": True}, dict(lr=2.0 ** -3, momentum=0.5, wd=2.0 ** -4, max_norm=2.0 ** 40), "step")
