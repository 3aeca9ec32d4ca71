"""ClippedSGD: what the reference does after every loss.backward() (model.py:1542-1557, 1632-1637) — clip_grad_norm_ over all
parameters, and on every BATCH_SIZE-th iteration optim.SGD(momentum, weight decay on the non-BN group).step() and zero_grad() — as
three launches of csrc/optim.hip on a device-resident table of the tensors, whatever their number, without a host synchronisation.
The rule is stated at mrcnn_optim_clip_coef in include/maskrcnn_hip.h; parameters on the CPU run the same rule in numpy float64
(the family's device="cpu" convention), in the same summation order.

    opt = ClippedSGD([{"params": weights, "weight_decay": 1e-4}, {"params": bn}], lr=0.001, momentum=0.9, max_norm=5.0)
    loss.backward(); opt.clip_()                    # the iterations between two optimiser steps
    loss.backward(); opt.step(zero_grad=True)       # clip, update, and the gradients left at +0
"""
from __future__ import annotations

import collections
import math

import numpy as np
import torch

from . import ops
from ._lib import lib

TILE = int(lib.mrcnn_optim_tile())            # elements of a tile: a compile-time constant of csrc/optim.hip
_THREADS, _WAVE = 256, 64                     # a tile's workgroup and the finishing workgroup; the wave of gfx950
MAX_TENSORS, MAX_NUMEL, MAX_TILES = 65535, (1 << 31) - 1, 1 << 24

TensorTable = collections.namedtuple("TensorTable", "table wd tile_off tiles aligned")


def build_table(entries, tile: int = TILE) -> TensorTable:
    """The host form of the tensor table the kernels read. entries: one (address of p, address of g or 0, address of b, numel,
    weight decay) per tensor → TensorTable(table int64 [T,4], wd float64 [T], tile_off int64 [T+1]: the exclusive prefix sum of
    ceil(numel / tile), whether the tensor has a gradient or not; tiles = tile_off[T]; aligned bool [T]: the three addresses on
    16-byte boundaries, where the kernels use 16-byte accesses), all numpy. The limits only the builder can see are refused here, as
    a RuntimeError in the bindings' format."""
    who = "sgd_table"
    t = len(entries)
    if not 1 <= t <= MAX_TENSORS:
        raise RuntimeError(f"{who}: the number of tensors must be in 1 .. {MAX_TENSORS}, got {t}")
    table = np.empty((t, 4), dtype=np.int64)
    wd = np.empty(t, dtype=np.float64)
    for i, (p, g, b, numel, decay) in enumerate(entries):
        if not 0 <= int(numel) <= MAX_NUMEL:
            raise RuntimeError(f"{who}: numel of tensor {i} must be below 2^31, got {numel}")
        if not math.isfinite(decay):
            raise RuntimeError(f"{who}: wd of tensor {i} must be a finite number, got {decay}")
        table[i] = (p, g, b, numel)
        wd[i] = decay
    tile_off = np.zeros(t + 1, dtype=np.int64)
    np.cumsum(-(-table[:, 3] // tile), out=tile_off[1:])
    tiles = int(tile_off[-1])
    if tiles > MAX_TILES:
        raise RuntimeError(f"{who}: tiles must be at most 2^24 ({tile} elements a tile), got {tiles}")
    aligned = ((table[:, 0] | table[:, 1] | table[:, 2]) & 15) == 0
    return TensorTable(table, wd, tile_off, tiles, aligned)


def _scan_total(v: np.ndarray) -> np.ndarray:
    """block_sum of csrc/workgroup.hpp over the last axis (256 threads): per wave of 64 the shuffle scan's last lane — the balanced
    tree —, then the wave sums in wave order from +0."""
    w = v.reshape(*v.shape[:-1], _THREADS // _WAVE, _WAVE)
    while w.shape[-1] > 1:
        w = w[..., 0::2] + w[..., 1::2]
    w = w[..., 0]
    total = np.zeros(w.shape[:-1], dtype=np.float64)
    for i in range(w.shape[-1]):
        total = total + w[..., i]
    return total


def sumsq_fixed_order(grads, tile: int = TILE) -> float:
    """S of the rule in the kernels' summation order, in numpy float64. grads: per tensor of the table a float32 array, or None for
    a tensor without a gradient (its tiles count, as +0: they decide which thread of the finishing pass adds which tile)."""
    vecs = tile // (4 * _THREADS)
    parts = []
    for g, numel in grads:
        n_tiles = -(-numel // tile)
        if g is None or n_tiles == 0:
            parts.append(np.zeros(n_tiles, dtype=np.float64))
            continue
        x = np.zeros(n_tiles * tile, dtype=np.float64)
        x[:numel] = np.asarray(g, dtype=np.float32).reshape(-1).astype(np.float64)
        x = (x * x).reshape(n_tiles, vecs, _THREADS, 4)          # element (256 i + k) 4 + j of a tile: thread k
        acc = np.zeros((n_tiles, _THREADS), dtype=np.float64)
        for i in range(vecs):
            for j in range(4):
                acc = acc + x[:, i, :, j]
        parts.append(_scan_total(acc))
    part = np.concatenate(parts) if parts else np.zeros(0)
    tiles = part.size
    chunk = -(-tiles // _THREADS)
    runs = np.zeros(_THREADS * chunk, dtype=np.float64)
    runs[:tiles] = part
    runs = runs.reshape(_THREADS, chunk)
    acc = np.zeros(_THREADS, dtype=np.float64)
    for i in range(chunk):
        acc = acc + runs[:, i]
    return float(_scan_total(acc))


class ClippedSGD(torch.optim.Optimizer):
    """torch.optim.SGD(momentum, weight_decay; dampening 0, no nesterov) behind clip_grad_norm_(all parameters, max_norm), on fp32
    parameters of ONE device. Groups may differ in weight_decay only (the reference's two groups); lr, momentum and max_norm are
    read from param_groups at every call, so torch's LR schedulers work. max_norm=None: no clipping and no non-finite check.

    clip_() is the reference's clip_grad_norm_ line; step(zero_grad=False) is clip + update (+ zeroing). Both return the total norm
    as a 0-dim float64 tensor on the parameters' device and leave the call's int32 [1] status in opt.status (bit 0: the squared
    norm was NaN or Inf — then parameters and momentum buffers are untouched, and so are the gradients but for a requested
    zeroing). Nothing synchronises with the host.

    The kernels work through a table of addresses. It is built at construction; before EVERY call the data_ptr() of each
    parameter, gradient (None: the tensor is skipped, as in torch) and momentum buffer is compared with what the table holds, and
    a fresh table is uploaded when any differs — a replaced p.grad, zero_grad(set_to_none=True), a loaded state. Momentum buffers
    are state[p]["momentum_buffer"], zeros from construction on: state_dict() and load_state_dict() interchange with
    torch.optim.SGD's."""

    def __init__(self, params, lr: float, momentum: float = 0.9, weight_decay: float = 0.0, max_norm: float | None = 5.0):
        self._sig = None         # what the uploaded table was built from
        self._device_table = None
        self._status = None
        # every key torch.optim.SGD's groups carry, so that either optimiser loads the other's state_dict
        defaults = dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False, maximize=False, foreach=None,
                        differentiable=False, fused=None, max_norm=max_norm)
        super().__init__(params, defaults)
        self._hyper()

    # ------------------------------------------------------------------------------------------------ configuration
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._buffers()
        self._params()

    def _buffers(self) -> None:
        for group in self.param_groups:
            for p in group["params"]:
                if self.state[p].get("momentum_buffer") is None:
                    self.state[p]["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format).detach()

    def _params(self):
        """[(parameter, weight decay)] in table order, each checked."""
        out, dev = [], None
        for group in self.param_groups:
            for p in group["params"]:
                if p.dtype != torch.float32 or p.layout != torch.strided or not p.is_contiguous():
                    raise ValueError(f"ClippedSGD: parameters must be dense contiguous float32 tensors, got {str(p.dtype)[6:]} "
                                     f"{list(p.shape)} ({p.layout}, strides {tuple(p.stride())})")
                dev = p.device if dev is None else dev
                if p.device != dev:
                    raise ValueError(f"ClippedSGD: parameters on more than one device ({dev} and {p.device})")
                out.append((p, float(group["weight_decay"])))
        return out

    def _hyper(self):
        """(lr, momentum, max_norm) of this call: one value over all groups."""
        first = self.param_groups[0]
        for group in self.param_groups:
            for key in ("lr", "momentum", "max_norm"):
                if group[key] != first[key]:
                    raise ValueError(f"ClippedSGD: groups may differ in weight_decay only, got {key} {first[key]} and {group[key]}")
            for key in ("nesterov", "dampening", "maximize"):
                if group.get(key):
                    raise ValueError(f"ClippedSGD: {key} is not supported (got {group[key]})")
        lr, momentum, max_norm = float(first["lr"]), float(first["momentum"]), first["max_norm"]
        if not math.isfinite(lr):
            raise ValueError(f"ClippedSGD: lr must be finite, got {lr}")
        if not 0.0 <= momentum < 1.0:
            raise ValueError(f"ClippedSGD: momentum must be in [0, 1), got {momentum}")
        if max_norm is not None and not float(max_norm) > 0:
            raise ValueError(f"ClippedSGD: max_norm must be above 0 or None, got {max_norm}")
        return lr, momentum, None if max_norm is None else float(max_norm)

    def _tensors(self):
        """[(p, gradient or None, momentum buffer, weight decay)] of this call, each gradient checked."""
        out = []
        for p, wd in self._params():
            g, b = p.grad, self.state[p].get("momentum_buffer")
            if g is not None and (g.dtype != torch.float32 or g.layout != torch.strided or g.shape != p.shape or not g.is_contiguous()
                                  or g.device != p.device):
                raise ValueError(f"ClippedSGD: a gradient must be a contiguous float32 tensor of its parameter's shape {list(p.shape)} "
                                 f"on {p.device}, got {str(g.dtype)[6:]} {list(g.shape)} ({g.layout}, strides "
                                 f"{tuple(g.stride()) if g.layout == torch.strided else None}) on {g.device}")
            if b is None or b.dtype != torch.float32 or b.shape != p.shape or b.device != p.device or not b.is_contiguous():
                raise ValueError(f"ClippedSGD: state[p]['momentum_buffer'] must be a contiguous float32 tensor of the parameter's shape "
                                 f"{list(p.shape)} on {p.device}")
            out.append((p, g, b, wd))
        return out

    @property
    def status(self):
        """int32 [1] of the last clip_() / step(): bit 0 = the squared gradient norm was not finite. None before the first call."""
        return self._status

    # ------------------------------------------------------------------------------------------------ the calls
    def clip_(self):
        """clip_grad_norm_(all parameters, max_norm) in place on the gradients → the total norm, 0-dim float64."""
        return self._run("clip")

    def step(self, closure=None, *, zero_grad: bool = False):
        """Clip, then the momentum step; zero_grad=True also leaves every gradient that took part at +0 (the reference's
        optimizer.zero_grad(), without a pass of its own) → the total norm, 0-dim float64 (None with max_norm=None). A closure is
        evaluated first, as torch's optimisers do, but its loss is NOT returned: the return value is the norm."""
        if closure is not None:
            with torch.enable_grad():
                closure()
        return self._run("step_zero" if zero_grad else "step")

    def zero_grad(self, set_to_none: bool = False) -> None:
        """torch's zero_grad, but the gradient tensors are kept by default: their addresses stay what the table holds."""
        super().zero_grad(set_to_none=set_to_none)

    def load_state_dict(self, state_dict) -> None:
        """torch's, then what a torch.optim.SGD state lacks: max_norm in the groups, and zeros for a missing momentum buffer."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            group.setdefault("max_norm", self.defaults["max_norm"])
        self._buffers()
        self._hyper()

    @torch.no_grad()
    def _run(self, mode: str):
        lr, momentum, max_norm = self._hyper()
        if mode == "clip" and max_norm is None:
            raise ValueError("ClippedSGD: clip_() needs a max_norm")
        tensors = self._tensors()
        if not tensors[0][0].is_cuda:
            return self._run_numpy(tensors, lr, momentum, max_norm, mode)
        # The one check that is never skipped: a table that no longer names the live tensors is a write through a dead pointer.
        sig = [(p.data_ptr(), 0 if g is None else g.data_ptr(), b.data_ptr(), p.numel(), wd) for p, g, b, wd in tensors]
        if sig != self._sig:
            host = build_table(sig)
            dev = tensors[0][0].device
            with torch.cuda.device(dev):     # new tensors on the current stream: launches in flight keep the table they were given
                self._device_table = (torch.from_numpy(host.table).to(dev), torch.from_numpy(host.wd).to(dev),
                                      torch.from_numpy(host.tile_off).to(dev), host.tiles)
            self._sig = sig
        table, wd, tile_off, tiles = self._device_table
        info = status = None
        if max_norm is not None:
            info, status = ops.grad_clip_coef(table, tile_off, max_norm, tiles=tiles)
        ops.sgd_apply(table, wd, tile_off, info, status, lr, momentum, mode, tiles=tiles)
        self._status = status if status is not None else torch.zeros(1, dtype=torch.int32, device=table.device)
        return None if info is None else info[1]

    def _run_numpy(self, tensors, lr, momentum, max_norm, mode):
        """The rule on CPU parameters, in place through numpy views of the tensors."""
        views = [(p.detach().numpy(), None if g is None else g.detach().numpy(), b.detach().numpy(), wd) for p, g, b, wd in tensors]
        build_table([(0, 0, 0, p.size, wd) for p, _, _, wd in views])     # the same limits
        c, bad, info = 1.0, False, None
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            if max_norm is not None:
                s = sumsq_fixed_order([(g, p.size) for p, g, _, _ in views])
                norm = math.sqrt(s) if s == s else s
                q = max_norm / (norm + 1e-6)
                c, bad = (q if q < 1.0 else 1.0), not math.isfinite(s)
                info = torch.tensor([s, norm, c], dtype=torch.float64)
            for p, g, b, wd in views:
                if g is None:
                    continue
                if not bad:
                    cg = c * g.astype(np.float64)
                    if mode != "clip":
                        p64 = p.astype(np.float64)
                        nb = momentum * b.astype(np.float64) + (cg + wd * p64)
                        b[...] = nb.astype(np.float32)
                        p[...] = (p64 - lr * nb).astype(np.float32)
                    if mode != "step_zero":
                        g[...] = cg.astype(np.float32)
                if mode == "step_zero":
                    g[...] = 0.0
        self._status = torch.tensor([int(bad)], dtype=torch.int32)
        return None if info is None else info[1]
