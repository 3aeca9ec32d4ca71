"""The RPN in training mode: a dense pass without a graph for the proposals, and a differentiable branch on the sampled anchors alone.

Nothing in the reference carries a gradient through the proposals: rpn_refine reaches NMS through .data (model.py:1349-1365), roi_align
detaches the boxes (:358), mrn_samples computes its targets from .data (:484). The only gradient into the RPN comes from
RPN.class_loss and RPN.boxes_loss (model.py:652-718), and those gather the anchors with rpn_match != 0 — at most
RPN_TRAIN_ANCHORS_PER_IMAGE of 261 888 at 1024 x 1024. The dense graph would push zeros through the shared 3x3 conv (256 -> 512) and the
two 1x1 heads on 87 296 pixels per image and save a [B,87296,512] activation for it. Here

    rpn = TrainableRPN.from_state_dict(sd).to("cuda")
    scores, deltas = rpn.dense(fms)                              # no_grad: what MaskRCNNInference.proposals consumes
    out = rpn.losses(fms, rpn_match, rpn_bbox)                   # RpnLosses, with a grad_fn
    (out.rpn_class_loss + out.rpn_bbox_loss).backward()          # gradients in the five maps and the six parameters

and the differentiable branch is, for the sampled anchors (csrc/rpn_train.hip; the rules are stated at mrcnn_anchor_compact in
include/maskrcnn_hip.h): ops.anchor_compact, the gather of the 3x3xC patches under their pixels (pyramid_patches: one autograd node,
forward ops.pyramid_patch_gather, backward ops.pyramid_patch_scatter), the shared conv and the fused heads as two layers.conv_bn_act
GEMMs on [B*count,1,1,9C] rows — the classifier's conv1 trick —, the selection of each anchor's six values and losses.rpn_losses on
the compacted rows. Nothing in that path synchronises with the host.

Anchor order is ops.rpn_scores_deltas': level l has H_l x W_l pixels and apl anchors per pixel, anchor
a = first[l] + (y * W_l + x) * apl + r; of the fused head output anchor r owns logits 2r, 2r+1 and deltas 2*apl + 4r .. +3.

CPU parameters, or device="cpu", run the same rules without the library: compact_numpy, gather_numpy and scatter_numpy below restate
the three kernels, and the GEMMs, the selection and the losses are stock torch and losses' numpy route.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import losses as _losses
from .losses import RpnLosses

__all__ = ["pyramid_patches", "TrainableRPN", "anchor_firsts", "compact_numpy", "gather_numpy", "scatter_numpy", "STATUS_OVERFLOW"]

STATUS_OVERFLOW = 2      # bit 1 of TrainableRPN.losses(...).status: the image has more than `count` anchors with match != 0


# ----------------------------------------------------------------------------------------------------------------------
# The three kernels' rules in numpy
# ----------------------------------------------------------------------------------------------------------------------
def anchor_firsts(sizes, anchors_per_location: int = 3) -> list:
    """[(H_l, W_l)] → [first[0] = 0, .., first[L] = A]: the first anchor of each level, and the number of anchors."""
    first = [0]
    for h, w in sizes:
        first.append(first[-1] + int(h) * int(w) * int(anchors_per_location))
    return first


def compact_numpy(match, count: int):
    """match [B,A] → (index int32 [B,count], num int32 [B], status int32 [B]): an image's anchors with match != 0 in ascending order,
    -1 past num = min(count, their number); status bit 0: more than count of them."""
    m = np.asarray(match)
    b = m.shape[0]
    index = np.full((b, count), -1, np.int32)
    num, status = np.zeros(b, np.int32), np.zeros(b, np.int32)
    for i in range(b):
        nz = np.nonzero(m[i].reshape(-1))[0]
        num[i] = min(count, len(nz))
        status[i] = int(len(nz) > count)
        index[i, :num[i]] = nz[:count]
    return index, num, status


def _entries(index, num, sizes, apl):
    """(b, k, level, py, px) of every live slot, in ascending (b, k)."""
    first = anchor_firsts(sizes, apl)
    index, num = np.asarray(index), np.asarray(num)
    for b in range(index.shape[0]):
        for k in range(min(max(int(num[b]), 0), index.shape[1])):
            a = int(index[b, k])
            if not 0 <= a < first[-1]:
                continue
            l = max(i for i in range(len(sizes)) if a >= first[i])
            pix = (a - first[l]) // apl
            yield b, k, l, pix // sizes[l][1], pix % sizes[l][1]


def gather_numpy(maps, index, num, anchors_per_location: int = 3) -> np.ndarray:
    """maps: [B,H_l,W_l,C] arrays → patches [B*K,9*C] in the maps' dtype: row (b, k), column (ky*3+kx)*C + c holds
    map_l[b, py+ky-1, px+kx-1, c]; +0 for a tap outside the map and for an empty slot."""
    maps = [np.asarray(m) for m in maps]
    index = np.asarray(index)
    bsz, cap = index.shape
    c = maps[0].shape[3]
    out = np.zeros((bsz, cap, 3, 3, c), maps[0].dtype)
    sizes = [m.shape[1:3] for m in maps]
    for b, k, l, py, px in _entries(index, num, sizes, anchors_per_location):
        h, w = sizes[l]
        for ky in range(3):
            for kx in range(3):
                y, x = py + ky - 1, px + kx - 1
                if 0 <= y < h and 0 <= x < w:
                    out[b, k, ky, kx] = maps[l][b, y, x]
    return out.reshape(bsz * cap, 9 * c)


def scatter_numpy(dpatch, index, num, map_sizes, channels: int, anchors_per_location: int = 3, needs=None) -> list:
    """dpatch [B*K,9*C] → [grad_l [B,H_l,W_l,C]] in dpatch's dtype (None where needs[l] is false): per element the sum from +0, in
    ascending slot, each add rounded in that dtype, of dpatch[b,k,y-py+1,x-px+1,c] over the entries of level l within one pixel."""
    index = np.asarray(index)
    bsz, cap = index.shape
    d = np.asarray(dpatch).reshape(bsz, cap, 3, 3, channels)
    sizes = [(int(h), int(w)) for h, w in map_sizes]
    needs = [True] * len(sizes) if needs is None else list(needs)
    grads = [np.zeros((bsz, h, w, channels), d.dtype) if need else None for (h, w), need in zip(sizes, needs)]
    for b, k, l, py, px in _entries(index, num, sizes, anchors_per_location):
        if grads[l] is None:
            continue
        h, w = sizes[l]
        for ky in range(3):
            for kx in range(3):
                y, x = py + ky - 1, px + kx - 1
                if 0 <= y < h and 0 <= x < w:
                    grads[l][b, y, x] = grads[l][b, y, x] + d[b, k, ky, kx]    # slots ascend: one add per slot and element
    return grads


# ----------------------------------------------------------------------------------------------------------------------
# autograd
# ----------------------------------------------------------------------------------------------------------------------
class _PyramidPatches(torch.autograd.Function):
    @staticmethod
    def forward(ctx, index, num, apl, *maps):
        ctx.save_for_backward(index, num)
        ctx.call = (apl, [tuple(m.shape[1:3]) for m in maps], maps[0].size(3))
        if maps[0].is_cuda:
            from . import ops
            return ops.pyramid_patch_gather(list(maps), index, num, apl)
        return torch.from_numpy(gather_numpy([m.detach().numpy() for m in maps], index.numpy(), num.numpy(), apl))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        index, num = ctx.saved_tensors
        apl, sizes, channels = ctx.call
        needs = ctx.needs_input_grad[3:]
        if grad.is_cuda:
            from . import ops
            grads = ops.pyramid_patch_scatter(grad.contiguous(), index, num, sizes, channels, apl, needs=needs)
        else:
            grads = [None if g is None else torch.from_numpy(g)
                     for g in scatter_numpy(grad.contiguous().numpy(), index.numpy(), num.numpy(), sizes, channels, apl, needs)]
        return (None, None, None, *grads)


class _SelectColumns(torch.autograd.Function):
    """x [R,N], cols int64 [R,M], unique within a row → x.gather(1, cols). The backward WRITES the gradient at those columns of a
    zero matrix (stock gather's backward adds it there with atomics): nothing to order, so two calls give the same bits."""

    @staticmethod
    def forward(ctx, x, cols):
        ctx.save_for_backward(cols)
        ctx.width = x.size(1)
        return x.gather(1, cols)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        cols, = ctx.saved_tensors
        return grad.new_zeros(grad.size(0), ctx.width).scatter_(1, cols, grad), None


def pyramid_patches(maps, index: torch.Tensor, num: torch.Tensor, anchors_per_location: int = 3) -> torch.Tensor:
    """The 3x3xC patches of the pyramid under the pixels of the sampled anchors, with a grad_fn: maps = 1 .. 8 float32 NHWC tensors
    [B,H_l,W_l,C] (C % 4 == 0), index int32 [B,K] and num int32 [B] as ops.anchor_compact returns them → float32 [B*K,9*C], row
    (b, k) in the order an OHWI weight [Cout,3,3,C] flattens (SamePad2d(3,1), then the window); +0 rows for the empty slots. The
    forward is ops.pyramid_patch_gather (a bit-exact copy), the backward ops.pyramid_patch_scatter: deterministic, map-stationary,
    and computed only for the maps that need a gradient. index and num get none. CPU tensors run the numpy restatements."""
    maps = [m.contiguous() for m in maps]
    return _PyramidPatches.apply(index, num, int(anchors_per_location), *maps)


def _anchor_columns(index: torch.Tensor, sizes, apl: int) -> torch.Tensor:
    """index int32 [B,K] → int64 [B*K,6]: the columns of anchor r = (index - first[level]) % apl in the fused head output, logits
    2r, 2r+1 and deltas 2*apl + 4r .. +3 (r = 0 for an empty slot, whose row is zeros and whose match is 0). Scalars only: no
    host-to-device copy."""
    idx = index.reshape(-1).clamp(min=0).to(torch.int64)
    level_first = torch.zeros_like(idx)
    for f in anchor_firsts(sizes, apl)[1:-1]:
        level_first = torch.where(idx >= f, torch.full_like(idx, f), level_first)
    r = (idx - level_first) % apl
    return torch.stack([2 * r, 2 * r + 1, 2 * apl + 4 * r, 2 * apl + 4 * r + 1, 2 * apl + 4 * r + 2, 2 * apl + 4 * r + 3], dim=1)


class TrainableRPN(nn.Module):
    """RPN (model.py:597-649) with the reference's parameter names and layouts — conv_shared.weight [512,C,3,3], conv_class.weight
    [2*apl,512,1,1], conv_bbox.weight [4*apl,512,1,1] and their biases —, so the `rpn.` slice of a reference state dict loads and
    train_model's layer regexes apply. The three convs are held as nn.Conv2d for their parameters only; they are never called.

    dense(fms)                    (fg scores [B,A], deltas [B,A,4]) from the current parameters, under no_grad
    sampled(fms, index, num)      (logits [B,K,2], bbox [B,K,4]) of the compacted anchors, with a grad_fn
    losses(fms, rpn_match, target_bbox, count=None, reduction="mean")   RpnLosses on the sampled anchors

    fms: the pyramid levels, float32 NHWC [B,H_l,W_l,C]. With the parameters on a GPU everything runs in the library; with CPU
    parameters, or device="cpu", in numpy and stock torch."""

    def __init__(self, channels: int = 256, anchors_per_location: int = 3, hidden: int = 512):
        super().__init__()
        self.channels, self.anchors_per_location, self.hidden = int(channels), int(anchors_per_location), int(hidden)
        self.conv_shared = nn.Conv2d(self.channels, self.hidden, kernel_size=3, stride=1)
        self.conv_class = nn.Conv2d(self.hidden, 2 * self.anchors_per_location, kernel_size=1, stride=1)
        self.conv_bbox = nn.Conv2d(self.hidden, 4 * self.anchors_per_location, kernel_size=1, stride=1)

    @classmethod
    def from_state_dict(cls, sd: dict, prefix: str = "rpn.") -> "TrainableRPN":
        shared, klass = sd[prefix + "conv_shared.weight"], sd[prefix + "conv_class.weight"]
        rpn = cls(shared.size(1), klass.size(0) // 2, shared.size(0))
        rpn.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})
        return rpn

    # ------------------------------------------------------------------------------------------------------------------
    def _device(self, device) -> torch.device:
        return torch.device(device) if device is not None else self.conv_shared.weight.device

    def _maps(self, fms, dev):
        fms = [f.to(dev) for f in fms]
        b = fms[0].size(0)
        for l, f in enumerate(fms):
            if f.dim() != 4 or f.dtype != torch.float32 or f.size(0) != b or f.size(3) != self.channels:
                raise ValueError(f"TrainableRPN: fms[{l}] must be float32 [{b},H,W,{self.channels}] (NHWC), got {f.dtype} {tuple(f.shape)}")
        return fms

    def _weights(self, dev):
        """(shared OHWI [hidden,3,3,C], its bias, fused head [6*apl,1,1,hidden], its bias) on dev, each with a grad_fn: the permute
        and the concatenation are differentiable, so autograd hands every parameter its own gradient."""
        w_shared = self.conv_shared.weight.to(dev).permute(0, 2, 3, 1).contiguous()
        w_head = torch.cat([self.conv_class.weight, self.conv_bbox.weight], 0).to(dev).permute(0, 2, 3, 1).contiguous()
        b_head = torch.cat([self.conv_class.bias, self.conv_bbox.bias]).to(dev)
        return w_shared, self.conv_shared.bias.to(dev), w_head, b_head

    def dense(self, fms, device=None):
        """rpn_detect (model.py:1294-1304) on whole maps → (fg scores float32 [B,A], deltas float32 [B,A,4]) in anchor order, without a
        graph: ops.conv_bn_act on the exact direct route for the shared conv (SamePad2d(3,1), ReLU) and the fused heads, then
        ops.rpn_scores_deltas on the NHWC head outputs. The library's form takes the five levels P2..P6 and three anchors per
        location. The weights are packed from the current parameters on every call (a Winograd route would have to transform
        them every step as well)."""
        dev = self._device(device)
        apl = self.anchors_per_location
        with torch.no_grad():
            fms = self._maps(fms, dev)
            w_shared, b_shared, w_head, b_head = self._weights(dev)
            if dev.type == "cpu":
                heads = []
                for f in fms:
                    h = torch.relu(torch.nn.functional.conv2d(f.permute(0, 3, 1, 2), self.conv_shared.weight.to(dev), b_shared, padding=1))
                    o = torch.nn.functional.conv2d(h, w_head.permute(0, 3, 1, 2), b_head).permute(0, 2, 3, 1)
                    heads.append(o.reshape(o.size(0), -1, 6 * apl))
                logits = torch.cat([o[..., :2 * apl].reshape(o.size(0), -1, 2) for o in heads], 1)
                deltas = torch.cat([o[..., 2 * apl:].reshape(o.size(0), -1, 4) for o in heads], 1)
                return torch.softmax(logits, dim=2)[..., 1], deltas
            from . import ops
            if len(fms) != 5 or apl != 3:
                raise ValueError(f"TrainableRPN.dense: the library takes the 5 levels P2..P6 with 3 anchors per location, got {len(fms)} "
                                 f"levels with {apl}")
            heads = []
            for f in fms:
                h = ops.conv_bn_act(f.contiguous(), w_shared, None, b_shared, 1, (1, 1, 1, 1), True)
                heads.append(ops.conv_bn_act(h, w_head, None, b_head))
            return ops.rpn_scores_deltas(heads)

    def sampled(self, fms, index: torch.Tensor, num: torch.Tensor, device=None):
        """The RPN on the compacted anchors → (logits float32 [B,K,2], bbox float32 [B,K,4]) with a grad_fn; row (b, k) is what the
        dense graph gives for anchor index[b,k]: pyramid_patches, layers.conv_bn_act on [B*K,1,1,9C] with ReLU (the shared conv as
        a GEMM), layers.conv_bn_act to the fused 6*apl channels, and the selection of anchor r's six values. An empty slot's row is
        the network's value on a zero patch; its match is 0, so no loss reads it. index int32 [B,K] and num int32 [B] as
        ops.anchor_compact returns them."""
        dev = self._device(device)
        apl = self.anchors_per_location
        fms = self._maps(fms, dev)
        index, num = index.to(dev), num.to(dev)
        b, k = index.shape
        w_shared, b_shared, w_head, b_head = self._weights(dev)
        patches = pyramid_patches(fms, index, num, apl)
        w_gemm = w_shared.view(self.hidden, 1, 1, 9 * self.channels)
        if dev.type == "cpu":
            h = torch.relu(patches @ w_gemm.view(self.hidden, -1).t() + b_shared)
            o = h @ w_head.view(6 * apl, -1).t() + b_head
        else:
            from . import layers
            h = layers.conv_bn_act(patches.view(b * k, 1, 1, 9 * self.channels), w_gemm, None, b_shared, act=1)
            o = layers.conv_bn_act(h, w_head, None, b_head).view(b * k, 6 * apl)
        six = _SelectColumns.apply(o, _anchor_columns(index, [tuple(f.shape[1:3]) for f in fms], apl))
        return six[:, :2].reshape(b, k, 2), six[:, 2:].reshape(b, k, 4)

    def losses(self, fms, rpn_match, target_bbox, count: int | None = None, reduction: str = "mean", device=None) -> RpnLosses:
        """RPN.class_loss and RPN.boxes_loss (model.py:652-718) computed, forward and backward, on the anchors with rpn_match != 0
        alone → RpnLosses(rpn_class_loss, rpn_bbox_loss, status). rpn_match [B,A,1] or [B,A] of -1 / 0 / 1 and target_bbox float32
        [B,rows,4] as targets.rpn_targets returns them. count: the capacity of the compaction, by default rows (what sample_by_key
        leaves at most); in 1 .. 1024. The k-th positive in anchor order is still the k-th positive of the compacted row, so it
        meets target_bbox[b,k] as in losses.rpn_losses; the empty slots get match 0. status: bit 0 as losses.rpn_losses (more
        positives than target rows), bit 1 (STATUS_OVERFLOW): the image has more than count anchors with match != 0, and those past
        the first count are left out. Gradients flow into the maps that require one and into the six parameters."""
        dev = self._device(device)
        match = rpn_match if isinstance(rpn_match, torch.Tensor) else torch.from_numpy(np.asarray(rpn_match))
        match = match.to(dev)
        if match.dim() == 3 and match.size(2) == 1:
            match = match.squeeze(2)
        if match.dim() != 2 or match.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"TrainableRPN.losses: rpn_match must be int32 or int64 [B,A,1] or [B,A], got {match.dtype} {tuple(match.shape)}")
        match = match.to(torch.int32).contiguous()
        target_bbox = (target_bbox if isinstance(target_bbox, torch.Tensor) else torch.from_numpy(np.asarray(target_bbox))).to(dev)
        count = int(target_bbox.size(1) if count is None else count)
        first = anchor_firsts([tuple(f.shape[1:3]) for f in fms], self.anchors_per_location)
        if match.size(1) != first[-1]:
            raise ValueError(f"TrainableRPN.losses: rpn_match must have the pyramid's {first[-1]} anchors, got {match.size(1)}")
        if dev.type == "cpu":
            if not 1 <= count <= 1024:
                raise ValueError(f"TrainableRPN.losses: count must be in 1 .. 1024, got {count}")
            index, num, overflow = (torch.from_numpy(v) for v in compact_numpy(match.numpy(), count))
        else:
            from . import ops
            index, num, overflow = ops.anchor_compact(match, count)
        logits, bbox = self.sampled(fms, index, num, device=dev)
        at_index = match.gather(1, index.clamp(min=0).to(torch.int64))
        at_index = torch.where(index >= 0, at_index, torch.zeros_like(at_index))
        out = _losses.rpn_losses(at_index, logits, bbox, target_bbox, reduction=reduction, device=dev)
        return RpnLosses(out.rpn_class_loss, out.rpn_bbox_loss, out.status | (overflow * STATUS_OVERFLOW))
