"""The classifier and mask heads in training mode; the mask branch on the positive slots and on each slot's own class plane alone.

Nothing but Mask.mask_loss (model.py:922-953) carries a gradient into the mask head, and it gathers (positive slot, its class) pairs:
at most int(count * 0.33) of the `count` slots of an image — targets.detection_targets puts them first — and one of conv5's C planes.
The dense graph would run the four 3x3 convs and the deconv on three times the rows, write [B,count,C,28,28] and push a gradient that is
+0 in C - 1 planes of C back through the 1x1 conv. Here

    heads = TrainableHeads(TrainableClassifier.from_state_dict(sd, image_area=area), TrainableMask.from_state_dict(sd, image_area=area)).to("cuda")
    t = targets.detection_targets(rois, gt_boxes, gt_class_ids, gt_masks)
    out = heads.losses(fms, t)                                   # losses.HeadLosses, with a grad_fn
    (out.class_loss + out.bbox_loss + out.mask_loss).backward()  # gradients in the four maps and every head parameter

and the mask branch is: RoIAlign at pool 14 of the first P = mask_slots slots, the four 3x3 convs and the deconv as layers.conv_bn_act /
layers.deconv2x2 on those B * P slots, then class_plane_conv (the 1x1 conv to the slot's class, sigmoid) and mask_plane_loss
(csrc/mask_train.hip; the rules are stated at mrcnn_class_plane_conv_f32 in include/maskrcnn_hip.h). The classifier is composition:
RoIAlign at pool 7 on all slots with roi_counts, three layers.conv_bn_act GEMMs with row_counts, losses.classifier_losses. BatchNorm is
frozen: it is folded into (scale, shift) by modules.fold_bn on every call from the current buffers and gets no gradient; a conv bias gets
its gradient through the shift. Nothing in that path synchronises with the host.

The trunk runs DENSE on the P slots: a slot past num_pos is pooled and computed like any other (its RoI is a negative's box or zeros, so
every value is finite) and never used — class_plane_conv hands it a +0 gradient. layers.deconv2x2 takes no row counts, and rows left
unwritten in front of it would reach its weight gradient as 0 * NaN.

CPU tensors run the two new rules in numpy (class_plane_conv_numpy, class_plane_backward_numpy, mask_plane_terms_numpy below) and the
layers in stock torch; RoIAlign has no CPU form, so on the CPU the heads start at the pooled crops (TrainableMask.planes_from_pooled,
TrainableClassifier.head).
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import layers as _layers
from . import losses as _losses
from . import modules as _modules
from .losses import HeadLosses, MAX_CLASSES

__all__ = ["class_plane_conv", "mask_plane_loss", "TrainableClassifier", "TrainableMask", "TrainableHeads", "class_plane_conv_numpy",
           "class_plane_backward_numpy", "mask_plane_terms_numpy", "plane_status_numpy", "STATUS_BAD_CLASS", "STATUS_NO_ROOM"]

STATUS_BAD_CLASS = 2     # bit 1: a class id outside 0 .. C-1 in a slot below num (losses.head_losses' bit)
STATUS_NO_ROOM = 4       # bit 2: a positive at or past slot P below num: the planes have no room for it, it is left out
_PIXELS, _WAVES, _LANES, _THREADS = 64, 4, 64, 256


# ----------------------------------------------------------------------------------------------------------------------
# The rules in numpy
# ----------------------------------------------------------------------------------------------------------------------
def _active(ids, num, slots: int, classes: int):
    """ids [B,count], num [B] → (active bool [B,P], class int64 [B,P])."""
    ids, num = np.asarray(ids).astype(np.int64), np.asarray(num).astype(np.int64)
    b, count = ids.shape
    n = np.minimum(np.clip(num, 0, count), slots)
    k = ids[:, :slots]
    return (np.arange(slots)[None, :] < n[:, None]) & (k > 0) & (k < classes), k


def plane_status_numpy(ids, num, slots: int, classes: int) -> np.ndarray:
    """status int32 [B]: STATUS_BAD_CLASS for a class id outside 0 .. C-1 below num[b], STATUS_NO_ROOM for a positive at or past slot P."""
    ids, num = np.asarray(ids).astype(np.int64), np.asarray(num).astype(np.int64)
    b, count = ids.shape
    below = np.arange(count)[None, :] < np.clip(num, 0, count)[:, None]
    bad = (below & ((ids < 0) | (ids >= classes))).any(axis=1)
    over = (below & (ids > 0) & (np.arange(count)[None, :] >= slots)).any(axis=1)
    return (STATUS_BAD_CLASS * bad + STATUS_NO_ROOM * over).astype(np.int32)


def _ordered_dot(x: np.ndarray, wk: np.ndarray) -> np.ndarray:
    """x float32 [Q,Cin], wk float32 [Cin] → float64 [Q]: the exact products summed in the kernel's order — lane l of 64 adds the channels
    4 (l + 64 i) + j, i outer, j inner, from +0; then v[l] += v[l ^ d] for d = 32 .. 1."""
    prod = x.astype(np.float64) * wk.astype(np.float64)[None, :]
    q, cin = prod.shape
    groups = -(-cin // (4 * _LANES))
    padded = np.zeros((q, groups * 4 * _LANES))
    padded[:, :cin] = prod
    padded = padded.reshape(q, groups, _LANES, 4)
    acc = np.zeros((q, _LANES))
    for i in range(groups):
        for j in range(4):
            acc = acc + padded[:, i, :, j]
    lanes = np.arange(_LANES)
    for d in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ d]
    return acc[:, 0]


def class_plane_conv_numpy(x, w, bias, ids, num, act: int = 0):
    """mrcnn_class_plane_conv_f32 in numpy: x float32 [B*P,mh,mw,Cin], w float32 [C,Cin], bias float32 [C] or None, ids [B,count], num [B]
    → (y float32 [B*P,mh,mw], z float32 the same shape: the pre-activation, status int32 [B]). z is the kernel's, bit for bit; y at
    act 2 goes through numpy's exp, which need not round as the device's expf does."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    s, mh, mw, cin = x.shape
    b = np.asarray(ids).shape[0]
    slots, classes = s // b, w.shape[0]
    on, k = _active(ids, num, slots, classes)
    z = np.zeros((s, mh * mw), np.float32)
    for i in np.flatnonzero(on.reshape(-1)):
        cls = int(k.reshape(-1)[i])
        total = _ordered_dot(x[i].reshape(mh * mw, cin), w[cls])
        z[i] = (np.float64(np.asarray(bias, np.float32)[cls]) + total if bias is not None else total).astype(np.float32)
    y = z
    if act == 2:
        with np.errstate(over="ignore"):
            y = np.where(on.reshape(-1)[:, None], np.float32(1) / (np.float32(1) + np.exp(-z)), np.float32(0)).astype(np.float32)
    return y.reshape(s, mh, mw), z.reshape(s, mh, mw), plane_status_numpy(ids, num, slots, classes)


def _ordered_pixel_sum(terms: np.ndarray) -> np.ndarray:
    """terms float64 [Q,n] → float64 [n]: chunks of 64 pixels; within a chunk v = 0 .. 3 adds the pixels v + 4 j from +0, the four are added
    ((v0 + v1) + v2) + v3, and the chunk sums from +0 in ascending chunk."""
    q, n = terms.shape
    chunks = -(-q // _PIXELS)
    padded = np.zeros((chunks * _PIXELS, n))
    padded[:q] = terms
    padded = padded.reshape(chunks, _PIXELS // _WAVES, _WAVES, n)
    wave = np.zeros((chunks, _WAVES, n))
    for j in range(_PIXELS // _WAVES):
        wave = wave + padded[:, j]
    chunk = ((wave[:, 0] + wave[:, 1]) + wave[:, 2]) + wave[:, 3]
    total = np.zeros(n)
    for c in range(chunks):
        total = total + chunk[c]
    return total


def class_plane_backward_numpy(dy, y, x, w, ids, num, act: int = 0):
    """mrcnn_class_plane_conv_backward_f32 in numpy → (dx float32 [B*P,mh,mw,Cin], dw float32 [C,Cin], dbias float32 [C]), bit for bit
    (y: the forward's own output at act 2; ignored at act 0)."""
    dy, x, w = np.asarray(dy, np.float32), np.asarray(x, np.float32), np.asarray(w, np.float32)
    s, mh, mw, cin = x.shape
    b = np.asarray(ids).shape[0]
    slots, classes = s // b, w.shape[0]
    on, k = _active(ids, num, slots, classes)
    dx = np.zeros(x.shape, np.float32)
    dw, db = np.zeros((classes, cin)), np.zeros(classes)
    for i in np.flatnonzero(on.reshape(-1)):                       # ascending (b, s)
        cls = int(k.reshape(-1)[i])
        g = dy[i].reshape(-1)
        if act == 2:
            v = np.asarray(y, np.float32)[i].reshape(-1)
            t = np.float32(1) - v
            u = v * t
            g = g * u
        dx[i] = (g[:, None] * w[cls][None, :]).reshape(mh, mw, cin)
        g64 = g.astype(np.float64)[:, None]
        dw[cls] = dw[cls] + _ordered_pixel_sum(g64 * x[i].reshape(mh * mw, cin).astype(np.float64))
        db[cls] = db[cls] + _ordered_pixel_sum(g64)[0]
    return dx, dw.astype(np.float32), db.astype(np.float32)


def _workgroup_sum(terms: np.ndarray) -> np.float64:
    """A slot's terms float64 [Q] in the order of the loss kernels: thread t of 256 adds elements t, t + 256, .. from +0; each wave's 64
    thread sums meet in the shuffle scan (lane 63's value); the four wave sums are added in wave order."""
    q = terms.shape[0]
    rows = -(-q // _THREADS)
    padded = np.zeros(rows * _THREADS)
    padded[:q] = terms
    v = np.zeros(_THREADS)
    for r in padded.reshape(rows, _THREADS):
        v = v + r
    v = v.reshape(_WAVES, _LANES)
    lanes = np.arange(_LANES)
    for d in (1, 2, 4, 8, 16, 32):
        up = np.concatenate([np.zeros((_WAVES, d)), v[:, :-d]], axis=1)
        v = np.where(lanes[None, :] >= d, v + up, v)
    total = np.float64(0)
    for wv in range(_WAVES):
        total = total + v[wv, _LANES - 1]
    return total


def mask_plane_terms_numpy(p, target_mask, ids, num, classes: int = MAX_CLASSES):
    """mrcnn_mask_plane_loss_forward in numpy: p float32 [B,P,mh,mw], target_mask float32 [B,count,mh,mw], ids [B,count], num [B] →
    (sums float64 [B], counts int64 [B], status int32 [B], derivative float64 [B,P,mh,mw]: each element's, 0 for a slot that is not
    active, not yet divided by a count). The summation order is the kernels'; log and log1p are numpy's."""
    p, tm = np.asarray(p, np.float32), np.asarray(target_mask, np.float32)
    b, slots, mh, mw = p.shape
    on, _ = _active(ids, num, slots, classes)
    sums, counts, deriv = np.zeros(b), np.zeros(b, np.int64), np.zeros(p.shape)
    for i in range(b):
        for s in range(slots):                                     # slot order
            if on[i, s]:
                term, deriv[i, s] = _losses._binary_cross_entropy(p[i, s].astype(np.float64), tm[i, s].astype(np.float64))
                sums[i] = sums[i] + _workgroup_sum(term.reshape(-1))
                counts[i] += mh * mw
    return sums, counts, plane_status_numpy(ids, num, slots, classes), deriv


# ----------------------------------------------------------------------------------------------------------------------
# autograd
# ----------------------------------------------------------------------------------------------------------------------
class _ClassPlaneConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, ids, num, act):
        x, w = x.contiguous(), w.contiguous()
        if x.is_cuda:
            from . import ops
            y, status = ops.class_plane_conv(x, w, bias, ids, num, act)
        else:
            y, _, status = class_plane_conv_numpy(x.detach().numpy(), w.detach().numpy(), None if bias is None else bias.detach().numpy(),
                                                  ids.numpy(), num.numpy(), act)
            y, status = torch.from_numpy(y), torch.from_numpy(status)
        ctx.save_for_backward(x, w, ids, num, y if act else None)
        ctx.act = act
        ctx.mark_non_differentiable(status)
        return y, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad, _):
        x, w, ids, num, y = ctx.saved_tensors
        needs = ctx.needs_input_grad[:3]
        if grad.is_cuda:
            from . import ops
            dx, dw, db = ops.class_plane_conv_backward(grad.contiguous(), y, x, w, ids, num, ctx.act, needs=needs)
        else:
            got = class_plane_backward_numpy(grad.contiguous().numpy(), None if y is None else y.numpy(), x.numpy(), w.numpy(), ids.numpy(),
                                             num.numpy(), ctx.act)
            dx, dw, db = (torch.from_numpy(g) if need else None for g, need in zip(got, needs))
        return dx, dw, db, None, None, None


class _MaskPlaneLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, target_mask, ids, num, classes, per_image):
        p = p.contiguous()
        ctx.call = (classes, per_image)
        if p.is_cuda:
            from . import ops
            sums, counts, status = ops.mask_plane_loss(p, target_mask, ids, num, classes)
            ctx.save_for_backward(p, target_mask, ids, num, counts)
            loss = _losses._reduce_device(sums[:, None], counts[:, None], per_image)[..., 0]
        else:
            sums, counts, status, ctx.deriv = mask_plane_terms_numpy(p.detach().numpy(), target_mask.numpy(), ids.numpy(), num.numpy(), classes)
            loss, ctx.denominators = _losses.reduce_numpy(sums[:, None], counts[:, None], "per_image" if per_image else "mean")
            loss, status = torch.from_numpy(np.ascontiguousarray(loss[..., 0])), torch.from_numpy(status)
        ctx.mark_non_differentiable(status)
        return loss, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _):
        classes, per_image = ctx.call
        if grad_loss.is_cuda:
            from . import ops
            p, target_mask, ids, num, counts = ctx.saved_tensors
            grad = ops.mask_plane_loss_backward(p, target_mask, ids, num, classes, counts, grad_loss.to(torch.float32).reshape(-1).contiguous(),
                                                per_image)
        else:
            go = grad_loss.detach().numpy().astype(np.float64).reshape(-1, 1)
            grad = torch.from_numpy(_losses._scaled([ctx.deriv], ctx.denominators, go if per_image else go[0])[0])
        return grad, None, None, None, None, None


def _targets(who, ids, num, dev):
    ids = (ids if isinstance(ids, torch.Tensor) else torch.from_numpy(np.asarray(ids))).to(dev)
    num = (num if isinstance(num, torch.Tensor) else torch.from_numpy(np.asarray(num))).to(dev)
    if ids.dim() != 2 or ids.dtype not in (torch.int32, torch.int64) or tuple(num.shape) != (ids.size(0),):
        raise ValueError(f"{who}: ids must be int32 or int64 [B,count] and num [B], got {ids.dtype} {tuple(ids.shape)} and {tuple(num.shape)}")
    return ids.to(torch.int32).contiguous(), num.to(torch.int32).contiguous()


def class_plane_conv(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None, ids, num, act: int = 0):
    """The 1x1 conv to each slot's own class with a grad_fn → (y float32 [B*P,mh,mw], status int32 [B]). x float32 [B*P,mh,mw,Cin] (NHWC,
    Cin % 4 == 0), w float32 [C,Cin], bias float32 [C] or None, ids int [B,count] (target_class_ids), num int [B], act 0 none / 2 sigmoid.
    Slot (b, s) is active when s < min(num[b], P) and 0 < ids[b,s] < C; a slot that is not is +0 in y and in the gradient of x, and its
    rows are never read. Gradients for x, w and bias: ops.class_plane_conv_backward, deterministic. CPU tensors run the numpy rules."""
    ids, num = _targets("class_plane_conv", ids, num, x.device)
    return _ClassPlaneConv.apply(x, w, bias, ids, num, int(act))


def mask_plane_loss(p: torch.Tensor, target_mask: torch.Tensor, ids, num, reduction: str = "mean", num_classes: int = MAX_CLASSES):
    """Mask.mask_loss on class planes with a grad_fn → (loss float32, 0-dim or [B] for "per_image"; status int32 [B]). p float32
    [B,P,mh,mw], target_mask float32 [B,count,mh,mw], ids int [B,count], num int [B]; the active slots are class_plane_conv's for
    C = num_classes. The loss is the batch's sum / the batch's count ("mean") or each image's own; 0 with zero gradients when empty. The
    gradient goes to p."""
    per_image = _losses._check_reduction("mask_plane_loss", reduction)
    ids, num = _targets("mask_plane_loss", ids, num, p.device)
    return _MaskPlaneLoss.apply(p, target_mask.to(p.device, torch.float32).contiguous(), ids, num, int(num_classes), per_image)


# ----------------------------------------------------------------------------------------------------------------------
# The heads
# ----------------------------------------------------------------------------------------------------------------------
def _frozen_bn(channels: int, momentum: float = 0.1) -> nn.BatchNorm2d:
    bn = nn.BatchNorm2d(channels, eps=_modules.BN_EPS, momentum=momentum)
    for p in bn.parameters():
        p.requires_grad_(False)
    return bn


class _Head(nn.Module):
    def _state(self) -> dict:
        return {**dict(self.named_parameters()), **dict(self.named_buffers())}

    def _device(self, device) -> torch.device:
        return torch.device(device) if device is not None else next(self.parameters()).device

    def _maps(self, fms, dev):
        fms = [f.to(dev) for f in fms]
        if len(fms) != 4 or any(f.dim() != 4 or f.dtype != torch.float32 or f.size(3) != self.depth for f in fms):
            raise ValueError(f"{type(self).__name__}: fms must be the 4 float32 NHWC maps P2..P5 with {self.depth} channels, got "
                             f"{[tuple(f.shape) for f in fms]}")
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__}: RoIAlign has no CPU form; on the CPU start at the pooled crops")
        return [f.contiguous() for f in fms]

    @classmethod
    def from_state_dict(cls, sd: dict, prefix: str, **kwargs):
        head = cls(**cls._shape_of(sd, prefix), **kwargs)
        head.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})
        return head


class TrainableClassifier(_Head):
    """Classifier (model.py:724-800) with the reference's parameter names and layouts: conv1.weight [hidden,depth,pool,pool], conv2.weight
    [hidden,hidden,1,1], bn1 / bn2 (frozen), linear_class [C,hidden], linear_bbox [4C,hidden]. The modules hold parameters only.

    forward(fms, rois, num_rois)   (logits [B,count,C], bbox [B,count,C,4]) with a grad_fn; rois float32 [B,count,4] normalised
    head(pooled, num_rois)         the same from the crops [B*count,pool,pool,depth]; runs on the CPU too (stock torch)
    losses(fms, t, reduction)      (class_loss, bbox_loss, status) for t a targets.DetectionTargets

    Rows of the slots at or past num_rois[b] hold unspecified values: RoIAlign and the three GEMMs skip them (roi_counts / row_counts),
    and no loss reads them."""

    def __init__(self, depth: int = 256, pool: int = 7, num_classes: int = 81, hidden: int = 1024, image_area: float = 1024.0 * 1024.0):
        super().__init__()
        self.depth, self.pool, self.num_classes, self.hidden, self.image_area = int(depth), int(pool), int(num_classes), int(hidden), float(image_area)
        self.conv1 = nn.Conv2d(self.depth, self.hidden, kernel_size=self.pool, stride=1)
        self.bn1 = _frozen_bn(self.hidden, 0.01)
        self.conv2 = nn.Conv2d(self.hidden, self.hidden, kernel_size=1, stride=1)
        self.bn2 = _frozen_bn(self.hidden, 0.01)
        self.linear_class = nn.Linear(self.hidden, self.num_classes)
        self.linear_bbox = nn.Linear(self.hidden, 4 * self.num_classes)

    @staticmethod
    def _shape_of(sd, prefix):
        w = sd[prefix + "conv1.weight"]
        return dict(depth=w.size(1), pool=w.size(2), hidden=w.size(0), num_classes=sd[prefix + "linear_class.weight"].size(0))

    @classmethod
    def from_state_dict(cls, sd: dict, prefix: str = "classifier.", **kwargs) -> "TrainableClassifier":
        return super().from_state_dict(sd, prefix, **kwargs)

    def head(self, pooled: torch.Tensor, num_rois: torch.Tensor | None = None, rois_per_image: int = 0, device=None):
        dev = self._device(device)
        pooled = pooled.to(dev)
        r, c = pooled.size(0), self.num_classes
        sd = self._state()
        s1, t1 = _modules.fold_bn(sd, "conv1", "bn1", dev)
        s2, t2 = _modules.fold_bn(sd, "conv2", "bn2", dev)
        w1 = self.conv1.weight.to(dev).permute(0, 2, 3, 1).reshape(self.hidden, 1, 1, -1)
        w2 = self.conv2.weight.to(dev).permute(0, 2, 3, 1).contiguous()
        w_fc = torch.cat([self.linear_class.weight, self.linear_bbox.weight], 0).to(dev)
        b_fc = torch.cat([self.linear_class.bias, self.linear_bbox.bias]).to(dev)
        x = pooled.reshape(r, 1, 1, -1)
        if dev.type == "cpu":
            h = torch.relu((x.view(r, -1) @ w1.view(self.hidden, -1).t()) * s1 + t1)
            h = torch.relu((h @ w2.view(self.hidden, -1).t()) * s2 + t2)
            y = h @ w_fc.t() + b_fc
        else:
            rc = {} if num_rois is None else dict(row_counts=num_rois.to(dev, torch.int32).contiguous(), rows_per_group=int(rois_per_image))
            h = _layers.conv_bn_act(x, w1.contiguous(), s1, t1, act=1, **rc)
            h = _layers.conv_bn_act(h, w2, s2, t2, act=1, **rc)
            y = _layers.conv_bn_act(h, w_fc.view(5 * c, 1, 1, self.hidden), None, b_fc, **rc).view(r, 5 * c)
        return y[:, :c], y[:, c:].reshape(r, c, 4)

    def forward(self, fms, rois: torch.Tensor, num_rois: torch.Tensor, device=None):
        dev = self._device(device)
        fms = self._maps(fms, dev)
        from . import ops
        b, count = rois.shape[:2]
        num_rois = num_rois.to(dev, torch.int32).contiguous()
        pooled = ops.roi_align_pyramid(fms, rois.to(dev, torch.float32).reshape(b * count, 4).contiguous(), self.pool, self.image_area,
                                       rois_per_image=count, roi_counts=num_rois)
        logits, bbox = self.head(pooled, num_rois, count, device=dev)
        return logits.reshape(b, count, -1), bbox.reshape(b, count, -1, 4)

    def losses(self, fms, t, reduction: str = "mean", device=None):
        logits, bbox = self.forward(fms, t.rois, t.num_pos + t.num_neg, device=device)
        return _losses.classifier_losses(t, logits, bbox, reduction=reduction, device=self._device(device))


class TrainableMask(_Head):
    """Mask (model.py:848-920) with the reference's parameter names and layouts: conv1 .. conv4.weight [depth,depth,3,3] with bn1 .. bn4
    (frozen), deconv.weight [depth,depth,2,2] (ConvTranspose2d: [Cin,Cout,2,2]), conv5.weight [C,depth,1,1]. The modules hold parameters
    only.

    planes(fms, t)                         p float32 [B,P,2 pool,2 pool]: the sigmoid plane of each of the first P slots' own class
    planes_from_pooled(pooled, ids, num)   (p, status) from the crops [B*P,pool,pool,depth]; runs on the CPU too
    losses(fms, t, reduction)              (mask_loss, status)

    P = mask_slots: by default int(count * positive_ratio), what detection_targets leaves positive at most. status: STATUS_BAD_CLASS,
    STATUS_NO_ROOM (an image with more than P positives: those past P are left out of the loss)."""

    def __init__(self, depth: int = 256, pool: int = 14, num_classes: int = 81, image_area: float = 1024.0 * 1024.0,
                 mask_slots: int | None = None, positive_ratio: float = 0.33):
        super().__init__()
        self.depth, self.pool, self.num_classes, self.image_area = int(depth), int(pool), int(num_classes), float(image_area)
        self.mask_slots, self.positive_ratio = mask_slots, float(positive_ratio)
        for i in (1, 2, 3, 4):
            setattr(self, f"conv{i}", nn.Conv2d(self.depth, self.depth, kernel_size=3, stride=1))
            setattr(self, f"bn{i}", _frozen_bn(self.depth))
        self.deconv = nn.ConvTranspose2d(self.depth, self.depth, kernel_size=2, stride=2)
        self.conv5 = nn.Conv2d(self.depth, self.num_classes, kernel_size=1, stride=1)

    @staticmethod
    def _shape_of(sd, prefix):
        return dict(depth=sd[prefix + "conv1.weight"].size(1), num_classes=sd[prefix + "conv5.weight"].size(0))

    @classmethod
    def from_state_dict(cls, sd: dict, prefix: str = "mask.", **kwargs) -> "TrainableMask":
        return super().from_state_dict(sd, prefix, **kwargs)

    def slots(self, count: int) -> int:
        p = int(count * self.positive_ratio) if self.mask_slots is None else int(self.mask_slots)
        if not 1 <= p <= count:
            raise ValueError(f"TrainableMask: mask_slots={p} must be in 1 .. count = {count}")
        return p

    def trunk(self, pooled: torch.Tensor, device=None) -> torch.Tensor:
        """The four 3x3 convs + BN + ReLU and the deconv + ReLU on crops [S,pool,pool,depth] → [S,2 pool,2 pool,depth], NHWC."""
        dev = self._device(device)
        x = pooled.to(dev)
        sd = self._state()
        w_de = self.deconv.weight.to(dev).permute(2, 3, 1, 0).reshape(4 * self.depth, 1, 1, self.depth)
        for i in (1, 2, 3, 4):
            scale, shift = _modules.fold_bn(sd, f"conv{i}", f"bn{i}", dev)
            w = getattr(self, f"conv{i}").weight.to(dev)
            if dev.type == "cpu":
                z = F.conv2d(x.permute(0, 3, 1, 2), w, None, padding=1).permute(0, 2, 3, 1)
                x = torch.relu(z * scale + shift)
            else:
                x = _layers.conv_bn_act(x.contiguous(), w.permute(0, 2, 3, 1).contiguous(), scale, shift, (1, 1, 1, 1), 1)
        if dev.type == "cpu":
            y = F.conv_transpose2d(x.permute(0, 3, 1, 2), self.deconv.weight.to(dev), self.deconv.bias.to(dev), stride=2)
            return torch.relu(y).permute(0, 2, 3, 1).contiguous()
        return _layers.deconv2x2(x, w_de.contiguous(), self.deconv.bias.to(dev).repeat(4), 1)

    def planes_from_pooled(self, pooled: torch.Tensor, ids, num, device=None):
        dev = self._device(device)
        x = self.trunk(pooled, device=dev)
        return class_plane_conv(x, self.conv5.weight.to(dev).view(self.num_classes, self.depth), self.conv5.bias.to(dev), ids, num, act=2)

    def _planes(self, fms, t, dev):
        fms = self._maps(fms, dev)
        from . import ops
        b, count = t.rois.shape[:2]
        p = self.slots(count)
        rois = t.rois.to(dev, torch.float32)[:, :p].reshape(b * p, 4).contiguous()
        pooled = ops.roi_align_pyramid(fms, rois, self.pool, self.image_area, rois_per_image=p)
        planes, status = self.planes_from_pooled(pooled, t.target_class_ids, t.num_pos + t.num_neg, device=dev)
        return planes.view(b, p, planes.size(1), planes.size(2)), status

    def planes(self, fms, t, device=None) -> torch.Tensor:
        return self._planes(fms, t, self._device(device))[0]

    def losses(self, fms, t, reduction: str = "mean", device=None):
        planes, _ = self._planes(fms, t, self._device(device))
        return mask_plane_loss(planes, t.target_mask, t.target_class_ids, t.num_pos + t.num_neg, reduction, self.num_classes)


class TrainableHeads(nn.Module):
    """The two heads behind one call: losses(fms, t, reduction="mean") → losses.HeadLosses(class_loss, bbox_loss, mask_loss, status) for
    the NHWC maps P2 .. P5 and t a targets.DetectionTargets whose RoIs are in the coordinates ops.roi_align_pyramid takes. Gradients reach
    the four maps and every head parameter; status ORs the classifier losses' bits and the mask branch's."""

    def __init__(self, classifier: TrainableClassifier, mask: TrainableMask):
        super().__init__()
        self.classifier, self.mask = classifier, mask

    def losses(self, fms, t, reduction: str = "mean", device=None) -> HeadLosses:
        class_loss, bbox_loss, status = self.classifier.losses(fms, t, reduction, device)
        mask_loss, mask_status = self.mask.losses(fms, t, reduction, device)
        return HeadLosses(class_loss, bbox_loss, mask_loss, status | mask_status)
