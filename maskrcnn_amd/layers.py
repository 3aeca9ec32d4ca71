"""Differentiable forms of the model's building blocks — what train_model trains in any of its schedules (model.py:1010-1016: "heads"
is fpn.P*, rpn.*, classifier.*, mask.*; "3+" … "all" add the ResNet stages and the stem; BatchNorm frozen and in eval mode in all of
them): every such layer is an fp32 NHWC conv with the fused epilogue act(scale * conv + shift (+ residual)) at stride 1 or 2, the 2x2
transposed conv, the zero-padded max-pool, or a whole Bottleneck.

    conv_bn_act(x, w, scale, shift, pad, act, residual, res_div, row_counts, rows_per_group, stride)
    deconv2x2(x, w4, bias4, act)
    maxpool(x, kernel, stride, pad)
    bottleneck(x, w1, s1, t1, w2, s2, t2, w3, s3, t3, wd, sd, td, stride)

The forward is the existing exact-fp32 direct launch (ops.conv_bn_act / ops.deconv2x2 / ops.maxpool, unchanged: those calls save
nothing and return tensors without a grad_fn); the backward is ops.conv_bn_act_backward (csrc/conv_backward.hip), ops.dilate2_sum and
ops.maxpool_backward (csrc/pool_backward.hip). Gradients go to x, w, shift / bias4 and the residual. `scale` gets none: BatchNorm is
frozen in every schedule."""
from __future__ import annotations

import torch

from . import ops


class _ConvBnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, scale, shift, residual, row_counts, pad, act, res_div, rows_per_group, stride):
        x, w = x.contiguous(), w.contiguous()
        residual = None if residual is None else residual.contiguous()
        y = ops.conv_bn_act(x, w, scale, shift, stride, pad, act, residual, res_div, row_counts=row_counts, rows_per_group=rows_per_group)
        ctx.save_for_backward(x, w, scale, y if act else None, row_counts)
        ctx.call = (pad, act, res_div if residual is not None else 0, rows_per_group, stride)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, w, scale, y, row_counts = ctx.saved_tensors
        pad, act, res_div, rows_per_group, stride = ctx.call
        need = ctx.needs_input_grad
        r = ops.conv_bn_act_backward(grad, x, w, y, scale, pad, act, res_div, False, row_counts, rows_per_group,
                                     needs=(need[0], need[1], need[3], need[4] and res_div != 0), stride=stride)
        dx = r.dx
        if stride == 2 and dx is not None:
            dx = ops.dilate2_sum(dx, None, x.size(1), x.size(2))
        return dx, r.dw, None, r.dshift, r.dresidual, None, None, None, None, None, None


class _Deconv2x2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w4, bias4, act):
        x, w4 = x.contiguous(), w4.contiguous()
        y = ops.deconv2x2(x, w4, bias4.contiguous(), act)
        ctx.save_for_backward(x, w4, y if act else None)
        ctx.act = act
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, w4, y = ctx.saved_tensors
        need = ctx.needs_input_grad
        r = ops.conv_bn_act_backward(grad, x, w4, y, None, (0, 0, 0, 0), ctx.act, 0, True, needs=(need[0], need[1], need[2], False))
        return r.dx, r.dw, r.dshift, None


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, stride, pad):
        x = x.contiguous()
        y = ops.maxpool(x, kernel, stride, pad)
        ctx.call = (kernel, stride, pad)
        if (kernel, stride, pad) == (1, 2, (0, 0, 0, 0)):      # P6: a window of one tap always takes it, the input is not needed
            ctx.size = (x.size(1), x.size(2))
        else:
            ctx.save_for_backward(x)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        kernel, stride, pad = ctx.call
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        if not ctx.saved_tensors:
            return ops.dilate2_sum(grad, None, *ctx.size), None, None, None
        return ops.maxpool_backward(grad, ctx.saved_tensors[0], kernel, stride, pad), None, None, None


class _Bottleneck(torch.autograd.Function):
    """Inputs: 0 x; 1-3 w1 s1 t1; 4-6 w2 s2 t2; 7-9 w3 s3 t3; 10-12 wd sd td; 13 stride."""

    @staticmethod
    def forward(ctx, x, w1, s1, t1, w2, s2, t2, w3, s3, t3, wd, sd, td, stride):
        x = x.contiguous()
        w1, w2, w3 = w1.contiguous(), w2.contiguous(), w3.contiguous()
        wd = None if wd is None else wd.contiguous()
        res = x if wd is None else ops.conv_bn_act(x, wd, sd, td, stride, relu=False)
        h1 = ops.conv_bn_act(x, w1, s1, t1, stride, relu=True)
        h2 = ops.conv_bn_act(h1, w2, s2, t2, 1, (1, 1, 1, 1), True)
        y = ops.conv_bn_act(h2, w3, s3, t3, 1, relu=True, residual=res)
        ctx.save_for_backward(x, h1, h2, y, w1, s1, w2, s2, w3, s3, wd, sd)
        ctx.stride = stride
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, h1, h2, y, w1, s1, w2, s2, w3, s3, wd, sd = ctx.saved_tensors
        need, stride, none = ctx.needs_input_grad, ctx.stride, (0, 0, 0, 0)
        need_x, need_w1, need_t1, need_w2, need_t2 = need[0], need[1], need[3], need[4], need[6]
        need_wd, need_td = wd is not None and need[10], wd is not None and need[12]
        need_h1 = need_x or need_w1 or need_t1                   # the gradient of conv1's output
        need_h2 = need_h1 or need_w2 or need_t2                  # ... of conv2's output
        need_g = need_x or need_wd or need_td                    # ... of the residual branch
        r3 = ops.conv_bn_act_backward(grad, h2, w3, y, s3, none, 1, 1, needs=(need_h2, need[7], need[9], need_g))
        g = r3.dresidual
        r2 = ops.conv_bn_act_backward(r3.dx, h1, w2, h2, s2, (1, 1, 1, 1), 1, needs=(need_h1, need_w2, need_t2, False)) if need_h2 else None
        r1 = ops.conv_bn_act_backward(r2.dx, x, w1, h1, s1, none, 1, needs=(need_x, need_w1, need_t1, False), stride=stride) if need_h1 else None
        rd = None
        if wd is not None and need_g:
            rd = ops.conv_bn_act_backward(g, x, wd, None, sd, none, 0, needs=(need_x, need_wd, need_td, False), stride=stride)
        dx = None
        if need_x and stride == 2:
            dx = ops.dilate2_sum(r1.dx, rd.dx, x.size(1), x.size(2))
        elif need_x:
            dx = r1.dx + (g if wd is None else rd.dx)
        pick = lambda r, name: None if r is None else getattr(r, name)
        return (dx, pick(r1, "dw"), None, pick(r1, "dshift"), pick(r2, "dw"), None, pick(r2, "dshift"), r3.dw, None, r3.dshift,
                pick(rd, "dw"), None, pick(rd, "dshift"), None)


def conv_bn_act(x: torch.Tensor, w: torch.Tensor, scale: torch.Tensor | None = None, shift: torch.Tensor | None = None,
                pad=(0, 0, 0, 0), act: int = 0, residual: torch.Tensor | None = None, res_div: int = 1,
                row_counts: torch.Tensor | None = None, rows_per_group: int = 0, stride: int = 1) -> torch.Tensor:
    """y = act(scale * conv(x, w) + shift (+ residual)) with a grad_fn: x [B,H,W,Cin] NHWC float32 (Cin % 4 == 0),
    w [Cout,KH,KW,Cin], scale / shift [Cout] or None, pad = (top, left, bottom, right) each at most the kernel size - 1, act 0 none /
    1 ReLU / 2 sigmoid, residual [B,OH/res_div,OW/res_div,Cout] with res_div 1 or 2, row_counts / rows_per_group as ops.conv_bn_act
    takes them (stride 1 only). stride 1 or 2: at stride 2 the gradient of x exists for a 1x1 kernel without padding (the first block
    of C3 / C4 / C5; ops.dilate2_sum writes it out from the compact form), the gradients of w and shift for any kernel (the stem's
    7x7, whose input is the image). Gradients for x, w, shift and residual; none for scale."""
    stride = int(stride)
    if stride not in (1, 2):
        ops.refuse("conv_bn_act", "stride", "1 or 2", stride)
    return _ConvBnAct.apply(x, w, scale, shift, residual, row_counts, tuple(int(v) for v in pad), int(act), int(res_div),
                            int(rows_per_group), stride)


def deconv2x2(x: torch.Tensor, w4: torch.Tensor, bias4: torch.Tensor, act: int = 0) -> torch.Tensor:
    """The 2x2 stride-2 transposed conv + bias + activation with a grad_fn: x [B,H,W,Cin], w4 [4*C,1,1,Cin] (row (dy*2+dx)*C + co),
    bias4 [4*C] (the bias once per tap: a caller that makes it with bias.repeat(4) gets the four taps added by autograd) →
    [B,2H,2W,C]. act 0 none / 1 ReLU. Gradients for x, w4 and bias4."""
    return _Deconv2x2.apply(x, w4, bias4, int(act))


def maxpool(x: torch.Tensor, kernel: int, stride: int, pad=(0, 0, 0, 0)) -> torch.Tensor:
    """The zero-padded max-pool with a grad_fn: x [B,H,W,C] NHWC float32 (C % 4 == 0), kernel 1 .. 3, stride 1 .. 2, pad = (top,
    left, bottom, right) each at most kernel - 1 (the stem: kernel 3, stride 2, pad = ops.same_pad(H, W, 3, 2); P6: kernel 1, stride
    2). The forward is ops.maxpool; the backward recomputes each window's first maximum from x (ops.maxpool_backward: a window whose
    maximum is a padding zero drops its gradient), and P6, whose windows have one tap, goes through ops.dilate2_sum."""
    kernel, stride, pad = int(kernel), int(stride), tuple(int(v) for v in pad)
    if not 1 <= kernel <= 3:
        ops.refuse("maxpool", "kernel", "an int in 1 .. 3", kernel)
    if not 1 <= stride <= 2:
        ops.refuse("maxpool", "stride", "1 or 2", stride)
    if len(pad) != 4 or min(pad) < 0 or max(pad) > kernel - 1:
        ops.refuse("maxpool", "pad", f"(top, left, bottom, right) in 0 .. kernel - 1 = {kernel - 1}", pad)
    if not (isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.dim() == 4 and x.size(3) % 4 == 0):
        ops.refuse("maxpool", "x", "float32 [B,H,W,C] with C a multiple of 4", x)
    return _MaxPool.apply(x, kernel, stride, pad)


def bottleneck(x: torch.Tensor, w1, s1, t1, w2, s2, t2, w3, s3, t3, wd=None, sd=None, td=None, stride: int = 1) -> torch.Tensor:
    """Bottleneck.forward (model.py:190-211) with a grad_fn, as ONE autograd node for the whole block: conv1 1x1 (stride) + BN + ReLU,
    SamePad2d(3,1) + conv2 3x3 + BN + ReLU, conv3 1x1 + BN, + residual (x, or the 1x1 downsample conv (stride) + BN of x), ReLU.
    x [B,H,W,Cin] NHWC float32, w1 [planes,1,1,Cin], w2 [planes,3,3,planes], w3 [4*planes,1,1,planes], wd [4*planes,1,1,Cin] or None
    (then Cin = 4*planes and stride 1), s* / t* the folded BatchNorm (scale, shift) of each conv; stride 1 or 2.

    The forward is four direct exact-fp32 launches in NHWC (no Winograd, no k-blocked intermediates), so it equals the composition of
    ops.conv_bn_act calls bit for bit; it saves x, the two intermediates and y. The backward is ops.conv_bn_act_backward for conv3
    (ReLU, res_div 1: its dresidual is the residual branch's gradient g), conv2, conv1 and the downsample conv on g; the input's
    gradient is then ops.dilate2_sum(dxc1, dxcd) at stride 2 (the two compact gradients summed while the full map is written),
    dxc1 + dxcd at stride 1 with a downsample, dx1 + g for an identity block. Gradients for x, the four weights and the four shifts;
    the scales get none (frozen BatchNorm). What does not require a gradient is not computed: the first trainable block of a
    schedule (x without requires_grad) computes no dx at all, a frozen weight no dw. A conv bias is folded into the shift by
    modules.fold_bn, shift = beta + scale * (bias - mean), so dbias = scale * dshift is the caller's one multiply."""
    stride = int(stride)
    if stride not in (1, 2):
        ops.refuse("bottleneck", "stride", "1 or 2", stride)
    if wd is None and (stride != 1 or sd is not None or td is not None or x.size(-1) != w3.size(0)):
        ops.refuse("bottleneck", "wd", f"a downsample weight [{w3.size(0)},1,1,{x.size(-1)}] where the stride is 2 or Cin != 4 * planes "
                   "(and sd, td None without it)", wd)
    return _Bottleneck.apply(x, w1, s1, t1, w2, s2, t2, w3, s3, t3, wd, sd, td, stride)


__all__ = ["conv_bn_act", "deconv2x2", "maxpool", "bottleneck"]
