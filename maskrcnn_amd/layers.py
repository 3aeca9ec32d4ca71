"""Differentiable forms of the head layers' building blocks — what train_model(layers="heads") trains (model.py:1010-1016: fpn.P*,
rpn.*, classifier.*, mask.*, BatchNorm frozen and in eval mode): every such layer is a stride-1 fp32 NHWC conv with the fused
epilogue act(scale * conv + shift (+ residual)), or the 2x2 transposed conv.

    conv_bn_act(x, w, scale, shift, pad, act, residual, res_div, row_counts, rows_per_group)
    deconv2x2(x, w4, bias4, act)

The forward is the existing exact-fp32 direct launch (ops.conv_bn_act / ops.deconv2x2, unchanged: those calls save nothing and
return tensors without a grad_fn); the backward is ops.conv_bn_act_backward (csrc/conv_backward.hip). Gradients go to x, w, shift /
bias4 and the residual. `scale` gets none: BatchNorm is frozen in that stage."""
from __future__ import annotations

import torch

from . import ops


class _ConvBnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, scale, shift, residual, row_counts, pad, act, res_div, rows_per_group):
        x, w = x.contiguous(), w.contiguous()
        residual = None if residual is None else residual.contiguous()
        y = ops.conv_bn_act(x, w, scale, shift, 1, pad, act, residual, res_div, row_counts=row_counts, rows_per_group=rows_per_group)
        ctx.save_for_backward(x, w, scale, y if act else None, row_counts)
        ctx.call = (pad, act, res_div if residual is not None else 0, rows_per_group)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, w, scale, y, row_counts = ctx.saved_tensors
        pad, act, res_div, rows_per_group = ctx.call
        need = ctx.needs_input_grad
        r = ops.conv_bn_act_backward(grad, x, w, y, scale, pad, act, res_div, False, row_counts, rows_per_group,
                                     needs=(need[0], need[1], need[3], need[4] and res_div != 0))
        return r.dx, r.dw, None, r.dshift, r.dresidual, None, None, None, None, None


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


def conv_bn_act(x: torch.Tensor, w: torch.Tensor, scale: torch.Tensor | None = None, shift: torch.Tensor | None = None,
                pad=(0, 0, 0, 0), act: int = 0, residual: torch.Tensor | None = None, res_div: int = 1,
                row_counts: torch.Tensor | None = None, rows_per_group: int = 0) -> torch.Tensor:
    """y = act(scale * conv(x, w) + shift (+ residual)) at stride 1 with a grad_fn: x [B,H,W,Cin] NHWC float32 (Cin % 4 == 0),
    w [Cout,KH,KW,Cin], scale / shift [Cout] or None, pad = (top, left, bottom, right) each at most the kernel size - 1, act 0 none /
    1 ReLU / 2 sigmoid, residual [B,OH/res_div,OW/res_div,Cout] with res_div 1 or 2, row_counts / rows_per_group as ops.conv_bn_act
    takes them. Gradients for x, w, shift and residual; none for scale."""
    return _ConvBnAct.apply(x, w, scale, shift, residual, row_counts, tuple(int(v) for v in pad), int(act), int(res_div),
                            int(rows_per_group))


def deconv2x2(x: torch.Tensor, w4: torch.Tensor, bias4: torch.Tensor, act: int = 0) -> torch.Tensor:
    """The 2x2 stride-2 transposed conv + bias + activation with a grad_fn: x [B,H,W,Cin], w4 [4*C,1,1,Cin] (row (dy*2+dx)*C + co),
    bias4 [4*C] (the bias once per tap: a caller that makes it with bias.repeat(4) gets the four taps added by autograd) →
    [B,2H,2W,C]. act 0 none / 1 ReLU. Gradients for x, w4 and bias4."""
    return _Deconv2x2.apply(x, w4, bias4, int(act))


__all__ = ["conv_bn_act", "deconv2x2"]
