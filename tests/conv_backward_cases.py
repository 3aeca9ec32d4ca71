"""Cases, data and the float64 reference of the conv backward tests (ops.conv_bn_act_backward, csrc/conv_backward.hip).

The data are as in conv_exact_cases: x integers in [-4, 4], dy and w integers in [-3, 3], scale a per-channel power of two from
{0.5, 1, 2, 4}, shift per-channel integers that differ between neighbours. Every product and partial sum of the backward is then
an integer multiple of 1/2 far below 2^24 (check_invariants asserts it for every case), so each fp32 result — whatever the chunking
of the weight gradient and the route of the data gradient — equals the float64 one bit for bit.

The reference is torch on the CPU in float64: F.conv2d plus autograd of act(scale * conv + shift + residual). Nothing here needs a
GPU or a fixture."""
import dataclasses
import functools

import numpy as np
import torch
import torch.nn.functional as F

from conv_exact_cases import channel_scale, channel_shift

F64 = torch.float64


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    b: int
    h: int
    w: int
    cin: int
    cout: int          # GEMM columns: 4 x the channels with scatter
    k: tuple           # (kh, kw)
    pad: tuple         # (top, left, bottom, right)
    act: int = 0
    scale: bool = False
    res_div: int = 0
    scatter: bool = False
    counts: tuple = ()  # row groups: valid rows per group
    rpg: int = 0
    single: bool = False   # the weight gradient is one chunk

    @property
    def out_hw(self):
        return self.h + self.pad[0] + self.pad[2] - self.k[0] + 1, self.w + self.pad[1] + self.pad[3] - self.k[1] + 1

    @property
    def m(self):
        return self.b * self.out_hw[0] * self.out_hw[1]

    @property
    def cout4(self):
        return -(-self.cout // 4) * 4

    @property
    def shape_args(self):
        return (self.b, self.h, self.w, self.cin, self.cout, *self.k, 1, *self.pad)


def chunk_of(case) -> int:
    from maskrcnn_amd import ops
    return ops.conv_backward_chunk(case.b, case.h, case.w, case.cin, case.cout, *case.k, case.pad)


def chunks_of(case) -> int:
    return -(-case.m // chunk_of(case))


@functools.lru_cache(maxsize=1)
def _multi_chunk_map():
    """The smallest odd map s x s at which batch 5, 3x3 SAME, 8 -> 8 channels is at least 3 chunks, the last one ragged."""
    for s in range(3, 200, 2):
        c = Case("probe", 5, s, s, 8, 8, (3, 3), (1, 1, 1, 1))
        if chunks_of(c) >= 3 and c.m % chunk_of(c):
            return s
    raise AssertionError("no multi-chunk map below 200 x 200")


ROW_COUNTS = (0, 0, 0, 37, 100, 0, 100, 5, 0, 0, 0, 100, 1)


@functools.lru_cache(maxsize=1)
def cases():
    s = _multi_chunk_map()
    same3, none = (1, 1, 1, 1), (0, 0, 0, 0)
    return (
        Case("1x1_generic", 3, 13, 11, 20, 18, (1, 1), none),                                  # Cout4 = 20; no channel count a multiple of 32
        Case("3x3_ragged", 3, 13, 11, 32, 33, (3, 3), same3, act=1, scale=True),
        Case("3x3_pow2", 2, 16, 16, 64, 64, (3, 3), same3, act=1, scale=True),
        Case("3x3_straddle", 2, 6, 5, 12, 129, (3, 3), same3),                                 # N tile straddles taps; second M' tile of one row
        Case("7x7_pad3", 2, 9, 7, 8, 36, (7, 7), (3, 3, 3, 3)),
        Case("3x3_unpadded_single", 2, 6, 5, 8, 12, (3, 3), none, single=True),                # data-gradient pads are 2
        Case("2x2_asymmetric_single", 2, 5, 4, 8, 6, (2, 2), (0, 0, 1, 1), scale=True, single=True),
        Case("one_pixel_single", 2, 3, 3, 8, 5, (3, 3), none, single=True),
        Case("residual_1", 2, 6, 7, 8, 16, (3, 3), same3, act=1, scale=True, res_div=1),       # g != z
        Case("residual_2", 2, 14, 10, 16, 12, (1, 1), none, scale=True, res_div=2),
        Case("scatter", 3, 5, 7, 32, 4 * 9, (1, 1), none, act=1, scatter=True),
        Case("multi_chunk", 5, s, s, 8, 8, (3, 3), same3),
        Case("rows", 1300, 1, 1, 64, 81, (1, 1), none, act=1, scale=True, counts=ROW_COUNTS, rpg=100),
        Case("rows_2x2", 24, 2, 2, 8, 10, (3, 3), same3, act=1, scale=True, counts=(0, 12, 32), rpg=32),   # 4 pixels per slot
    )


def case(name):
    return {c.id: c for c in cases()}[name]


def valid_rows(c):
    """bool [M]: the output rows that contribute (all of them without row groups)."""
    if not c.counts:
        return np.ones(c.m, bool)
    assert len(c.counts) * c.rpg == c.m
    return (np.arange(c.m) % c.rpg) < np.repeat(np.array(c.counts), c.rpg)


# ---------------------------------------------------------------------------------------------------------------------
# the float64 graph
# ---------------------------------------------------------------------------------------------------------------------
def conv64(x, w, pad):
    """conv(x, w) at stride 1 on NHWC / OHWI float64 tensors with (top, left, bottom, right) zero padding → NHWC."""
    pt, pl, pb, pr = pad
    xn = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xn, w.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)


def scatter_nhwc(t4):
    """[B,H,W,4*C] GEMM columns (dy*2+dx)*C + co → [B,2H,2W,C]."""
    b, h, w, c4 = t4.shape
    return t4.reshape(b, h, w, 2, 2, c4 // 4).permute(0, 1, 3, 2, 4, 5).reshape(b, 2 * h, 2 * w, c4 // 4)


def gather_nhwc(t):
    """The inverse of scatter_nhwc."""
    b, h2, w2, c = t.shape
    return t.reshape(b, h2 // 2, 2, w2 // 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h2 // 2, w2 // 2, 4 * c)


def conv_grads64(x, w, z, pad):
    """(dx, dw) of sum(conv(x, w) * z) in float64: the two sums of the rule, from any z."""
    x, w = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    conv64(x, w, pad).backward(z)
    return x.grad, w.grad


Data = dataclasses.make_dataclass("Data", ["x", "w", "scale", "shift", "residual", "dy", "y", "pre", "valid",
                                           "g", "z", "dx", "dw", "dshift", "dresidual"])


def _operands(c, seed, rounded=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    oh, ow = c.out_hw
    if rounded:
        draw = lambda lim, shape: rng.standard_normal(shape)
    else:
        draw = lambda lim, shape: rng.integers(-lim, lim + 1, shape).astype(np.float64)
    x = draw(4, (c.b, c.h, c.w, c.cin))
    w = draw(3, (c.cout, *c.k, c.cin))
    dy = draw(3, (c.b, oh, ow, c.cout))
    res = draw(8, (c.b, oh // c.res_div, ow // c.res_div, c.cout)) if c.res_div else None
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(F64)
    return t(x), t(w), t(dy), t(res)


def reference(c, x, w, dy, res, scale, shift, y=None):
    """Autograd of act(scale * conv + shift + residual) in float64 on GEMM-layout tensors ([B,OH,OW,cout]; the scatter is a
    relabelling of those elements). Rows that row groups switch off are masked out of the loss and their x rows zeroed, which is
    what 'the valid rows alone' means. With `y` given (rounded data) the activation's derivative is taken at that y."""
    valid = torch.from_numpy(valid_rows(c)).reshape(c.b, *c.out_hw, 1)
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    shift = shift.detach().clone().requires_grad_(True)
    res = None if res is None else res.detach().clone().requires_grad_(True)
    pre = conv64(x, w, c.pad)
    if scale is not None:
        pre = pre * scale
    pre = pre + shift
    if res is not None:
        pre = pre + (res if c.res_div == 1 else res.repeat_interleave(2, 1).repeat_interleave(2, 2))
    pre.retain_grad()
    yy = torch.relu(pre) if c.act == 1 else torch.sigmoid(pre) if c.act == 2 else pre
    (yy * dy * valid).sum().backward()
    return pre.detach(), yy.detach(), valid, pre.grad, x.grad, w.grad, shift.grad, None if res is None else res.grad


@functools.lru_cache(maxsize=4)
def build(c, seed=None):
    """The operands and every expected result in float64, GEMM layout (scatter cases: .y and .dy are [B,H,W,4C]; the test scatters
    them). Rows that the row groups switch off keep finite values here; the GPU tests overwrite them with NaN. Seeds are tried
    in turn until, for ReLU cases, between 20 % and 80 % of pre is negative (the reference alone decides)."""
    base = sum((i + 1) * ord(ch) for i, ch in enumerate(c.id)) % (2 ** 31) if seed is None else seed
    scale = torch.from_numpy(channel_scale(c.cout)).to(F64) if c.scale else None
    shift = torch.from_numpy(channel_shift(c.cout)).to(F64)
    for attempt in range(50):
        x, w, dy, res = _operands(c, base + attempt)
        if c.counts:      # a switched-off output row's taps are switched off with it: its x is never read (the slot's whole map)
            keep = torch.from_numpy(valid_rows(c)).reshape(c.b, *c.out_hw, 1)
            assert c.out_hw == (c.h, c.w)
            x = x * keep
        pre, y, valid, g, dx, dw, dshift, dres = reference(c, x, w, dy, res, scale, shift)
        neg = float((pre < 0).double().mean())
        if c.act != 1 or 0.2 <= neg <= 0.8:
            break
    else:
        raise AssertionError(f"{c.id}: no seed gives 20-80 % negative pre-activations")
    z = g if scale is None else g * scale
    z = F.pad(z, (0, c.cout4 - c.cout))
    return Data(x, w, scale, shift, res, dy, y, pre, valid, g, z, dx, dw, dshift, dres)


def check_invariants(c, d):
    """What makes bit equality with float64 a theorem for case c, and what makes the case a test of anything."""
    grid = 2.0     # every value is a multiple of 1/2 (scale 0.5)
    absx, absw, absz = d.x.abs(), d.w.abs(), d.z[..., :c.cout].abs()
    sum_zw, sum_zx = conv_grads64(absx, absw, absz, c.pad)
    assert float(sum_zx.max()) * grid < 2 ** 24, (c.id, "sum |z||x|", float(sum_zx.max()))
    assert float(sum_zw.max()) * grid < 2 ** 24, (c.id, "sum |z||w|", float(sum_zw.max()))
    for name, t in (("x", d.x), ("w", d.w), ("dy", d.dy), ("z", d.z[..., :c.cout])):
        if c.counts and name != "w":      # x, dy and z have one row per output row here (1x1, or SAME on the slot's own map)
            t = t.reshape(c.m, -1)[d.valid.reshape(-1)]
        assert float((t != 0).double().mean()) >= 0.3, (c.id, name, float((t != 0).double().mean()))
    for t in (d.z, d.g, d.dx, d.dw, d.dshift):
        assert bool((t * grid == torch.round(t * grid)).all()) and float(t.abs().max()) * grid < 2 ** 24
    if c.act == 1:
        pre = d.pre[d.valid.expand_as(d.pre)]
        assert 0.2 <= float((pre < 0).double().mean()) <= 0.8, (c.id, float((pre < 0).double().mean()))
    assert bool(d.dw.any()) and bool(d.dx.any()) and bool(d.dshift.any())


# ---------------------------------------------------------------------------------------------------------------------
# rounded data
# ---------------------------------------------------------------------------------------------------------------------
SIGMOID = Case("sigmoid_1x1", 3, 7, 9, 32, 5, (1, 1), (0, 0, 0, 0), act=2)
ROUNDED = ("3x3_ragged", "7x7_pad3", "multi_chunk", "sigmoid_1x1")


def rounded_case(name):
    return SIGMOID if name == "sigmoid_1x1" else case(name)


@functools.lru_cache(maxsize=4)
def build_rounded(c):
    """Standard-normal fp32 operands, y = the fp32 forward on the CPU, and g and z by the rule restated in torch fp32 operations,
    one rounding each."""
    f32 = torch.float32
    x, w, dy, _ = [None if t is None else t.to(f32) for t in _operands(c, 77 + len(c.id), rounded=True)]
    scale = torch.from_numpy(channel_scale(c.cout)).to(f32) if c.scale else None
    shift = torch.from_numpy(channel_shift(c.cout)).to(f32) * 0.25
    pre = conv64(x, w, c.pad)
    pre = (pre * scale if scale is not None else pre) + shift
    y = torch.relu(pre) if c.act == 1 else torch.sigmoid(pre) if c.act == 2 else pre
    if c.act == 1:
        g = torch.where(y > 0, dy, torch.zeros_like(dy))
    elif c.act == 2:
        t = 1.0 - y
        u = y * t
        g = dy * u
    else:
        g = dy
    z = F.pad(g * scale if scale is not None else g, (0, c.cout4 - c.cout))
    return dict(x=x, w=w, dy=dy, y=y.contiguous(), scale=scale, g=g, z=z)
