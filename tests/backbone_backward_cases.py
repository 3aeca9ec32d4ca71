"""Cases, data and the float64 references of the backbone backward tests: ops.conv_bn_act_backward with a stride, ops.dilate2_sum,
ops.maxpool_backward (csrc/conv_backward.hip, csrc/pool_backward.hip) and layers.bottleneck / layers.maxpool.

As in conv_backward_cases the data are integers on which every product and partial sum of the forward and of the backward is exact
in fp32: x in [-4, 4] (blocks: [-2, 2]), gradients in [-3, 3], weights in {-1, 0, 1}, per-channel power-of-two scales (single convs:
{0.5, 1, 2, 4}; blocks and the chain: {1, 2}, so that a graph of seven layers stays on the integers), integer shifts. Each fp32
result — whatever the chunking of the weight gradient — then equals the float64 one bit for bit; check_conv and check_graph assert
the conditions (every value on the grid, every conv's sums of absolute products far enough below 2^24 grid steps) for every case.

The references are stock torch on the CPU in float64: F.conv2d / F.max_pool2d on F.pad, and autograd. The two new rules are also
restated in numpy (dilate2_sum_np, maxpool_backward_np). Nothing here needs a GPU or a fixture."""
import dataclasses
import functools

import numpy as np
import torch
import torch.nn.functional as F

from conv_exact_cases import channel_scale, channel_shift

F64 = torch.float64


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(F64)


def ints(rng, lim, *shape):
    return t64(rng.integers(-lim, lim + 1, shape).astype(np.float64))


def out_size(n, lo, hi, k, s):
    return (n + lo + hi - k) // s + 1


# ---------------------------------------------------------------------------------------------------------------------
# the float64 layers
# ---------------------------------------------------------------------------------------------------------------------
def conv64(x, w, pad=(0, 0, 0, 0), stride=1):
    """conv(x, w) on NHWC / OHWI float64 tensors with (top, left, bottom, right) zero padding → NHWC."""
    pt, pl, pb, pr = pad
    xn = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xn, w.permute(0, 3, 1, 2), stride=stride).permute(0, 2, 3, 1)


def pool64(x, kernel, stride, pad=(0, 0, 0, 0)):
    """F.pad(…, 0) then MaxPool2d (model.py:227-228) on an NHWC float64 tensor → NHWC."""
    pt, pl, pb, pr = pad
    xn = F.pad(x.permute(0, 3, 1, 2).contiguous(), (pl, pr, pt, pb))
    return F.max_pool2d(xn, kernel, stride).permute(0, 2, 3, 1)


def conv_grads64(x, w, z, pad, stride):
    """(dx, dw) of sum(conv(x, w) * z) in float64."""
    x, w = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    conv64(x, w, pad, stride).backward(z)
    return x.grad, w.grad


# ---------------------------------------------------------------------------------------------------------------------
# single strided convs
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Conv:
    id: str
    b: int
    h: int
    w: int
    cin: int
    cout: int
    k: tuple
    pad: tuple
    stride: int = 2
    act: int = 0
    scale: bool = False

    @property
    def out_hw(self):
        return (out_size(self.h, self.pad[0], self.pad[2], self.k[0], self.stride),
                out_size(self.w, self.pad[1], self.pad[3], self.k[1], self.stride))

    @property
    def m(self):
        return self.b * self.out_hw[0] * self.out_hw[1]

    @property
    def cout4(self):
        return -(-self.cout // 4) * 4

    @property
    def pointwise(self):
        return self.k == (1, 1) and self.pad == (0, 0, 0, 0)


CONVS = (
    Conv("1x1_s2_odd", 2, 9, 11, 8, 12, (1, 1), (0, 0, 0, 0), act=1, scale=True),       # odd H and W
    Conv("1x1_s2_ragged_cout", 1, 5, 6, 8, 10, (1, 1), (0, 0, 0, 0), act=1, scale=True),  # Cout % 4 != 0: z has two pad channels
    Conv("1x1_s2_multi_chunk", 2, 32, 32, 4, 32, (1, 1), (0, 0, 0, 0)),                  # M = 512: four chunks of 128 pixels
    Conv("7x7_s2_stem", 2, 18, 14, 4, 64, (7, 7), (3, 3, 3, 3), act=1, scale=True),      # the stem's form: taps over every border
    Conv("3x3_s2", 1, 7, 8, 8, 8, (3, 3), (1, 1, 1, 1)),
)
MULTI_CHUNK = "1x1_s2_multi_chunk"
ROUNDED = (MULTI_CHUNK, "7x7_s2_stem")


def conv_case(name):
    return {c.id: c for c in CONVS}[name]


def chunk_of(c) -> int:
    from maskrcnn_amd import ops
    return ops.conv_backward_chunk(c.b, c.h, c.w, c.cin, c.cout, *c.k, c.pad, stride=c.stride)


ConvData = dataclasses.make_dataclass("ConvData", ["x", "w", "scale", "shift", "dy", "y", "pre", "g", "z", "dx", "dw", "dshift"])


def _conv_reference(c, x, w, dy, scale, shift):
    x, w, shift = [t.detach().clone().requires_grad_(True) for t in (x, w, shift)]
    pre = conv64(x, w, c.pad, c.stride)
    pre = (pre * scale if scale is not None else pre) + shift
    pre.retain_grad()
    y = torch.relu(pre) if c.act == 1 else pre
    (y * dy).sum().backward()
    return pre.detach(), y.detach(), pre.grad, x.grad, w.grad, shift.grad


@functools.lru_cache(maxsize=None)
def build_conv(c):
    """Operands and expected results in float64; dx is the FULL gradient [B,H,W,Cin]. Seeds are tried in turn until, for ReLU cases,
    between 20 % and 80 % of pre is negative."""
    base = sum((i + 1) * ord(ch) for i, ch in enumerate(c.id))
    scale = t64(channel_scale(c.cout)) if c.scale else None
    shift = t64(channel_shift(c.cout))
    for attempt in range(50):
        rng = np.random.Generator(np.random.PCG64(base + attempt))
        x, w, dy = ints(rng, 4, c.b, c.h, c.w, c.cin), ints(rng, 1, c.cout, *c.k, c.cin), ints(rng, 3, c.b, *c.out_hw, c.cout)
        pre, y, g, dx, dw, dshift = _conv_reference(c, x, w, dy, scale, shift)
        if c.act != 1 or 0.2 <= float((pre < 0).double().mean()) <= 0.8:
            break
    else:
        raise AssertionError(f"{c.id}: no seed gives 20-80 % negative pre-activations")
    z = F.pad(g if scale is None else g * scale, (0, c.cout4 - c.cout))
    return ConvData(x, w, scale, shift, dy, y, pre, g, z, dx, dw, dshift)


def on_grid(t, grid, what):
    assert bool((t * grid == torch.round(t * grid)).all()) and float(t.abs().max()) * grid < 2 ** 24, what


def check_conv(c, d):
    """What makes bit equality with float64 a theorem for case c, and what makes the case a test of anything."""
    grid = 2.0                                            # scale 0.5: every value is a multiple of 1/2
    assert set(np.unique(d.w.numpy())) <= {-1.0, 0.0, 1.0}
    if d.scale is not None:
        assert bool((torch.log2(d.scale) == torch.round(torch.log2(d.scale))).all())
    absz = d.z[..., :c.cout].abs()
    sum_zw, sum_zx = conv_grads64(d.x.abs(), d.w.abs(), absz, c.pad, c.stride)
    assert float(sum_zx.max()) * grid < 2 ** 24 and float(sum_zw.max()) * grid < 2 ** 24, c.id
    assert float(conv64(d.x.abs(), d.w.abs(), c.pad, c.stride).max()) * grid < 2 ** 24
    for name in ("x", "w", "dy", "z", "g", "dx", "dw", "dshift", "y"):
        on_grid(getattr(d, name), grid, (c.id, name))
    for name in ("x", "w", "dy"):
        assert float((getattr(d, name) != 0).double().mean()) >= 0.3, (c.id, name)
    if c.act == 1:
        assert 0.2 <= float((d.pre < 0).double().mean()) <= 0.8
    assert bool(d.dw.any()) and bool(d.dx.any()) and bool(d.dshift.any())
    if c.pointwise:     # the full gradient lives on the even positions alone
        assert not bool(d.dx[:, 1::2].any()) and not bool(d.dx[:, :, 1::2].any())


@functools.lru_cache(maxsize=None)
def build_conv_rounded(c):
    """Standard-normal fp32 operands without activation or scale: z is dy, so dw is a function of (x, dy) alone."""
    rng = np.random.Generator(np.random.PCG64(91 + len(c.id)))
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    return dict(x=f(c.b, c.h, c.w, c.cin), w=f(c.cout, *c.k, c.cin), dy=f(c.b, *c.out_hw, c.cout))


# ---------------------------------------------------------------------------------------------------------------------
# dilate2_sum
# ---------------------------------------------------------------------------------------------------------------------
def dilate2_sum_np(a, b, height, width):
    """The rule restated: out[:, 2i, 2j] = a[:, i, j] (+ b[:, i, j] as one add in a's dtype), +0 elsewhere."""
    a = np.asarray(a)
    out = np.zeros((a.shape[0], height, width, a.shape[3]), a.dtype)
    out[:, ::2, ::2] = a if b is None else a + np.asarray(b)
    return out


def dilate2_sum64(a, b, height, width):
    """Autograd's way: the sum of the full-size gradients of two x[:, ::2, ::2] reads."""
    x = torch.zeros(a.shape[0], height, width, a.shape[3], dtype=F64, requires_grad=True)
    loss = (x[:, ::2, ::2] * a).sum()
    if b is not None:
        loss = loss + (x[:, ::2, ::2] * b).sum()
    loss.backward()
    return x.grad


DILATE_SHAPES = ((2, 9, 11, 8), (2, 32, 32, 4), (1, 6, 7, 12))      # (B, H, W, C): H and W odd, both even, one of each


def dilate_operands(shape, rounded=False):
    b, h, w, c = shape
    rng = np.random.Generator(np.random.PCG64(5 + h * w))
    compact = (b, (h + 1) // 2, (w + 1) // 2, c)
    if rounded:
        return tuple(torch.from_numpy(rng.standard_normal(compact).astype(np.float32)) for _ in range(2))
    return ints(rng, 50, *compact), ints(rng, 50, *compact)


# ---------------------------------------------------------------------------------------------------------------------
# max-pool backward
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Pool:
    id: str
    b: int
    h: int
    w: int
    c: int
    kernel: int
    stride: int
    same: bool = True      # pads from SamePad2d; False: none

    @property
    def pad(self):
        from maskrcnn_amd.ops import same_pad
        return tuple(same_pad(self.h, self.w, self.kernel, self.stride)) if self.same else (0, 0, 0, 0)

    @property
    def out_hw(self):
        pt, pl, pb, pr = self.pad
        return out_size(self.h, pt, pb, self.kernel, self.stride), out_size(self.w, pl, pr, self.kernel, self.stride)


POOLS = (
    Pool("3x3_s2_odd", 2, 7, 9, 8, 3, 2),            # pads (1, 1, 1, 1): on both sides
    Pool("3x3_s2_even", 1, 8, 8, 4, 3, 2),           # the stem's: pads at the bottom and the right alone
    Pool("1x1_s2", 2, 5, 6, 4, 1, 2, same=False),    # P6
)


def pool_case(name):
    return {p.id: p for p in POOLS}[name]


def pool_operands(p, rounded=False):
    """x: integers in [-2, 2] (many ties), but channel 1 all zero — every window is one tie, and ties with its padding zeros: in
    front of the real taps (top, left) the padding tap is taken and the gradient dropped, behind them (bottom, right) the first real
    zero is — and channel 2 all negative: a window that touches padding loses its gradient to the padding zero, an interior one has
    a real (often tied) maximum. dy: integers, or standard-normal fp32."""
    rng = np.random.Generator(np.random.PCG64(17 + p.h * p.w))
    x = rng.integers(-2, 3, (p.b, p.h, p.w, p.c)).astype(np.float64)
    if p.kernel > 1:
        x[..., 1] = 0.0
        x[..., 2] = -rng.integers(1, 3, (p.b, p.h, p.w)).astype(np.float64)
    shape = (p.b, *p.out_hw, p.c)
    dy = rng.standard_normal(shape).astype(np.float32).astype(np.float64) if rounded else rng.integers(-3, 4, shape).astype(np.float64)
    return t64(x), t64(dy)


def pool_grad64(p, x, dy):
    x = x.detach().clone().requires_grad_(True)
    pool64(x, p.kernel, p.stride, p.pad).backward(dy)
    return x.grad


def maxpool_backward_np(x, dy, kernel, stride, pad, dtype=np.float32):
    """The rule restated. Per output element the window is walked in (ky, kx) order, taps outside the image reading 0, from max = -inf
    at the first tap; a tap takes over when it is strictly greater (or NaN). The gradient goes to the taken tap unless that is
    padding. The windows are visited in ascending (oy, ox) order, so an input element's sum — in `dtype`, from +0 — has the gather
    form's order. → (dx, the number of dropped gradients)."""
    x, dy = np.asarray(x, dtype), np.asarray(dy, dtype)
    b, h, w, c = x.shape
    pt, pl, pb, pr = pad
    oh, ow = out_size(h, pt, pb, kernel, stride), out_size(w, pl, pr, kernel, stride)
    assert dy.shape == (b, oh, ow, c)
    dx = np.zeros_like(x)
    bi, ci = np.meshgrid(np.arange(b), np.arange(c), indexing="ij")
    dropped = 0
    for oy in range(oh):
        for ox in range(ow):
            best = np.full((b, c), -np.inf, dtype)
            arg = np.zeros((b, c), np.int64)
            for ky in range(kernel):
                for kx in range(kernel):
                    yy, xx = oy * stride - pt + ky, ox * stride - pl + kx
                    v = x[:, yy, xx, :] if 0 <= yy < h and 0 <= xx < w else np.zeros((b, c), dtype)
                    take = (v > best) | np.isnan(v)
                    best, arg = np.where(take, v, best), np.where(take, ky * kernel + kx, arg)
            yy, xx = oy * stride - pt + arg // kernel, ox * stride - pl + arg % kernel
            real = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            dropped += int((~real).sum())
            sel = (bi[real], yy[real], xx[real], ci[real])
            dx[sel] = (dx[sel] + dy[:, oy, ox, :][real]).astype(dtype)      # distinct elements within one window: a plain add
    return dx, dropped


# ---------------------------------------------------------------------------------------------------------------------
# Bottleneck blocks and the chain
# ---------------------------------------------------------------------------------------------------------------------
def block_scale(n):
    return t64(np.array([1.0, 2.0])[(np.arange(n) // 2) % 2])


@dataclasses.dataclass(frozen=True)
class Block:
    id: str
    b: int
    h: int
    w: int
    cin: int
    planes: int
    stride: int = 1
    down: bool = False

    @property
    def out_hw(self):
        return out_size(self.h, 0, 0, 1, self.stride), out_size(self.w, 0, 0, 1, self.stride)


BLOCKS = (
    Block("identity", 2, 6, 7, 16, 4),
    Block("downsample_s1", 2, 6, 7, 8, 4, down=True),
    Block("downsample_s2_odd", 2, 9, 7, 8, 4, stride=2, down=True),
)
BLOCK_PARAMS = ("w1", "t1", "w2", "t2", "w3", "t3", "wd", "td")


def block_case(name):
    return {k.id: k for k in BLOCKS}[name]


def block_operands(k, rng):
    """The block's parameters: weights in {-1, 0, 1}, scales in {1, 2}, integer shifts. wd / sd / td are None without a downsample."""
    c4 = 4 * k.planes
    p = dict(w1=ints(rng, 1, k.planes, 1, 1, k.cin), s1=block_scale(k.planes), t1=t64(channel_shift(k.planes)),
             w2=ints(rng, 1, k.planes, 3, 3, k.planes), s2=block_scale(k.planes), t2=t64(channel_shift(k.planes)[::-1]),
             w3=ints(rng, 1, c4, 1, 1, k.planes), s3=block_scale(c4), t3=t64(channel_shift(c4)),
             wd=None, sd=None, td=None)
    if k.down:
        p.update(wd=ints(rng, 1, c4, 1, 1, k.cin), sd=block_scale(c4), td=t64(channel_shift(c4)[::-1]))
    return p


def affine_conv64(x, w, s, t, pad=(0, 0, 0, 0), stride=1, tape=None):
    """scale * conv(x, w) + shift in float64; the layer is noted on `tape` with its pre-activation, whose gradient is kept."""
    pre = conv64(x, w, pad, stride)
    pre = (pre if s is None else pre * s) + t
    if tape is not None:
        pre.retain_grad()
        tape.append((x, w, s, pad, stride, pre))
    return pre


def block64(x, p, stride, tape=None):
    """Bottleneck.forward (model.py:190-211) from F.conv2d in float64 on NHWC tensors → (y, (h1, h2))."""
    res = x if p["wd"] is None else affine_conv64(x, p["wd"], p["sd"], p["td"], stride=stride, tape=tape)
    h1 = torch.relu(affine_conv64(x, p["w1"], p["s1"], p["t1"], stride=stride, tape=tape))
    h2 = torch.relu(affine_conv64(h1, p["w2"], p["s2"], p["t2"], (1, 1, 1, 1), tape=tape))
    return torch.relu(affine_conv64(h2, p["w3"], p["s3"], p["t3"], tape=tape) + res), (h1, h2)


def leaves(p):
    """Clones of the parameters that take a gradient, requiring one; the scales as they are."""
    return {n: (v.detach().clone().requires_grad_(True) if n in BLOCK_PARAMS and v is not None else v) for n, v in p.items()}


def check_graph(values, tape):
    """Exactness of a graph on the integers: every value an integer below 2^24, and for every conv on the tape the sums of the
    absolute products of its forward, of its data gradient and of its weight gradient — which bound every partial sum, in any
    order — below 2^22 (the affine's scale of at most 2 and the adds of shift and residual stay exact on top of them)."""
    for name, t in values.items():
        on_grid(t, 1.0, name)
    for x, w, s, pad, stride, pre in tape:
        x, w, z = x.detach().abs(), w.detach().abs(), (pre.grad if s is None else pre.grad * s).abs()
        on_grid(pre.detach(), 1.0, "pre")
        on_grid(z, 1.0, "z")
        sum_zw, sum_zx = conv_grads64(x, w, z, pad, stride)
        worst = max(float(conv64(x, w, pad, stride).max()), float(sum_zw.max()), float(sum_zx.max()))
        assert worst < 2 ** 22, (tuple(w.shape), worst)


BlockData = dataclasses.make_dataclass("BlockData", ["x", "p", "dy", "y", "mids", "grads", "tape"])


@functools.lru_cache(maxsize=None)
def build_block(k):
    rng = np.random.Generator(np.random.PCG64(sum(ord(ch) for ch in k.id)))
    x, p = ints(rng, 2, k.b, k.h, k.w, k.cin), block_operands(k, rng)
    dy = ints(rng, 3, k.b, *k.out_hw, 4 * k.planes)
    xg, q, tape = x.detach().clone().requires_grad_(True), leaves(p), []
    y, mids = block64(xg, q, k.stride, tape)
    (y * dy).sum().backward()
    grads = {"x": xg.grad, **{n: q[n].grad for n in BLOCK_PARAMS if q[n] is not None}}
    return BlockData(x, p, dy, y.detach(), tuple(m.detach() for m in mids), grads, tape)


def check_block(k, d):
    check_graph({"x": d.x, "dy": d.dy, "y": d.y, "h1": d.mids[0], "h2": d.mids[1], **d.grads}, d.tape)
    for n in ("w1", "w2", "w3", "wd"):
        assert d.p[n] is None or set(np.unique(d.p[n].numpy())) <= {-1.0, 0.0, 1.0}
    for t in (d.y, *d.mids):
        assert 0.15 <= float((t == 0).double().mean()) <= 0.85, (k.id, float((t == 0).double().mean()))
    assert all(bool(g.any()) for g in d.grads.values())
    assert set(d.grads) == {"x"} | {n for n in BLOCK_PARAMS if d.p[n] is not None}


# the chain: a stride-2 block, an identity block, maxpool(1, 2), a 1x1 stride-2 conv
CHAIN_BLOCKS = (Block("chain_a", 2, 9, 10, 8, 4, stride=2, down=True), Block("chain_b", 2, 5, 5, 16, 4))
CHAIN_COUT = 8


def chain64(x, pa, pb, wc, tc, tape=None):
    ya, _ = block64(x, pa, 2, tape)
    yb, _ = block64(ya, pb, 1, tape)
    p6 = pool64(yb, 1, 2)
    return affine_conv64(p6, wc, None, tc, stride=2, tape=tape), (ya, yb, p6)


ChainData = dataclasses.make_dataclass("ChainData", ["x", "pa", "pb", "wc", "tc", "dy", "y", "mids", "grads", "tape"])


@functools.lru_cache(maxsize=1)
def build_chain():
    """Gradient names: x, a.<param>, b.<param>, wc, tc."""
    ka, kb = CHAIN_BLOCKS
    rng = np.random.Generator(np.random.PCG64(2024))
    x = ints(rng, 1, ka.b, ka.h, ka.w, ka.cin)
    pa, pb = block_operands(ka, rng), block_operands(kb, rng)
    wc, tc = ints(rng, 1, CHAIN_COUT, 1, 1, 16), t64(channel_shift(CHAIN_COUT))
    dy = ints(rng, 2, ka.b, 2, 2, CHAIN_COUT)         # 9 x 10 -> 5 x 5 -> 3 x 3 (P6) -> 2 x 2
    xg, qa, qb, tape = x.detach().clone().requires_grad_(True), leaves(pa), leaves(pb), []
    wcg, tcg = wc.detach().clone().requires_grad_(True), tc.detach().clone().requires_grad_(True)
    y, mids = chain64(xg, qa, qb, wcg, tcg, tape)
    (y * dy).sum().backward()
    grads = {"x": xg.grad, "wc": wcg.grad, "tc": tcg.grad}
    grads.update({f"a.{n}": qa[n].grad for n in BLOCK_PARAMS if qa[n] is not None})
    grads.update({f"b.{n}": qb[n].grad for n in BLOCK_PARAMS if qb[n] is not None})
    return ChainData(x, pa, pb, wc, tc, dy, y.detach(), tuple(m.detach() for m in mids), grads, tape)


def check_chain(d):
    check_graph({"x": d.x, "dy": d.dy, "y": d.y, **{f"mid{i}": m for i, m in enumerate(d.mids)}, **d.grads}, d.tape)
    assert all(bool(g.any()) for g in d.grads.values()), [n for n, g in d.grads.items() if not bool(g.any())]
