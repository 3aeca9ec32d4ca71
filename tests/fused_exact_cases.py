"""Cases, data and float64 references of the exact-arithmetic sweep over the hand-written fused kernels: Winograd F(2x2)
(csrc/conv_wino.hip, plain and with the RPN heads), the pipelined fp16 conv with the heads, the whole-block fp32 Bottleneck
(csrc/bottleneck.hip), the three stem kernels (csrc/stem.hip), the one-launch fp16 C2 block (csrc/bottleneck_f16.hip) and the
fp16 mask tail (csrc/mask_tail_f16.hip). tests/test_fused_exact_host.py checks the data without a GPU,
tests/test_gpu_fused_exact.py runs the kernels. The twin of tests/conv_exact_cases.py, whose data rule it shares: small signed
integers, a per-channel power-of-two scale (channel_scale(n) * base) and channel_shift(n) as the shift, so that a swapped or
shifted channel, pixel, tap, image or sub-pixel changes the result.

On such data every one of these kernels is exactly computable:
  * F(2x2): G has the entries 0, +-1/2, 1 and B^T, A^T the entries 0, +-1, so every U = G g G^T, V = B^T d B, product and sum
    is a multiple of 1/4 of the operands' granule — exact in fp32 in any order while sum |U||V| stays below 2^24 granules;
  * stem: 147 integer products per output;
  * the fused fp16 kernels: fp32 accumulation of fp16 integers is exact, and the ONE rounding to fp16 per intermediate is
    round-to-nearest-even, which numpy's astype(float16) reproduces on the exact float64 value.
The references are F.conv2d / F.conv_transpose2d / F.max_pool2d in float64. Every reference takes `mut`, ONE thing done wrong
(MUTANTS): the host test asserts that each mutant changes `want`, i.e. that the data would notice that error in a kernel.

F(4x4) (csrc/conv_wino4.hip) is not here but in tests/wino4_exact_cases.py: with the interpolation points 0, +-3/4, +-3/2 its
G has the entries 64/81, 32/81 and 8/27, U = G g G^T is not dyadic for integer g, so no CONVOLUTION is exact there. But those
kernels take U as an operand, and B^T and A^T are dyadic: on a synthetic integer U the bilinear form they evaluate is exact, and
that sweep holds them to it bit for bit (the tolerance tests of tests/test_gpu_conv.py keep showing that the form is a
convolution)."""
import dataclasses
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

from conv_exact_cases import channel_scale, channel_shift, kblocked  # noqa: F401  (kblocked: for the GPU test)

# one thing wrong in the reference (the input mutants — swapped channels, the last image replaced — change the operands instead)
MUTANTS = ("shift_tap", "trunc", "residual_after_relu", "edge_pad", "pool_pad_top_left")


# ---------------------------------------------------------------------------------------------------------------------
# shared pieces
# ---------------------------------------------------------------------------------------------------------------------
def _rng(case_id):
    return np.random.Generator(np.random.PCG64(sum((i + 1) * ord(ch) for i, ch in enumerate(case_id)) % (2 ** 31)))


def _ints(rng, r, shape):
    return rng.integers(-r, r + 1, shape).astype(np.float64)


def r16(v, trunc=False):
    """The float64 array rounded to fp16 (round to nearest even; trunc: toward zero — a mutant), as float64."""
    with np.errstate(over="ignore"):
        r = v.astype(np.float16)
    if trunc:
        over = np.abs(r.astype(np.float64)) > np.abs(v)
        r = np.where(over, np.nextafter(r, np.float16(0)), r)
    return r.astype(np.float64)


def conv64(x, w, pad=(0, 0, 0, 0), stride=1, mut=None):
    """conv(x NHWC, w OHWI) in float64 -> NHWC, zero pad (top, left, bottom, right). Exact: every value is an integer times a
    power of two far below 2^53. mut "edge_pad": the pad replicates the edge; "shift_tap": the centre tap reads one pixel to
    the left of where it should."""
    pt, pl, pb, pr = pad
    xt = torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2)
    xt = F.pad(xt, (pl, pr, pt, pb), mode="replicate" if mut == "edge_pad" and max(pad) else "constant")
    wt = torch.from_numpy(np.ascontiguousarray(w)).permute(0, 3, 1, 2).contiguous()
    if mut == "shift_tap":
        tap = torch.zeros_like(wt)
        ky, kx = wt.shape[2] // 2, wt.shape[3] // 2
        tap[:, :, ky, kx] = wt[:, :, ky, kx]
        y = F.conv2d(xt, wt - tap, None, stride=stride) + F.conv2d(torch.roll(xt, 1, 3), tap, None, stride=stride)
    else:
        y = F.conv2d(xt, wt, None, stride=stride)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def conv_abs(x, w, pad=(0, 0, 0, 0), stride=1):
    """The largest sum |x||w| over the outputs."""
    return float(conv64(np.abs(x), np.abs(w), pad, stride).max())


G_ = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)


def _tiles(xp, h, wd):
    """The 4 x 4 input tiles (stride 2) of the padded map xp [B,h+2,wd+2,C] -> [B,h/2,wd/2,4,4,C]."""
    return np.stack([np.stack([xp[:, i:i + h:2, j:j + wd:2] for j in range(4)], 3) for i in range(4)], 3)


def wino_abs(x, w):
    """The absolute Winograd evaluation |A^T| [sum_c |U| .* (|B^T||d||B|)] |A| of the 3x3 SAME conv, its largest element: a bound
    on every partial sum of the F(2x2) kernels in any order (U = G g G^T itself, then absolute values)."""
    b, h, wd, _ = x.shape
    u = np.abs(np.einsum("ij,ojkc,lk->oilc", G_, w, G_))
    d = _tiles(np.pad(np.abs(x), ((0, 0), (1, 1), (1, 1), (0, 0))), h, wd)
    v = np.einsum("pi,btuijc,qj->btupqc", np.abs(BT), d, np.abs(BT))
    m = np.einsum("btupqc,opqc->btupqo", v, u)
    return float(np.einsum("ip,btupqo,jq->btuijo", np.abs(AT), m, np.abs(AT)).max())


def wino64(x, w):
    """The same conv evaluated AS F(2x2) in float64 (the host test compares it with conv64: the transforms are the textbook's)."""
    b, h, wd, _ = x.shape
    u = np.einsum("ij,ojkc,lk->oilc", G_, w, G_)
    d = _tiles(np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0))), h, wd)
    m = np.einsum("btupqc,opqc->btupqo", np.einsum("pi,btuijc,qj->btupqc", BT, d, BT), u)
    y = np.einsum("ip,btupqo,jq->btuijo", AT, m, AT)
    return np.ascontiguousarray(y.transpose(0, 1, 3, 2, 4, 5).reshape(b, h, wd, -1))


def _tr(mut, name):
    """Does the mutant truncate this fp16 intermediate? ("trunc": all of them, "trunc:<name>": that one)"""
    return mut == "trunc" or mut == f"trunc:{name}"


def affine(acc, scale, shift):
    return acc * (1.0 if scale is None else scale) + shift


def relu(v):
    return np.maximum(v, 0.0) + 0.0     # -0.0 -> +0.0


def _data(**kw):
    return types.SimpleNamespace(**kw)


class Budget:
    """The exactness ledger of a case: (name, largest absolute value a sum or result can reach, granule). The host test asserts
    bound / granule < 2^24 for every line."""

    def __init__(self):
        self.lines = []

    def add(self, name, bound, granule):
        """bound, granule: numbers, or one per channel."""
        self.lines.append((name, np.asarray(bound, dtype=np.float64), np.asarray(granule, dtype=np.float64)))

    def affine(self, name, acc_abs, g_acc, scale, shift, extra=0.0, g_extra=1.0):
        """acc * scale + shift (+ a residual of at most `extra`, a multiple of g_extra), channel by channel: a power-of-two
        scale moves the bound and the granule alike, the integer shift and the residual do not. -> the result's granule."""
        sc = np.ones_like(shift) if scale is None else scale
        g = np.minimum(np.minimum(g_acc * sc, 1.0), g_extra)
        self.add(name, sc * acc_abs + np.abs(shift) + extra, g)
        return float(g.min())

    def bits(self):
        return {n: float(np.log2(np.maximum(b, g) / g).max()) for n, b, g in self.lines}


# ---------------------------------------------------------------------------------------------------------------------
# F(2x2) plain: ops.conv3x3_winograd, x in [-4,4], w in [-3,3]
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class WinoCase:
    tiles: str      # "linear": under 16 x 16 px, the linear-tile kernel by default; "spatial": 8 x 8-position blocks by default
    b: int
    h: int
    w: int
    cin: int
    cout: int

    @property
    def id(self):
        return f"wino-{self.tiles}-{self.b}x{self.h}x{self.w}x{self.cin}x{self.cout}"


WINO_SHAPES = {
    "linear": [(1, 2, 2, 8, 5),        # one position, one k tile
               (3, 6, 10, 16, 70),     # 45 positions, fewer than one tile; images share a tile; ragged N
               (2, 14, 14, 24, 96)],   # 98 positions: two M tiles, the second ragged; three k tiles; N = 64 + 32
    "spatial": [(1, 16, 16, 8, 64),    # one 8 x 8 block
                (2, 20, 36, 24, 72),   # 10 x 18 positions: ragged blocks in both directions, two images
                (1, 32, 16, 512, 64)], # long K
}
WINO_CASES = [WinoCase(t, *s) for t, shapes in WINO_SHAPES.items() for s in shapes]
WINO_VARIANTS = [(s, r) for s in (False, True) for r in (False, True)]      # (with scale, with ReLU)


def wino_operands(case):
    rng = _rng(case.id)
    x = _ints(rng, 4, (case.b, case.h, case.w, case.cin))
    w = _ints(rng, 3, (case.cout, 3, 3, case.cin))
    return dict(x=x, w=w, scale=channel_scale(case.cout), shift=channel_shift(case.cout))


def wino_eval(case, o, with_scale=True, with_relu=True, mut=None):
    acc = conv64(o["x"], o["w"], (1, 1, 1, 1), mut=mut)
    pre = affine(acc, o["scale"] if with_scale else None, o["shift"])
    return dict(acc=acc, pre=pre, want=(relu(pre) if with_relu else pre + 0.0))


@functools.lru_cache(maxsize=2)
def build_wino(case):
    o = wino_operands(case)
    e = wino_eval(case, o)
    bud = Budget()
    a = wino_abs(o["x"], o["w"])
    bud.add("winograd sums", a, 0.25)
    bud.affine("affine", a, 0.25, o["scale"], o["shift"])
    want = {(s, r): wino_eval(case, o, s, r)["want"] if (s, r) != (True, True) else e["want"] for s, r in WINO_VARIANTS}
    pres = {s: affine(e["acc"], o["scale"] if s else None, o["shift"]) for s in (False, True)}
    return _data(**o, acc=e["acc"], pres=pres, want=want, budget=bud, f16_operands=(), relu_layers={"pre": e["pre"]},
                 rounded={})


# ---------------------------------------------------------------------------------------------------------------------
# the RPN heads inside a conv: ops.conv3x3_winograd_heads (fp32) and ops.conv_f16_pipelined_heads (fp16 operands, Cout 512)
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class HeadsCase:
    op: str         # "wino" / "f16p"
    b: int
    h: int
    w: int
    cin: int
    cout: int

    @property
    def id(self):
        return f"heads-{self.op}-{self.b}x{self.h}x{self.w}x{self.cin}x{self.cout}"


# f16p: conv_f16_pipelined_supported asks for Cin % 64 == 0 and sets no lower limit on the map (Cout is 512 by the consumer's
# form): one pixel tile holding 4 of its rows, and 3 x 13 x 11 = 429 rows, whose last tile is ragged at every tile height
# (128, 160, 192, 256)
HEADS_CASES = [HeadsCase("wino", 1, 16, 16, 8, 64), HeadsCase("wino", 2, 20, 36, 16, 128),
               HeadsCase("f16p", 1, 2, 2, 64, 512), HeadsCase("f16p", 3, 13, 11, 64, 512)]
HEADS_BASE = {"wino": 1.0, "f16p": 0.125}


def heads_operands(case):
    rng = _rng(case.id)
    # f16p: x in [-127,127], so that the conv sums have up to 16 significant bits and the fp16 activation tile really rounds
    x = _ints(rng, 127 if case.op == "f16p" else 4, (case.b, case.h, case.w, case.cin))
    w = _ints(rng, 3, (case.cout, 3, 3, case.cin))
    wh = np.zeros((32, case.cout))
    wh[:18] = _ints(rng, 2, (18, case.cout))       # rows 18..31 stay zero
    return dict(x=x, w=w, scale=channel_scale(case.cout) * HEADS_BASE[case.op], shift=channel_shift(case.cout), w_head32=wh,
                bias=channel_shift(18))


def heads_eval(case, o, mut=None):
    acc = conv64(o["x"], o["w"], (1, 1, 1, 1), mut=mut)
    pre = affine(acc, o["scale"], o["shift"])
    act_exact = relu(pre)
    act = r16(act_exact, _tr(mut, "act")) if case.op == "f16p" else act_exact     # the fp16 tile the head MFMAs read
    sums = act @ o["w_head32"].T                                                 # [B,H,W,32]
    return dict(acc=acc, pre=pre, act_exact=act_exact, act=act, sums=sums, want=sums[..., :18] + o["bias"] + 0.0)


@functools.lru_cache(maxsize=2)
def build_heads(case):
    o = heads_operands(case)
    e = heads_eval(case, o)
    bud = Budget()
    a = wino_abs(o["x"], o["w"]) if case.op == "wino" else conv_abs(o["x"], o["w"], (1, 1, 1, 1))
    g_acc = 0.25 if case.op == "wino" else 1.0
    bud.add("conv sums", a, g_acc)
    g_act = bud.affine("affine", a, g_acc, o["scale"], o["shift"])
    habs = float((e["act"] @ np.abs(o["w_head32"]).T).max())
    bud.add("head sums", habs, g_act)
    bud.add("head sums + bias", habs + np.abs(o["bias"]).max(), g_act)
    f16 = ("x", "w", "w_head32") if case.op == "f16p" else ()
    rounded = {"act": (e["act_exact"], e["act"])} if case.op == "f16p" else {}
    return _data(**o, **e, budget=bud, f16_operands=f16, relu_layers={"pre": e["pre"]}, rounded=rounded)


# ---------------------------------------------------------------------------------------------------------------------
# whole-block fp32 Bottleneck: ops.bottleneck_fused, 256 -> 64 -> 64 -> 256, identity residual, conv2 as F(2x2)
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class BlockCase:
    b: int
    h: int
    w: int

    @property
    def id(self):
        return f"block32-{self.b}x{self.h}x{self.w}"


BLOCK_CASES = [BlockCase(1, 16, 16), BlockCase(2, 32, 48)]     # one 16 x 16 tile; 2 x 3 tiles on each of two images
BLOCK_BASE = (1 / 8, 1 / 16, 1 / 16)     # keeps the three layers' activations near the size of x and of the shifts


def block_operands(case):
    rng = _rng(case.id)
    x = _ints(rng, 4, (case.b, case.h, case.w, 256))
    o = dict(x=x, w1=_ints(rng, 1, (64, 1, 1, 256)), w2=_ints(rng, 1, (64, 3, 3, 64)), w3=_ints(rng, 1, (256, 1, 1, 64)))
    for i, n in ((1, 64), (2, 64), (3, 256)):
        o[f"s{i}"], o[f"t{i}"] = channel_scale(n) * BLOCK_BASE[i - 1], channel_shift(n)
    return o


def block_eval(case, o, mut=None):
    pre1 = affine(conv64(o["x"], o["w1"]), o["s1"], o["t1"])
    a1 = relu(pre1)
    pre2 = affine(conv64(a1, o["w2"], (1, 1, 1, 1), mut=mut), o["s2"], o["t2"])
    a2 = relu(pre2)
    pre3 = affine(conv64(a2, o["w3"]), o["s3"], o["t3"])
    want = relu(pre3) + o["x"] if mut == "residual_after_relu" else relu(pre3 + o["x"])
    return dict(pre1=pre1, a1=a1, pre2=pre2, a2=a2, pre3=pre3 + o["x"], want=want + 0.0)


@functools.lru_cache(maxsize=2)
def build_block(case):
    o = block_operands(case)
    e = block_eval(case, o)
    bud = Budget()
    c1 = conv_abs(o["x"], o["w1"])
    bud.add("conv1 sums", c1, 1.0)
    g1 = bud.affine("conv1 affine", c1, 1.0, o["s1"], o["t1"])
    c2 = wino_abs(e["a1"], o["w2"])
    bud.add("conv2 winograd sums", c2, g1 / 4)
    g2 = bud.affine("conv2 affine", c2, g1 / 4, o["s2"], o["t2"])
    c3 = conv_abs(e["a2"], o["w3"])
    bud.add("conv3 sums", c3, g2)
    bud.affine("conv3 affine + residual", c3, g2, o["s3"], o["t3"], extra=4.0)
    return _data(**o, **e, budget=bud, f16_operands=(), relu_layers={k: e[k] for k in ("pre1", "pre2", "pre3")}, rounded={})


# ---------------------------------------------------------------------------------------------------------------------
# stem: conv 7x7 stride 2 pad 3 + affine + ReLU (ops.stem_conv, three forms), then SamePad (0, 1) + max-pool 3/2
# (ops.stem_pool_f32, ops.stem_pool_f16). Image [B,3,H,W], weights [64,7,7,4] with channel 3 zero, integers in [-3,3]
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class StemCase:
    op: str         # "conv_nhwc", "conv_nchw", "conv_f16" (stem_conv's three forms); "pool_f32", "pool_f16"
    b: int
    h: int
    w: int
    dead: bool = False    # every shift so negative that the whole ReLU map is zero

    @property
    def id(self):
        return f"stem-{self.op}-{self.b}x{self.h}x{self.w}" + ("-dead" if self.dead else "")

    @property
    def f16_image(self):
        return self.op == "pool_f16" and not self.dead

    @property
    def out16(self):
        return self.op in ("conv_f16", "pool_f16")


STEM_CONV_SHAPES = [(1, 2, 2), (2, 38, 70), (3, 32, 16)]      # one output pixel; ragged 16 x 16-output tiles; three images
STEM_POOL_SHAPES = [(1, 4, 4), (3, 16, 16), (2, 60, 132)]     # 1 x 1 pooled; ...; pooled 15 x 33: no multiple of 7 (8) rows or 16 columns
STEM_CASES = ([StemCase(op, *s) for op in ("conv_nhwc", "conv_nchw", "conv_f16") for s in STEM_CONV_SHAPES] +
              [StemCase(op, *s) for op in ("pool_f32", "pool_f16") for s in STEM_POOL_SHAPES] +
              [StemCase(op, 2, 24, 36, dead=True) for op in ("pool_f32", "pool_f16")])
STEM_DEAD_SHIFT = -float(2 ** 18)


def stem_operands(case):
    rng = _rng(case.id)
    if case.f16_image:      # multiples of 1/64 in [-128, 127]: 14 significant bits, so the kernel's fp32 -> fp16 conversion rounds
        img = rng.integers(-128 * 64, 127 * 64 + 1, (case.b, case.h, case.w, 3)).astype(np.float64) / 64.0
    else:
        img = rng.integers(-128, 128, (case.b, case.h, case.w, 3)).astype(np.float64)
    w = np.zeros((64, 7, 7, 4))
    w[..., :3] = _ints(rng, 3, (64, 7, 7, 3))
    shift = channel_shift(64) + (STEM_DEAD_SHIFT if case.dead else 0.0)
    return dict(img=img, w=w, scale=channel_scale(64), shift=shift)      # img NHWC with 3 channels


def stem_eval(case, o, mut=None):
    x = r16(o["img"], _tr(mut, "image")) if case.op == "pool_f16" else o["img"]     # the kernel's fp32 -> fp16 conversion of the image
    pre = affine(conv64(x, o["w"][..., :3], (3, 3, 3, 3), 2, mut=mut), o["scale"], o["shift"])
    act_exact = relu(pre)
    act = r16(act_exact, _tr(mut, "act")) if case.out16 else act_exact
    e = dict(x=x, pre=pre, act_exact=act_exact, act=act, want=act + 0.0)
    if case.op.startswith("pool"):
        # SamePad2d(3, 2) on an even conv size: ONE zero row / column at the bottom / right, (top, left, bottom, right) = (0, 0, 1, 1)
        pad = (1, 0, 1, 0) if mut == "pool_pad_top_left" else (0, 1, 0, 1)        # F.pad order: left, right, top, bottom
        t = F.pad(torch.from_numpy(act).permute(0, 3, 1, 2), pad)
        e["want"] = F.max_pool2d(t, 3, 2).permute(0, 2, 3, 1).contiguous().numpy() + 0.0
    return e


@functools.lru_cache(maxsize=2)
def build_stem(case):
    o = stem_operands(case)
    e = stem_eval(case, o)
    bud = Budget()
    g = 1 / 64 if case.f16_image else 1.0
    a = conv_abs(e["x"], o["w"][..., :3], (3, 3, 3, 3), 2)
    bud.add("conv sums", a, g)
    bud.affine("affine", a, g, o["scale"], o["shift"])
    rounded = {}
    if case.f16_image:
        rounded["image"] = (o["img"], e["x"])
    if case.out16 and not case.dead and case.h > 2:     # a 2 x 2 image has 12 live taps of 147: its sums need few bits
        rounded["act"] = (e["act_exact"], e["act"])
    return _data(**o, **e, budget=bud, f16_operands=(), relu_layers={} if case.dead else {"pre": e["pre"]}, rounded=rounded)


# ---------------------------------------------------------------------------------------------------------------------
# ops.bottleneck_c2_f16: identity block (Cin 256) and first block (Cin 64 with the downsample branch), fp16 in and out
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class C2Case:
    b: int
    h: int
    w: int
    first: bool

    @property
    def id(self):
        return f"c2f16-{'first' if self.first else 'identity'}-{self.b}x{self.h}x{self.w}"

    @property
    def cin(self):
        return 64 if self.first else 256


C2_SHAPES = [(1, 8, 16), (1, 5, 3), (3, 21, 37)]       # one 8 x 16 tile; sub-tile; ragged tiles and images
C2_CASES = [C2Case(*s, first) for first in (False, True) for s in C2_SHAPES]
C2_BASE = (1 / 16, 1 / 32, 1 / 16, 1 / 4)              # conv1, conv2, conv3, downsample
C2_BASE3_FIRST = 1 / 8    # the first block's residual (the downsample branch) reaches 170 where x reaches 4: with 1/16 the last
#                           sum needs 23.4 of the 24 bits, with 1/8 one less
# conv1's fp16 map (<= 10 bits per value) and the downsample branch (<= 8.2) are fp16 values as they are: `rounded` does not
# claim them. A downsample branch that rounded would need shifts near 2048, where no output is left for the ReLU to cut.


def c2_operands(case):
    rng = _rng(case.id)
    o = dict(x=_ints(rng, 4, (case.b, case.h, case.w, case.cin)), w1=_ints(rng, 2, (64, 1, 1, case.cin)),
             w2=_ints(rng, 2, (64, 3, 3, 64)), w3=_ints(rng, 2, (256, 1, 1, 64)))
    for i, n in ((1, 64), (2, 64), (3, 256)):
        o[f"s{i}"], o[f"t{i}"] = channel_scale(n) * C2_BASE[i - 1], channel_shift(n)
    if case.first:
        o["s3"] = channel_scale(256) * C2_BASE3_FIRST
        o["wd"] = _ints(rng, 2, (256, 1, 1, 64))
        o["sd"], o["td"] = channel_scale(256) * C2_BASE[3], channel_shift(256)
    return o


def c2_eval(case, o, mut=None):
    pre1 = affine(conv64(o["x"], o["w1"]), o["s1"], o["t1"])
    a1 = r16(relu(pre1), _tr(mut, "conv1"))
    pre2 = affine(conv64(a1, o["w2"], (1, 1, 1, 1), mut=mut), o["s2"], o["t2"])
    a2 = r16(relu(pre2), _tr(mut, "conv2"))
    pre3 = affine(conv64(a2, o["w3"]), o["s3"], o["t3"])
    res_exact = affine(conv64(o["x"], o["wd"]), o["sd"], o["td"]) if case.first else o["x"]
    res = r16(res_exact, _tr(mut, "downsample"))         # the downsample branch as the per-layer path leaves it in memory: fp16 (x is fp16 already)
    out_exact = relu(pre3) + res if mut == "residual_after_relu" else relu(pre3 + res)
    return dict(pre1=pre1, a1_exact=relu(pre1), a1=a1, pre2=pre2, a2_exact=relu(pre2), a2=a2, pre3=pre3 + res, res_exact=res_exact,
                res=res, out_exact=out_exact, want=r16(out_exact, _tr(mut, "out")) + 0.0)


@functools.lru_cache(maxsize=2)
def build_c2(case):
    o = c2_operands(case)
    e = c2_eval(case, o)
    bud = Budget()
    c1 = conv_abs(o["x"], o["w1"])
    bud.add("conv1 sums", c1, 1.0)
    g1 = bud.affine("conv1 affine", c1, 1.0, o["s1"], o["t1"])
    c2 = conv_abs(e["a1"], o["w2"], (1, 1, 1, 1))
    bud.add("conv2 sums", c2, g1)
    g2 = bud.affine("conv2 affine", c2, g1, o["s2"], o["t2"])
    c3 = conv_abs(e["a2"], o["w3"])
    bud.add("conv3 sums", c3, g2)
    gd = 1.0
    if case.first:
        cd = conv_abs(o["x"], o["wd"])
        bud.add("downsample sums", cd, 1.0)
        gd = bud.affine("downsample affine", cd, 1.0, o["sd"], o["td"])
    bud.affine("conv3 affine + residual", c3, g2, o["s3"], o["t3"], extra=float(np.abs(e["res"]).max()), g_extra=gd)
    f16 = ("x", "w1", "w2", "w3") + (("wd",) if case.first else ())
    rounded = {"conv2": (e["a2_exact"], e["a2"]), "out": (e["out_exact"], e["want"])}
    return _data(**o, **e, budget=bud, f16_operands=f16, relu_layers={k: e[k] for k in ("pre1", "pre2", "pre3")}, rounded=rounded)


# ---------------------------------------------------------------------------------------------------------------------
# ops.mask_tail_f16: deconv 2x2 stride 2 + bias + ReLU (fp16) -> conv5 1x1 + bias -> sigmoid, (R, h, w, classes)
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class TailCase:
    r: int
    h: int
    w: int
    classes: int

    @property
    def id(self):
        return f"tail-{self.r}x{self.h}x{self.w}x{self.classes}"


TAIL_CASES = [TailCase(1, 5, 3, 81),      # fewer than 256 pixels
              TailCase(3, 14, 14, 81),    # ragged pixel sets
              TailCase(7, 14, 14, 2), TailCase(2, 9, 14, 96)]     # the store tails
TAIL_XQ, TAIL_XR = 11, 192      # x = n * 2^-11, |n| <= 192
TAIL_W5Q = 4                    # conv5 weights: {-1, 0, 1} * 2^-4


def tail_operands(case):
    rng = _rng(case.id)
    x = _ints(rng, TAIL_XR, (case.r, case.h, case.w, 256)) / 2.0 ** TAIL_XQ
    wde = _ints(rng, 2, (4 * 256, 1, 1, 256))      # the deconv's GEMM weight: row (dy*2+dx)*256 + co
    w5 = _ints(rng, 1, (case.classes, 1, 1, 256)) / 2.0 ** TAIL_W5Q
    return dict(x=x, wde=wde, bde=channel_shift(256), w5=w5, b5=channel_shift(case.classes))


def tail_eval(case, o, mut=None):
    r, h, w = case.r, case.h, case.w
    cols = conv64(o["x"], o["wde"])                                           # [R,h,w,4*256]
    if mut == "shift_tap":      # sub-pixel (1, 1) reads the pixel to its left
        cols[..., 768:] = conv64(np.roll(o["x"], 1, 2), o["wde"][768:])
    de = cols.reshape(r, h, w, 2, 2, 256).transpose(0, 1, 3, 2, 4, 5).reshape(r, 2 * h, 2 * w, 256) + o["bde"]
    mid_exact = relu(de)
    mid = r16(mid_exact, _tr(mut, "deconv"))
    pre = conv64(mid, o["w5"]) + o["b5"]
    return dict(de=de, mid_exact=mid_exact, mid=mid, pre=pre, want=1.0 / (1.0 + np.exp(-pre)))


def tail_deconv_torch(case, o):
    """The deconv of tail_eval through F.conv_transpose2d (weight [Cin, Cout, 2, 2]) — the host test ties the two together."""
    wt = torch.from_numpy(o["wde"].reshape(2, 2, 256, 256)).permute(3, 2, 0, 1).contiguous()
    y = F.conv_transpose2d(torch.from_numpy(o["x"]).permute(0, 3, 1, 2), wt, torch.from_numpy(o["bde"]), stride=2)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


@functools.lru_cache(maxsize=2)
def build_tail(case):
    o = tail_operands(case)
    e = tail_eval(case, o)
    bud = Budget()
    g = 2.0 ** -TAIL_XQ
    a = conv_abs(o["x"], o["wde"])
    bud.add("deconv sums", a, g)
    bud.add("deconv + bias", a + 5, g)
    a5 = conv_abs(e["mid"], o["w5"])
    g5 = g * 2.0 ** -TAIL_W5Q
    bud.add("conv5 sums", a5, g5)
    bud.add("conv5 + bias", a5 + 5, g5)
    return _data(**o, **e, budget=bud, f16_operands=("x", "wde", "w5"), relu_layers={"de": e["de"]},
                 rounded={"deconv": (e["mid_exact"], e["mid"])})


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = {
    # name: (cases, build, operands, eval, the operand the input mutants change, the mutants that apply)
    "wino": (WINO_CASES, build_wino, wino_operands, wino_eval, "x", ("shift_tap", "edge_pad")),
    "heads": (HEADS_CASES, build_heads, heads_operands, heads_eval, "x", ("shift_tap", "edge_pad", "trunc")),
    "block32": (BLOCK_CASES, build_block, block_operands, block_eval, "x", ("shift_tap", "edge_pad", "residual_after_relu")),
    "stem": (STEM_CASES, build_stem, stem_operands, stem_eval, "img", ("shift_tap", "edge_pad", "trunc", "pool_pad_top_left")),
    "c2f16": (C2_CASES, build_c2, c2_operands, c2_eval, "x", ("shift_tap", "edge_pad", "trunc", "residual_after_relu")),
    "tail": (TAIL_CASES, build_tail, tail_operands, tail_eval, "x", ("shift_tap", "trunc")),
}
ALL_CASES = [c for fam in FAMILIES.values() for c in fam[0]]


def family_of(case):
    return case.id.split("-")[0]


def out_dtype(case):
    f16 = family_of(case) == "c2f16" or (family_of(case) == "stem" and case.out16)
    return np.float16 if f16 else np.float32


def build(case):
    """The operands (float64 arrays holding the exact values, NHWC / OHWI), every intermediate, `want64` (the expected output
    in float64, zeros normalised to +0) and `want`: the same in the output's own type (F(2x2) plain: one per (scale, ReLU)
    variant, NHWC — wino_layout gives the other layouts). `budget`: the exactness ledger; `rounded`: (exact, rounded) of every
    fp16 intermediate that is claimed to round; `relu_layers`: the pre-activations of every ReLU."""
    d = FAMILIES[family_of(case)][1](case)
    if not hasattr(d, "want64"):
        d.want64 = d.want
        dt = out_dtype(case)
        d.want = {k: v.astype(dt) for k, v in d.want64.items()} if isinstance(d.want64, dict) else d.want64.astype(dt)
    return d


def wino_layout(y, out):
    """NHWC -> what ops.conv3x3_winograd returns for `out`: "nhwc", "kblocked" [Cout/8,B,H,W,8] or "both"."""
    return y if out == "nhwc" else kblocked(y) if out == "kblocked" else (y, kblocked(y))


def coverage_problems(cases=None):
    """What the table lacks of the shapes, layouts, tilings, block kinds and kernel forms it promises ([] = nothing)."""
    cases = ALL_CASES if cases is None else cases
    have = {c.id for c in cases}
    need = [f"wino-{t}-" + "x".join(map(str, s)) for t, shapes in WINO_SHAPES.items() for s in shapes]
    need += ["heads-wino-1x16x16x8x64", "heads-wino-2x20x36x16x128"]
    need += ["block32-1x16x16", "block32-2x32x48"]
    need += [f"stem-{op}-{b}x{h}x{w}" for op in ("conv_nhwc", "conv_nchw", "conv_f16") for b, h, w in STEM_CONV_SHAPES]
    need += [f"stem-{op}-{b}x{h}x{w}" for op in ("pool_f32", "pool_f16") for b, h, w in STEM_POOL_SHAPES]
    need += [f"c2f16-{k}-{b}x{h}x{w}" for k in ("identity", "first") for b, h, w in C2_SHAPES]
    need += ["tail-1x5x3x81", "tail-3x14x14x81", "tail-7x14x14x2", "tail-2x9x14x96"]
    out = [f"missing: {n}" for n in need if n not in have]
    f16p = [c for c in cases if c.id.startswith("heads-f16p-")]
    if len(f16p) < 2 or not any((c.b * c.h * c.w) % 128 and c.b * c.h * c.w > 256 for c in f16p):
        out.append("missing: two conv_f16_pipelined_heads shapes, one with a ragged last tile")
    for op in ("pool_f32", "pool_f16"):
        if not any(c.id.startswith(f"stem-{op}-") and c.dead for c in cases if family_of(c) == "stem"):
            out.append(f"missing: the all-zero ReLU map for stem {op}")
    return out
