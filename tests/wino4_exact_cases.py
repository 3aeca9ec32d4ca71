"""Cases, data, float64 references and mutants of the exact-data sweep over the Winograd F(4x4, 3x3) kernels of
csrc/conv_wino4.hip — the plain conv, the form with the RPN heads and the form with the Bottleneck's conv3 — and over their
filter transform wino4_weights_kernel. tests/test_wino4_exact_host.py checks the data without a GPU,
tests/test_gpu_wino4_exact.py runs the kernels. The twin of tests/fused_exact_cases.py.

G of F(4x4) holds 64/81, 32/81 and 8/27, so U = G g G^T is not dyadic for integer g and no CONVOLUTION is exact in fp32. But G
never reaches the conv kernels: every entry point takes the transformed filter U as an operand and evaluates the bilinear form

    Y = A^T [ sum_c U_c .* (B^T d_c B) ] A

whose matrices B^T and A^T hold dyadic rationals only (points 0, +-3/4, +-3/2, inf). So the kernels are handed a SYNTHETIC U of
small integers: then every V = B^T d B, product, partial sum and output is a multiple of a known granule, exact in fp32 in any
order while the absolute evaluation |A^T| [sum_c |U| .* (|B^T||d||B|)] |A| stays below 2^24 granules — and the kernel must equal
a float64 evaluation of the same form bit for bit. The result is no convolution and need not be one: it pins indexing, padding,
staging, layouts, both transforms and the epilogues; the tolerance tests of tests/test_gpu_conv.py keep showing that the
algorithm is a convolution.

36 non-zero components per output channel would need about 35 bits. With ONE non-zero component (xi, nu) per output channel the
output transform adds zeros only, pixel (i, j) is A^T[i][xi] A^T[j][nu] M, and the sum fits for K = sum_c |U_c| up to k_table().
B^T, A^T and the layouts below are written from the kernel's comments, as a second statement of them, not imported from ops.py:
  u        [Cin/4][36 components xi*6+nu][2 channel pairs][Cout][2]       (xi: the transform along y, nu: along x)
  x        k-blocked [Cin/8][B*H*W][8];   output NHWC and / or k-blocked [Cout/8][B*H*W][8]
  heads    rows mt*512 + position*16 + i*4 + j of 32 columns, M tile mt = (b, 4-position block row, 8-position block column),
           position = row*8 + column inside the block; rows of positions outside the image hold the form evaluated on the
           image extended by zeros (the kernel stages zeros there and stores every row)
The filter transform is pinned separately: the denominators of G . G^T divide 3^10, so for g = 3^10 * {-2..2} * 2^k every U
entry is a short integer, and the kernel's double arithmetic and its cast to fp32 are exact."""
import dataclasses
import functools
from fractions import Fraction

import numpy as np

from conv_exact_cases import channel_scale, channel_shift, kblocked  # noqa: F401  (kblocked: for the GPU test)
from fused_exact_cases import Budget, _data, _rng, relu

# ---------------------------------------------------------------------------------------------------------------------
# the matrices, from the comments above bt3() and at4p() in csrc/conv_wino4.hip: points 0, +a, -a, +b, -b, inf
# ---------------------------------------------------------------------------------------------------------------------
_a, _b = 0.75, 1.5
_a2, _b2 = _a * _a, _b * _b
BT = np.array([[_a2 * _b2, 0, -(_a2 + _b2), 0, 1, 0],
               [0, -_a * _b2, -_b2, _a, 1, 0],
               [0, _a * _b2, -_b2, -_a, 1, 0],
               [0, -_a2 * _b, -_a2, _b, 1, 0],
               [0, _a2 * _b, -_a2, -_b, 1, 0],
               [0, _a2 * _b2, 0, -(_a2 + _b2), 0, 1]])
AT = np.array([[1, 1, 1, 1, 1, 0],
               [0, _a, -_a, _b, -_b, 0],
               [0, _a2, _a2, _b2, _b2, 0],
               [0, _a2 * _a, -_a2 * _a, _b2 * _b, -_b2 * _b, 1]])
POINTS = (Fraction(0), Fraction(3, 4), Fraction(-3, 4), Fraction(3, 2), Fraction(-3, 2))      # + inf: index 5


def _den(v):
    return Fraction(float(v)).denominator       # a float IS a dyadic rational: its exact denominator


BT_DEN = np.array([max(_den(v) for v in row) for row in BT], dtype=np.float64)                 # 64 16 16 32 32 64
BT_ROWABS = np.abs(BT).sum(1) * BT_DEN               # sum |B^T[xi]| in units of the row's granule, for |d| <= 1
AT_DEN = np.array([[_den(v) for v in row] for row in AT], dtype=np.float64)                    # [4][6]
AT_NUM = np.abs(AT) * AT_DEN                         # |A^T[i][xi]| in units of its own granule
G_V = 1.0 / (BT_DEN[:, None] * BT_DEN[None, :])      # granule of V, of U . V and of their sums at component (xi, nu)
# granule of output pixel (i, j) at component (xi, nu), [xi][nu][i][j]; 1 where A^T has a zero (the output is 0 there)
G_OUT = G_V[:, :, None, None] / (AT_DEN.T[:, None, :, None] * AT_DEN.T[None, :, None, :])
LIVE = (AT.T[:, None, :, None] != 0) & (AT.T[None, :, None, :] != 0)                          # [xi][nu][i][j]
MIN_SCALE = 0.5                                      # the smallest channel_scale
SHIFT_MAX = 5.0                                      # the largest |channel_shift|


def point_class(p):
    return "E" if p in (0, 5) else "3/4" if p in (1, 2) else "3/2"


def fits(xi, nu, k, terms=1, shift_unit=0.0, extra=0.0):
    """Do `terms` channels of component (xi, nu) with sum |U| = k each, |d| <= 1 at the worst pixel of a tile, every one
    scaled by >= MIN_SCALE and shifted by at most SHIFT_MAX * shift_unit, plus `extra` (a bias, a residual), stay below 2^24
    granules at every output pixel (i, j)? From first principles: |V| <= rowabs[xi] rowabs[nu] granules of V, the output
    transform multiplies by the numerators of A^T[i][xi] A^T[j][nu]."""
    acc = k * BT_ROWABS[xi] * BT_ROWABS[nu] * AT_NUM[:, xi][:, None] * AT_NUM[:, nu][None, :]        # [i][j], in granules
    g = G_OUT[xi, nu] * MIN_SCALE
    total = terms * (acc + SHIFT_MAX * shift_unit / g) + extra / g
    return bool((total[LIVE[xi, nu]] < 2.0 ** 24).all())


def k_table(xi, nu):
    """The largest K = sum_c |U_c| that is exact for component (xi, nu) with |d| <= 1 and nothing added."""
    unit = BT_ROWABS[xi] * BT_ROWABS[nu] * AT_NUM[:, xi].max() * AT_NUM[:, nu].max()
    return int((2 ** 24 - 1) // unit)


def k_use(xi, nu, terms=1, shift_unit=0.25, extra=0.0):
    """The K a case gives a channel of component (xi, nu): the largest that fits() beside the shift (0: none does)."""
    k = k_table(xi, nu)
    while k > 0 and not fits(xi, nu, k, terms, shift_unit, extra):
        k -= 1
    return k


# ---------------------------------------------------------------------------------------------------------------------
# the bilinear form in float64
# ---------------------------------------------------------------------------------------------------------------------
def grid(h, w):
    """4 x 8-position blocks per image along y / x (wino4_tile_rows / wino4_tile_cols of csrc/conv_common.hpp)."""
    return -(-(h // 4) // 4), -(-(w // 4) // 8)


def _patches(xp, ty, tx):
    """The 6 x 6 patches (stride 4) of the padded map -> [B,ty,tx,6,6,C]."""
    return np.stack([np.stack([xp[:, i:i + 4 * ty:4, j:j + 4 * tx:4] for j in range(6)], 3) for i in range(6)], 3)


def transform_input(x, mut=None, mats=(BT,)):
    """V = B^T d B of every position of the BLOCK grid (the positions beyond the image see the image extended by zeros, as the
    kernel stages it) -> [B, GY, GX, 6, 6, C]. mut "edge_pad": the pad replicates the edge."""
    b, h, w, c = x.shape
    tyb, txb = grid(h, w)
    gy, gx = 4 * tyb, 8 * txb
    xp = np.zeros((b, 4 * gy + 2, 4 * gx + 2, c), dtype=x.dtype)
    if mut == "edge_pad":
        xp[:, :h + 2, :w + 2] = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
    else:
        xp[:, 1:h + 1, 1:w + 1] = x
    m = mats[0].astype(x.dtype)
    return np.einsum("pi,btuijc,qj->btupqc", m, _patches(xp, gy, gx), m, optimize=True)


def _contract(v, u):
    """M = sum_c V[.., xi, nu, c] U[o, xi, nu, c], component by component, for the output channels that have an entry there:
    yields (xi, nu, channels, M [B, GY, GX, len(channels)])."""
    for xi in range(6):
        for nu in range(6):
            sel = np.nonzero(u[:, xi, nu].any(1))[0]
            if len(sel):
                yield xi, nu, sel, v[:, :, :, xi, nu] @ u[sel, xi, nu].T


_U_MUTANTS = {"transpose_components": lambda u: u.transpose(0, 2, 1, 3), "swap_34": lambda u: u[:, [0, 2, 1, 3, 4, 5]],
              "swap_32": lambda u: u[:, [0, 1, 2, 4, 3, 5]], "swap_pair_channels": lambda u: u[..., np.arange(u.shape[3]) ^ 1],
              "swap_pairs": lambda u: u[..., np.arange(u.shape[3]) ^ 2], "swap_ktiles": lambda u: u[..., np.arange(u.shape[3]) ^ 4]}


def bilinear(x, u, mut=None):
    """Y = A^T [sum_c U_c .* (B^T d_c B)] A on the block grid, float64: x [B,H,W,C] NHWC, u [O,6,6,C] ->
    [B, 16*tyb, 32*txb, O] (the image is its top left H x W). Every mutant is ONE thing wrong."""
    v = transform_input(x, mut)
    if mut in _U_MUTANTS:
        u = np.ascontiguousarray(_U_MUTANTS[mut](u))
    if mut == "shift_tile_x":
        v = np.roll(v, 1, 2)
    if mut == "shift_tile_y":
        v = np.roll(v, 1, 1)
    y = np.zeros(v.shape[:3] + (4, 4, u.shape[0]))
    for xi, nu, sel, m in _contract(v, u):
        y[..., sel] += (AT[:, xi][:, None, None] * AT[:, nu][None, :, None]) * m[:, :, :, None, None, :]
    if mut == "swap_n32":        # linear per channel: the accumulators of the two 32-channel halves of an N tile change places
        y = y[..., np.arange(y.shape[-1]) ^ 32]
    if mut == "transpose_pixel":
        y = y.swapaxes(3, 4)
    b, gy, gx = y.shape[:3]
    return np.ascontiguousarray(y.transpose(0, 1, 3, 2, 4, 5).reshape(b, 4 * gy, 4 * gx, -1))


def bilinear32(x, u, reverse):
    """The same form in fp32 throughout, the channel sum one channel at a time, forward or backward: what the host test
    compares with float64."""
    v = transform_input(x.astype(np.float32))
    assert v.dtype == np.float32
    uu = u.astype(np.float32)
    m = np.zeros(v.shape[:5] + (u.shape[0],), dtype=np.float32)
    order = range(x.shape[3])
    for c in (reversed(order) if reverse else order):
        m += v[..., c, None] * uu[..., c].transpose(1, 2, 0)
    at = AT.astype(np.float32)
    t = np.zeros(m.shape[:3] + (6, 4) + m.shape[5:], dtype=np.float32)          # along nu first, as the kernel does
    for q in (range(5, -1, -1) if reverse else range(6)):
        t += m[:, :, :, :, q, None, :] * at[:, q][:, None]
    y = np.zeros(m.shape[:3] + (4, 4) + m.shape[5:], dtype=np.float32)
    for p in (range(5, -1, -1) if reverse else range(6)):
        y += t[:, :, :, p, None] * at[:, p][:, None, None]
    b, gy, gx = y.shape[:3]
    return np.ascontiguousarray(y.transpose(0, 1, 3, 2, 4, 5).reshape(b, 4 * gy, 4 * gx, -1))


def u_layout(u):
    """u [O,6,6,C] -> the kernel's [C/4][36][2 channel pairs][O][2]."""
    o, c = u.shape[0], u.shape[3]
    return np.ascontiguousarray(u.reshape(o, 36, c // 4, 2, 2).transpose(2, 1, 3, 0, 4))


def head_rows(grid_map, h, w):
    """[B, 16*tyb, 32*txb, N] on the block grid -> the heads' M-tile-major rows [B*tyb*txb*512, N]."""
    b, n = grid_map.shape[0], grid_map.shape[3]
    tyb, txb = grid(h, w)
    v = grid_map.reshape(b, tyb, 4, 4, txb, 8, 4, n).transpose(0, 1, 4, 2, 5, 3, 6, 7)
    return np.ascontiguousarray(v.reshape(-1, n))


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    form: str       # "plain", "heads", "conv3"
    b: int
    h: int
    w: int
    cin: int
    cout: int
    c3: int = 0
    tag: str = ""   # "clamp": w stands for one row of M tiles past the persistent-grid clamp of the device

    @property
    def id(self):
        return f"w4-{self.form}-{self.b}x{self.h}x{self.w}x{self.cin}x{self.cout}" + (f"-c3_{self.c3}" if self.c3 else "") + \
            (f"-{self.tag}" if self.tag else "")

    @property
    def shift_unit(self):
        return 0.25 if self.form == "plain" else 1.0 / 16


def over_the_clamp(cus):
    """M tiles in one row that put a one-workgroup-per-CU persistent launcher just over its clamp: between one and two times
    the CU count and no multiple of 8 (the rule of tests/test_gpu_conv.py's _over_the_clamp)."""
    units = cus + 1
    while units % 8 == 0 or units < cus + 4:
        units += 1
    assert cus < units < 2 * cus
    return units


PLAIN_SHAPES = [(1, 4, 4, 8, 64),         # a single position
                (1, 16, 32, 8, 64),       # exactly one M tile
                (2, 20, 28, 24, 128),     # ragged 5 x 7 positions, 6 k tiles (the ring wraps), two N tiles, two images
                (1, 36, 40, 16, 256),     # four N tiles
                (3, 16, 32, 40, 64)]      # image i against image i alone
HEADS_SHAPES = [(1, 16, 32, 8, 128), (1, 16, 32, 8, 256), (2, 20, 28, 16, 128), (2, 20, 28, 8, 256), (2, 36, 40, 8, 128),
                (2, 36, 40, 16, 256),     # two and four N tiles each
                (1, 96, 96, 8, 128)]      # 6 x 3 = 18 M tiles in one image: trem >> W4_WALK_SHIFT is 1 for the last two, whose
#                                           N-tile walk starts at N tile 1
CONV3_SHAPES = [(1, 16, 32, 8, 32), (1, 20, 44, 16, 96), (2, 4, 4, 8, 256), (1, 16, 32, 8, 256), (1, 20, 44, 8, 32),
                (2, 4, 4, 24, 96)]        # (B, H, W, Cin, c3); Cout is 64


def cases(cus=256):
    wide = 32 * over_the_clamp(cus)
    out = [Case("plain", *s) for s in PLAIN_SHAPES] + [Case("plain", 1, 4, wide, 8, 64, tag="clamp")]
    out += [Case("heads", *s) for s in HEADS_SHAPES] + [Case("heads", 1, 4, wide, 8, 128, tag="clamp")]
    out += [Case("conv3", b, h, w, cin, 64, c3) for b, h, w, cin, c3 in CONV3_SHAPES]
    return out


ALL_CASES = cases()
VARIANTS = [(s, r) for s in (False, True) for r in (False, True)]       # plain: (with scale and shift, with ReLU)
# the components of the 18 real head rows: (xi, nu) that take two channels and more (fits()), all four (+-3/4, +-3/4) among them
# — the only ones that reach every pixel of a tile with two channels; with E components the rows walk every N tile
HEAD_COMPS = [(1, 1), (0, 0), (0, 1), (1, 2), (5, 5), (1, 0), (2, 1), (0, 3), (5, 0), (2, 2), (4, 0), (0, 5), (5, 2), (2, 5), (5, 4),
              (3, 5), (0, 2), (1, 5)]
MAX_ENTRIES = 6       # non-zero input channels of an output channel, at most


def comp_of(o):
    """The one non-zero component of output channel o: every 64-channel N tile holds all 36 (32 channels cannot)."""
    k = ((o % 64) + 13 * (o // 64)) % 36
    return k // 6, k % 6


def _select(case):
    """heads / conv3: the conv channels every consumer row sums -> {row: [channels]}, all of ONE component (one granule), as
    many as fits() allows: heads one per N tile (at least two N tiles), conv3 the one or two of the single N tile."""
    rows = {}
    if case.form == "heads":
        nt = case.cout // 64
        for r, (xi, nu) in enumerate(HEAD_COMPS):
            n = nt
            while n > 1 and k_use(xi, nu, n, case.shift_unit, SHIFT_MAX * case.shift_unit) < 1:
                n -= 1
            tiles = [(r + t) % nt for t in range(n)]
            rows[r] = [next(o for o in range(64 * t, 64 * t + 64) if comp_of(o) == (xi, nu)) for t in sorted(tiles)]
    elif case.form == "conv3":
        for r in range(case.c3):
            xi, nu = divmod((r * 7) % 36, 6)
            have = [o for o in range(64) if comp_of(o) == (xi, nu)]
            n = len(have)
            while n > 1 and k_use(xi, nu, n, case.shift_unit, (SHIFT_MAX + 3) * case.shift_unit) < 1:
                n -= 1
            rows[r] = have[:n] if r % 2 == 0 else have[-n:]
    return rows


def operands(case):
    rng = _rng(case.id)
    b, h, w, cin, cout = case.b, case.h, case.w, case.cin, case.cout
    x = rng.integers(-1, 2, (b, h, w, cin)).astype(np.float64)
    rows = _select(case)
    terms = {}                                   # channel -> how many channels its consumer rows sum at most
    for r, sel in rows.items():
        for o in sel:
            terms[o] = max(terms.get(o, 1), len(sel))
    extra = 0.0 if case.form == "plain" else (SHIFT_MAX + (3 if case.form == "conv3" else 0)) * case.shift_unit
    u = np.zeros((cout, 6, 6, cin))
    ks = np.zeros(cout, dtype=np.int64)
    nxt = {}                                     # component -> the input channel its next entry takes
    salt = sum(ord(ch) for ch in case.id)
    prev = None
    for o in range(cout):
        xi, nu = comp_of(o)
        k = k_use(xi, nu, terms.get(o, 1), case.shift_unit, extra if o in terms else 0.0)
        assert k >= 1, (case.id, o, xi, nu)
        n = min(k, cin, MAX_ENTRIES)
        first = nxt.get((xi, nu), (xi * 6 + nu + salt) % cin)
        if prev == {(first + j) % cin for j in range(n)}:      # never the input channels of the channel before
            first = (first + 1) % cin
        prev = {(first + j) % cin for j in range(n)}
        vals = np.ones(n)
        left = k - n
        for j in range(1, n, 2):                 # powers of two where the budget has room
            for v in (4, 2):
                if left >= v - 1:
                    vals[j], left = v, left - (v - 1)
                    break
        u[o, xi, nu, (first + np.arange(n)) % cin] = vals * rng.choice([-1.0, 1.0], n)
        nxt[(xi, nu)] = (first + n) % cin
        ks[o] = int(vals.sum())
    d = dict(x=x, u=u, k=ks, scale=channel_scale(cout), shift=channel_shift(cout) * case.shift_unit, rows=rows)
    if case.form == "heads":
        wh = np.zeros((32, cout))
        for r, sel in rows.items():              # +-1 / scale: every term of a row has the row's granule again
            wh[r, sel] = rng.choice([-1.0, 1.0], len(sel)) / d["scale"][sel]
        d.update(w_head32=wh, bias=channel_shift(18) * case.shift_unit)
    if case.form == "conv3":
        w3 = np.zeros((case.c3, 64))
        for r, sel in rows.items():              # the first sign is +: conv2's map is >= 0, an all-negative row dies in the ReLU
            w3[r, sel] = rng.choice([-1.0, 1.0], len(sel)) * ([1.0] + [1.0] * (len(sel) - 1)) / d["scale"][sel]
            w3[r, sel[0]] = abs(w3[r, sel[0]])
        d.update(w3=w3, scale3=channel_scale(case.c3), shift3=channel_shift(case.c3) * case.shift_unit,
                 residual=rng.integers(-3, 4, (b, h, w, case.c3)).astype(np.float64) * case.shift_unit)
    return d


def evaluate(case, o, with_scale=True, with_relu=True, mut=None):
    """-> acc (the form on the block grid), act (affine + ReLU of it), want: plain NHWC [B,H,W,Cout]; heads (the raw rows
    [tiles*512, 32], to_nhwc [B,H,W,18]); conv3 NHWC [B,H,W,c3]. with_scale=False: neither scale nor shift (plain), scale3 /
    shift3 (conv3)."""
    h, w = case.h, case.w
    acc = bilinear(o["x"], o["u"], mut)
    plain = case.form == "plain"
    if plain and not with_scale:
        pre = acc
    elif mut == "shift_before_scale":
        pre = (acc + o["shift"]) * o["scale"]
    else:
        pre = acc * o["scale"] + o["shift"]
    act = pre + 0.0 if (mut == "no_relu" or (plain and not with_relu)) else relu(pre)
    e = dict(acc=acc, pre=pre, act=act)
    if plain:
        e["want"] = np.ascontiguousarray(act[:, :h, :w])
    elif case.form == "heads":
        wh = o["w_head32"]
        if mut == "drop_ntile":
            wh = wh.copy()
            wh[:, 64:128] = 0
        sums = act @ wh.T                                                  # on the block grid
        e["sums"] = sums
        e["want"] = (head_rows(sums, h, w) + 0.0, np.ascontiguousarray(sums[:, :h, :w, :18]) + o["bias"] + 0.0)
    else:
        sums = act[:, :h, :w] @ o["w3"].T
        e["sums"] = sums
        lin = sums * o["scale3"] + o["shift3"] if with_scale else sums
        e["pre3"] = lin + o["residual"]
        e["want"] = relu(lin) + o["residual"] if mut == "residual_after_relu" else relu(lin + o["residual"])
    return e


def _per_pixel(t):
    """[B, 16*ty, 32*tx, N] -> the largest value per pixel (i, j) of a tile and channel, [4][4][N]."""
    b, gh, gw, n = t.shape
    return t.reshape(b, gh // 4, 4, gw // 4, 4, n).max((0, 1, 3))


@functools.lru_cache(maxsize=2)
def build(case):
    """The operands, every intermediate, `want` per variant in float64 (`want64`) and fp32, and the exactness ledger."""
    o = operands(case)
    cout = case.cout
    comp = np.array([comp_of(n) for n in range(cout)])
    xi, nu = comp[:, 0], comp[:, 1]
    bud = Budget()
    # the absolute evaluation: |V| = |B^T||d||B|, M = sum_c |U||V| at the channel's component, per pixel |A^T| M |A|
    vabs = transform_input(np.abs(o["x"]), mats=(np.abs(BT),))
    mabs = np.zeros(cout)
    for _, _, sel, m in _contract(vabs, np.abs(o["u"])):
        mabs[sel] = m.max((0, 1, 2))
    bud.add("component sums", mabs, G_V[xi, nu])
    yabs = (np.abs(AT).T[xi][:, :, None] * np.abs(AT).T[nu][:, None, :] * mabs[:, None, None]).transpose(1, 2, 0)     # [4][4][O]
    g_out = G_OUT[xi, nu].transpose(1, 2, 0)                                                            # [4][4][O]
    live = LIVE[xi, nu].transpose(1, 2, 0)
    bud.add("outputs", yabs, g_out)
    unit = case.shift_unit
    g_aff = np.where(live, np.minimum(g_out * o["scale"], unit), unit)
    bud.add("affine", yabs * o["scale"] + np.abs(o["shift"]), g_aff)
    e = evaluate(case, o)
    want = {}
    if case.form == "plain":
        for s, r in VARIANTS:
            want[(s, r)] = e["want"] if (s, r) == (True, True) else evaluate(case, o, s, r)["want"]
    elif case.form == "heads":
        wabs = np.abs(o["w_head32"][:18])
        habs = _per_pixel(np.abs(e["act"]) @ wabs.T)                                                    # [4][4][18]
        hc = np.array(HEAD_COMPS)
        g_row = np.where(LIVE[hc[:, 0], hc[:, 1]], np.minimum(G_OUT[hc[:, 0], hc[:, 1]], unit / 4), unit / 4).transpose(1, 2, 0)
        bud.add("head sums", habs, g_row)
        bud.add("head sums + bias", habs + np.abs(o["bias"]), g_row)
        want[(True, True)] = e["want"]
    else:
        rc = np.array([comp_of(o["rows"][r][0]) for r in range(case.c3)])
        g3 = np.where(LIVE[rc[:, 0], rc[:, 1]], np.minimum(G_OUT[rc[:, 0], rc[:, 1]], unit / 4), unit / 4).transpose(1, 2, 0)
        habs = _per_pixel(np.abs(e["act"]) @ np.abs(o["w3"]).T)
        bud.add("conv3 sums", habs, g3)
        rmax = float(np.abs(o["residual"]).max())
        bud.add("conv3 affine + residual", habs * o["scale3"] + np.abs(o["shift3"]) + rmax, np.minimum(g3 * o["scale3"], unit))
        bud.add("conv3 + residual, no affine", habs + rmax, np.minimum(g3, unit))
        want[(True, True)] = e["want"]
        want[(False, True)] = evaluate(case, o, with_scale=False)["want"]
    f32 = lambda v: tuple(t.astype(np.float32) for t in v) if isinstance(v, tuple) else v.astype(np.float32)
    return _data(**o, **{k: v for k, v in e.items() if k != "want"}, comp=comp, want64=want, want={k: f32(v) for k, v in want.items()},
                 budget=bud)


# ---------------------------------------------------------------------------------------------------------------------
# mutants: ONE thing wrong in the reference; the host test asserts that each changes `want` in every case it applies to
# ---------------------------------------------------------------------------------------------------------------------
MUTANTS = ("transpose_components", "swap_34", "swap_32", "swap_pair_channels", "swap_pairs", "swap_ktiles", "shift_tile_x",
           "shift_tile_y", "transpose_pixel", "edge_pad", "swap_n32", "last_image", "shift_before_scale", "no_relu")
FORM_MUTANTS = {"plain": (), "heads": ("drop_ntile",), "conv3": ("residual_after_relu",)}


def mutants_of(case):
    m = [k for k in MUTANTS if k != "last_image" or case.b > 1]
    return m + list(FORM_MUTANTS[case.form])


def mutant_want(case, o, mut):
    if mut == "last_image":
        o = dict(o)
        o["x"] = o["x"].copy()
        o["x"][-1] = o["x"][0]
        mut = None
    return evaluate(case, o, mut=mut)["want"]


def flat(want):
    return np.concatenate([t.ravel() for t in want]) if isinstance(want, tuple) else want.ravel()


# ---------------------------------------------------------------------------------------------------------------------
# coverage: conditions, not measurements
# ---------------------------------------------------------------------------------------------------------------------
def coverage_problems(all_cases=None):
    all_cases = ALL_CASES if all_cases is None else list(all_cases)
    out = []
    ids = {c.id for c in all_cases}
    need = [Case("plain", *s).id for s in PLAIN_SHAPES] + [Case("heads", *s).id for s in HEADS_SHAPES]
    need += [Case("conv3", b, h, w, cin, 64, c3).id for b, h, w, cin, c3 in CONV3_SHAPES]
    out += [f"missing: {n}" for n in need if n not in ids]
    for form in ("plain", "heads"):
        if not any(c.form == form and c.tag == "clamp" for c in all_cases):
            out.append(f"missing: a {form} case over the persistent-grid clamp")
    heads = [c for c in all_cases if c.form == "heads"]
    for nt in (2, 4):
        for shape in ((1, 16, 32), (2, 20, 28), (2, 36, 40)):
            if not any((c.b, c.h, c.w) == shape and c.cout == 64 * nt for c in heads):
                out.append(f"missing: heads {shape} with {nt} N tiles")
    if not any(grid(c.h, c.w)[0] * grid(c.h, c.w)[1] > 16 for c in heads if not c.tag):
        out.append("missing: a heads case with more than 16 M tiles per image (walks that start mid-way)")
    conv3 = [c for c in all_cases if c.form == "conv3"]
    for c3 in (32, 96, 256):
        if not any(c.c3 == c3 for c in conv3):
            out.append(f"missing: conv3 with c3 = {c3}")
    for shape in ((1, 16, 32), (1, 20, 44), (2, 4, 4)):
        if not any((c.b, c.h, c.w) == shape for c in conv3):
            out.append(f"missing: conv3 {shape}")
    slots = set()
    for case in all_cases:
        o = operands(case)
        u = o["u"]
        nz = u != 0
        if not (nz.reshape(case.cout, -1, case.cin).any(2).sum(1) == 1).all():
            out.append(f"{case.id}: an output channel without exactly one non-zero component")
        comps = np.array([comp_of(n) for n in range(case.cout)])
        for t in range(case.cout // 64):
            have = {tuple(k) for k in comps[64 * t:64 * t + 64]}
            if len(have) != 36:
                out.append(f"{case.id}: N tile {t} holds {len(have)} of the 36 components")
        # (input channel, component): as many distinct input channels as the component's budget gives it entries
        per = nz.any(0).reshape(36, case.cin).sum(1)
        entries = nz.sum((0, 3)).reshape(36)
        if not (per == np.minimum(entries, case.cin)).all():
            out.append(f"{case.id}: a component's entries repeat an input channel before all are used")
        if case.form == "plain":
            slots |= {(k, c % 8) for k, c in zip(*np.nonzero(nz.any(0).reshape(36, case.cin)))}
        first = [tuple(np.nonzero(nz[n].any((0, 1)))[0]) for n in range(case.cout)]
        if any(a == b_ for a, b_ in zip(first, first[1:])):
            out.append(f"{case.id}: two neighbouring output channels read the same input channels")
        if case.form == "heads":
            wh = o["w_head32"]
            if wh[18:].any():
                out.append(f"{case.id}: rows 18..31 of w_head32 are not zero")
            pix = np.zeros((4, 4), dtype=bool)
            for r in range(18):
                sel = np.nonzero(wh[r])[0]
                if len(sel) < 2 or len({s // 64 for s in sel}) < 2:
                    out.append(f"{case.id}: head row {r} sums {len(sel)} channels of {len({s // 64 for s in sel})} N tiles")
                pix |= LIVE[comp_of(sel[0])]
            if not pix.all():
                out.append(f"{case.id}: a pixel of the tile is zero in every head row")
            if not (np.nonzero(wh.any(0))[0] // 64 == np.arange(case.cout // 64)[:, None]).any(1).all():
                out.append(f"{case.id}: an N tile feeds no head row")
        if case.form == "conv3" and not (np.count_nonzero(o["w3"], axis=1) >= 1).all():
            out.append(f"{case.id}: an empty row of w3")
    if len(slots) != 36 * 8 and {c.id for c in ALL_CASES if c.form == "plain"} <= ids:
        out.append(f"plain cases: {len(slots)} of the 288 (component, channel slot of an 8-channel plane) pairs have a non-zero U entry")
    return out


def data_problems(case, d):
    """The conditions on the reference's values ([] = none). At least 40 % of the outputs are non-zero — where a component has
    a zero row of A^T (xi or nu in {0, inf}: three of four pixel rows) the output is the shift alone, so without scale and
    shift the raw form has 9/16 of its pixels live and its ReLU'd variant half of that: that one variant is held to 25 %. No
    two output channels are equal BEFORE the last ReLU (after it a channel of a single-position case can be all zero)."""
    out = []
    for key, w in d.want64.items():
        t = w[-1] if isinstance(w, tuple) else w       # heads: the NHWC form (the raw rows hold 14 zero columns by construction)
        nzf = float(np.count_nonzero(t)) / t.size
        if nzf < (0.25 if case.form == "plain" and key == (False, True) else 0.4):
            out.append(f"{case.id} {key}: {nzf:.2f} of the reference outputs are non-zero")
    t = {"plain": lambda: d.pre[:, :case.h, :case.w], "heads": lambda: d.want64[(True, True)][1], "conv3": lambda: d.pre3}[case.form]()
    ch = t.reshape(-1, t.shape[-1]).T
    if len({c.tobytes() for c in ch}) != ch.shape[0]:
        out.append(f"{case.id}: two output channels are equal")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the filter transform: U = G g G^T, G row of point p = [1 p p^2] / prod_{q != p} (p - q), last row [0 0 1]
# ---------------------------------------------------------------------------------------------------------------------
def g_matrix():
    rows = []
    for p in POINTS:
        n = Fraction(1)
        for q in POINTS:
            if q != p:
                n *= p - q
        rows.append([1 / n, p / n, p * p / n])
    rows.append([Fraction(0), Fraction(0), Fraction(1)])
    return rows


WEIGHT_SHAPES = [(64, 8), (128, 24), (1, 4), (40, 12)]      # (Cout, Cin); 40: no multiple of 64
WEIGHT_REAL_SHAPES = [(64, 8), (1, 4), (40, 12)]


def filter_exact(g):
    """G g G^T of g [O,3,3,C] (integers held in float64) in exact rational arithmetic -> [O,6,6,C] of Fractions."""
    gm = np.array(g_matrix(), dtype=object)                                          # [6][3]
    gf = np.vectorize(lambda v: Fraction(float(v)), otypes=[object])(g)
    t = np.tensordot(gm, gf, axes=([1], [1]))                                        # [6][O][3][C]
    return np.tensordot(gm, t, axes=([1], [2])).transpose(2, 1, 0, 3)                # [6nu][6xi][O][C] -> [O][xi][nu][C]


def weights_int(cout, cin):
    """g = 3^10 * {-2..2} * channel_scale -> (g, U exact as float64)."""
    rng = _rng(f"w4-weights-{cout}x{cin}")
    g = 3.0 ** 10 * rng.integers(-2, 3, (cout, 3, 3, cin)) * channel_scale(cout)[:, None, None, None]
    u = filter_exact(g)
    assert all(v.denominator & (v.denominator - 1) == 0 for v in u.ravel())
    return g, u.astype(np.float64)


def round_f32(fr):
    """The Fraction rounded ONCE to fp32 (nearest; through float64 it would be rounded twice)."""
    f = np.float32(float(fr))
    best, err = f, abs(Fraction(float(f)) - fr)
    for cand in (np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))):
        e = abs(Fraction(float(cand)) - fr)
        if e < err:
            best, err = cand, e
    return best


def weights_real(cout, cin):
    """Random fp32 g -> (g, the exact U rounded once to fp32 [O,6,6,C])."""
    rng = _rng(f"w4-weights-real-{cout}x{cin}")
    g = rng.standard_normal((cout, 3, 3, cin)).astype(np.float32)
    u = filter_exact(g.astype(np.float64))
    return g, np.vectorize(round_f32, otypes=[np.float32])(u)
