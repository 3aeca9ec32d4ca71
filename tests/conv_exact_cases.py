"""Cases, data, float64 reference and input invariants of the exact-arithmetic sweep over the implicit-GEMM convs
(tests/test_conv_exact_host.py checks them without a GPU, tests/test_gpu_conv_exact.py runs them).

The data are small signed integers (times a power of two), so every product and every partial sum of the convolution is exactly
representable in fp32: the kernel must equal a float64 evaluation BIT FOR BIT in any summation order — the fp32 MFMA, the two
SPLIT chains, fp16 operands with fp32 accumulation and the fp16 x 3 split alike. Scale is a per-channel power of two cycling
through {0.5, 1, 2, 4}, shift a per-channel integer that differs between neighbouring channels, so a swapped or shifted channel,
pixel, tap or image changes the result.

A case names the route it is meant to reach (`family`, `mode`, `epi`); which instantiation the fp32 dispatcher really picks is
asked of the dispatcher itself (ops.conv_route) and compared with a hand-written table in the host test."""
import dataclasses
import functools

import numpy as np
import torch
import torch.nn.functional as F

Q_SPLIT = 13   # the fp16 x 3 families: operands n * 2^-13 with |n| <= 8191 need up to 13 significand bits (fp16 holds 11)


@dataclasses.dataclass(frozen=True)
class Case:
    family: str
    shape: str            # "ragged" / "pow2" / a word for the extras
    op: str               # "f32" conv_bn_act / deconv2x2, "f16mfma", "f16io", "f16p"
    b: int
    h: int
    w: int
    cin: int
    cout: int             # GEMM columns: 4 x the deconv's channels when out_mode == 1
    k: int = 1
    stride: int = 1
    pad: tuple = (0, 0, 0, 0)
    act: int = 0          # 0 none, 1 ReLU, 2 sigmoid
    res: int = 0          # 0 none, 1 residual, 2 half-size residual
    res_kblocked: bool = False
    out_mode: int = 0     # 0 NHWC, 1 2x2 scatter, 2 k-blocked
    rows: tuple = None    # (rows_per_group, (count per group, ...)) for the row-group form
    products: int = 0     # fp16 kernels: 1 or 3
    x16: bool = False
    y16: bool = False
    split: str = ""       # "a": weights n * 2^-q, "b": x n * 2^-q (the fp16 x 3 families)
    big_shift: bool = False   # fp16 outputs: shifts that put the values where fp16 rounds (ties, spacing 2)
    tile: tuple = (0, 0)  # conv_f16_pipelined's tile_rows, tile_cols
    mode: int = 0         # the mode / epilogue the case is meant to reach (0 aligned, 1 generic, 2 pointwise; 0..4)
    epi: int = 0

    @property
    def id(self):
        t = f"-t{self.tile[0]}x{self.tile[1]}" if self.tile != (0, 0) else ""
        p = f"-p{self.products}" if self.products else ""
        io = f"-{'h' if self.x16 else 's'}{'h' if self.y16 else 's'}" if self.op == "f16io" else ""
        return f"{self.family}-m{self.mode}e{self.epi}-{self.shape}{p}{io}{t}"

    @property
    def out_hw(self):
        pt, pl, pb, pr = self.pad
        return (self.h + pt + pb - self.k) // self.stride + 1, (self.w + pl + pr - self.k) // self.stride + 1

    @property
    def m(self):
        oh, ow = self.out_hw
        return self.b * oh * ow

    @property
    def kdim(self):
        return self.k * self.k * self.cin


def in_hw(oh, ow, k, stride, pad):
    """Input size that gives an oh x ow output."""
    pt, pl, pb, pr = pad
    return (oh - 1) * stride + k - pt - pb, (ow - 1) * stride + k - pl - pr


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def _seed(case):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(case.id)) % (2 ** 31)


def channel_scale(n):
    return np.array([0.5, 1.0, 2.0, 4.0])[np.arange(n) % 4]


def channel_shift(n, big=False):
    c = np.arange(n)
    small = ((c * 7) % 11 - 5).astype(np.float64)          # neighbours differ by 7 or -4
    return small + (1200.0 + 450.0 * (c % 4) if big else 0.0)


Data = dataclasses.make_dataclass("Data", ["x", "w", "scale", "shift", "residual", "pre", "want", "q", "absmax"])


@functools.lru_cache(maxsize=2)
def build(case):
    """The operands (float64 arrays holding the exact values, NHWC / OHWI), the float64 pre-activation `pre` (NHWC) and the
    expected output `want` in the output's own layout. `q`: the operands are multiples of 2^-q. `absmax`: the largest
    sum of |x||w| over the outputs."""
    rng = np.random.Generator(np.random.PCG64(_seed(case)))
    sig = case.act == 2
    xr, wr, q = (1, 1, 0) if sig else (4, 3, 0)
    if case.split:
        xr, wr, q = (1, 8191, Q_SPLIT) if case.split == "a" else (8191, 1, Q_SPLIT)
    x = rng.integers(-xr, xr + 1, (case.b, case.h, case.w, case.cin)).astype(np.float64)
    w = rng.integers(-wr, wr + 1, (case.cout, case.k, case.k, case.cin)).astype(np.float64)
    if case.split == "a":
        w /= 2.0 ** q
    elif case.split == "b":
        x /= 2.0 ** q
    oh, ow = case.out_hw
    scale = None if case.out_mode == 1 else channel_scale(case.cout)
    shift = channel_shift(case.cout, case.big_shift)
    residual = None
    if case.res:
        residual = rng.integers(-8, 9, (case.b, oh // case.res, ow // case.res, case.cout)).astype(np.float64)
    acc, absmax = _conv64(case, x, w)
    pre = acc * (1.0 if scale is None else scale) + shift
    if residual is not None:
        pre = pre + (residual if case.res == 1 else residual.repeat(2, axis=1).repeat(2, axis=2))
    y = np.maximum(pre, 0.0) if case.act == 1 else 1.0 / (1.0 + np.exp(-pre)) if sig else pre
    y = y + 0.0   # -0.0 -> +0.0, as max(0, v) and an exact sum to zero give in round-to-nearest
    return Data(x, w, scale, shift, residual, pre, to_layout(case, y), q, absmax)


def _conv64(case, x, w):
    """conv(x, w) and conv(|x|, |w|) in float64 (exact: every value is an integer times 2^-q far below 2^53)."""
    pt, pl, pb, pr = case.pad
    if case.k == 1 and case.stride == 1 and case.pad == (0, 0, 0, 0):
        xm, wm = x.reshape(-1, case.cin), w.reshape(case.cout, case.cin)
        return ((xm @ wm.T).reshape(case.b, case.h, case.w, case.cout),
                float((np.abs(xm) @ np.abs(wm).T).max()))
    xt = F.pad(torch.from_numpy(x).permute(0, 3, 1, 2), (pl, pr, pt, pb))
    wt = torch.from_numpy(w).permute(0, 3, 1, 2).contiguous()
    acc = F.conv2d(xt, wt, None, stride=case.stride).permute(0, 2, 3, 1).contiguous().numpy()
    absmax = float(F.conv2d(xt.abs(), wt.abs(), None, stride=case.stride).max())
    return acc, absmax


def to_layout(case, y):
    """NHWC [B,OH,OW,N] -> the output layout of the case: the same, the 2x2 scatter [B,2OH,2OW,N/4] with column
    n = (dy*2+dx)*C + co going to pixel (2*oy+dy, 2*ox+dx), or k-blocked [N/8,B,OH,OW,8]."""
    b, oh, ow, n = y.shape
    if case.out_mode == 1:
        c = n // 4
        return np.ascontiguousarray(y.reshape(b, oh, ow, 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(b, 2 * oh, 2 * ow, c))
    if case.out_mode == 2:
        return np.ascontiguousarray(y.reshape(b, oh, ow, n // 8, 8).transpose(3, 0, 1, 2, 4))
    return y


def kblocked(t):
    """NHWC [B,H,W,N] -> [N/8,B,H,W,8]."""
    b, h, w, n = t.shape
    return np.ascontiguousarray(t.reshape(b, h, w, n // 8, 8).transpose(3, 0, 1, 2, 4))


def int64_reference(case, d):
    """The same operation in int64, tap by tap, without torch: twice the pre-activation (scale 0.5 makes halves) for a case
    with integer operands. Independent of _conv64."""
    assert d.q == 0
    pt, pl, pb, pr = case.pad
    oh, ow = case.out_hw
    xp = np.zeros((case.b, case.h + pt + pb, case.w + pl + pr, case.cin), dtype=np.int64)
    xp[:, pt:pt + case.h, pl:pl + case.w] = d.x.astype(np.int64)
    wi = d.w.astype(np.int64)
    acc = np.zeros((case.b, oh, ow, case.cout), dtype=np.int64)
    s = case.stride
    for ky in range(case.k):
        for kx in range(case.k):
            patch = xp[:, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s]
            acc += np.einsum("byxc,nc->byxn", patch, wi[:, ky, kx])
    two_scale = np.full(case.cout, 2, np.int64) if d.scale is None else (2 * d.scale).astype(np.int64)
    pre2 = acc * two_scale + (2 * d.shift).astype(np.int64)
    if d.residual is not None:
        r = d.residual.astype(np.int64)
        pre2 += 2 * (r if case.res == 1 else r.repeat(2, axis=1).repeat(2, axis=2))
    return pre2


# ---------------------------------------------------------------------------------------------------------------------
# invariants (conditions on the inputs, asserted for every case)
# ---------------------------------------------------------------------------------------------------------------------
def f16_ties_and_unrepresentable(v):
    """How many values of the float64 array are exact round-to-even ties of fp16, and how many lie above 2048 and are not
    representable."""
    v = np.asarray(v, dtype=np.float64).ravel()
    with np.errstate(over="ignore"):
        r = v.astype(np.float16)
    rf = r.astype(np.float64)
    lo = np.where(rf <= v, rf, np.nextafter(r, np.float16(-np.inf)).astype(np.float64))
    hi = np.where(rf >= v, rf, np.nextafter(r, np.float16(np.inf)).astype(np.float64))
    ties = (lo != hi) & (v - lo == hi - v)
    return int(ties.sum()), int(((np.abs(v) > 2048) & (rf != v)).sum())


def check_invariants(case, d):
    """Raises AssertionError unless the data make bit equality a theorem (see the module docstring) and exercise the kernel."""
    g = 2.0 ** -(d.q + 1)                      # every operand, product, partial sum and result is a multiple of g
    assert d.absmax * 2.0 ** d.q < 2 ** 24, (case.id, "a partial sum may not be exact in fp32", d.absmax)
    bound = 4.0 * d.absmax + np.abs(d.shift).max() + (8.0 if case.res else 0.0)
    assert bound / g < 2 ** 24, (case.id, "the result may not be exact in fp32", bound)
    assert float(np.abs(d.pre).max()) <= bound
    for name, t in (("x", d.x), ("w", d.w), ("residual", d.residual)):
        if t is not None:
            assert np.count_nonzero(t) >= 0.3 * t.size, (case.id, name, "too many zeros")
        if t is not None and name != "residual":
            n = t * 2.0 ** d.q
            assert np.array_equal(n, np.round(n)), (case.id, name)
    if case.split:
        t = torch.from_numpy(d.w if case.split == "a" else d.x).float()
        hi = t.half()
        lo = t - hi.float()
        assert torch.equal(lo.half().float(), lo), (case.id, "hi + lo does not hold the operand exactly")
        assert int((lo != 0).sum()) * 3 >= lo.numel(), (case.id, "the lo plane is mostly zero")
        other = d.x if case.split == "a" else d.w      # the other operand has no lo plane: the dropped lo x lo term is zero
        assert np.array_equal(other.astype(np.float16).astype(np.float64), other), case.id
    elif case.op != "f32":
        for t in (d.x, d.w):
            assert np.array_equal(t.astype(np.float16).astype(np.float64), t), (case.id, "operand is not an fp16 value")
    if case.y16:
        assert float(np.abs(d.pre).max()) < 65504, case.id
        if d.residual is not None:
            assert np.array_equal(d.residual.astype(np.float16).astype(np.float64), d.residual)
    if case.act == 1:
        neg = float((d.pre < 0).mean())
        assert 0.2 <= neg <= 0.8, (case.id, f"{neg:.2f} of the outputs are negative before the ReLU")


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 table: one family per line of the dispatcher (run_conv_f32 -> conv_route_f32)
# ---------------------------------------------------------------------------------------------------------------------
RAGGED, RAGGED_EVEN, POW2 = (13, 11), (14, 10), (16, 16)


def _odd_map_for_tiles(lo, hi, bm=128, batch=3):
    """An odd, non-power-of-two map (oh, ow) whose batch * oh * ow rows make more than lo and fewer than hi M tiles of bm
    rows, the last one partial."""
    for oh in range(13, 400, 2):
        for ow in range(11, oh + 1, 2):
            m = batch * oh * ow
            if lo < -(-m // bm) < hi and m % bm:
                return oh, ow
    raise AssertionError((lo, hi))


def _f32_case(family, shape, mode, epi, cout, *, split=False, cin=None, tap=None, b=None, omap=None, act=None, **kw):
    """One fp32 case. mode / epi: what it is meant to reach; tap = (k, stride, pad) for the aligned / generic modes."""
    ragged = shape != "pow2"
    if tap is None:
        if mode == 2:
            tap = (1, 2 if (ragged and epi == 0) else 1, (0, 0, 0, 0))
        elif mode == 1:     # generic: the stem's 7x7 stride 2 pad 3 on ragged maps, 3x3 or 1x1 elsewhere
            tap = (1, 1, (0, 0, 0, 0)) if epi in (1, 4) else (7, 2, (3, 3, 3, 3)) if (ragged and epi != 2) else (3, 1, (1, 1, 1, 1))
        elif split:         # K >= 1024
            tap = (7, 1, (3, 3, 3, 3)) if ragged else (3, 1, (1, 1, 1, 1))
        else:
            tap = (3, 1, (1, 1, 1, 1)) if epi == 2 else (3, 2, (0, 0, 1, 1)) if ragged else (5, 1, (2, 2, 2, 2))
    k, stride, pad = tap
    if cin is None:
        if mode == 2:
            cin = (1056 if ragged else 1024) if split else (64 if ragged else 32)
        elif mode == 1:
            cin = 20 if k == 1 else 4 if k == 7 else 12
        else:
            cin = (32 if k == 7 else 128) if split else 32
    if omap is None:
        omap = (RAGGED_EVEN if epi == 2 else RAGGED) if ragged else POW2
    h, w = in_hw(*omap, k, stride, pad)
    if act is None:
        act = 2 if epi == 3 else int(ragged) if epi in (0, 1, 4) else int(not ragged)
    res = epi if epi in (1, 2) else 0
    return Case(family, shape, "f32", b or (3 if ragged else 2), h, w, cin, cout, k, stride, pad, act, res,
                res_kblocked=bool(res and not ragged and cout % 8 == 0), out_mode=kw.pop("out_mode", 1 if epi == 4 else 0),
                mode=mode, epi=epi, **kw)


def _family(family, couts, scatter_couts, modes, epis, **kw):
    """Two shapes (ragged, batch 3; power of two, batch 2) for every (mode, epilogue) of a family. The 2x2 scatter comes
    from deconv2x2 only: a 1x1 unpadded GEMM, so never the aligned-tap mode."""
    out = []
    for mode in modes:
        for epi in epis:
            if epi == 4 and mode == 0:
                continue
            for shape, cout in zip(("ragged", "pow2"), scatter_couts if epi == 4 else couts):
                out.append(_f32_case(family, shape, mode, epi, cout, **kw))
    return out


def fp32_cases(cus=256):
    """The fp32 table for a device with `cus` compute units (the families that depend on `underfilled` size themselves)."""
    assert cus >= 64, "the small underfilled cases assume a device with at least 64 CUs"
    c = []
    # Cout <= 32: the 128x32 tile, any mode
    c += _family("t128x32", (31, 32), (28, 32), (0, 1, 2), (0, 1, 2, 3, 4))
    c += _family("t128x32_split", (31, 32), None, (0, 2), (0, 1, 2), split=True)
    # 32 < Cout <= 64: 256x64, BK 32 for generic K, BK 16 otherwise
    c += _family("t256x64_k32", (33, 64), (36, 64), (1,), (0, 1, 2, 3, 4))
    c += _family("t256x64_k16", (33, 64), (36, 64), (0, 2), (0, 1, 2, 3, 4))
    # 64 < Cout <= 96, Cin % 32 == 0: 128x96
    c += _family("t128x96", (65, 96), (68, 96), (0, 2), (0, 1, 2, 3, 4))
    # K <= 128 with Cout >= 256 (as aligned taps: a padded 1x1), or the scatter with K <= 256 and Cout >= 256: 128x128 BK 16
    c += _family("t128x128_k16", (257, 256), (260, 256), (0,), (0, 1, 2, 3), tap=(1, 1, (1, 1, 1, 1)), cin=64)
    c += _family("t128x128_k16", (257, 256), (260, 256), (2,), (0, 1, 2, 3, 4))
    # underfilled (Cout >= 128, fewer 128x128 tiles than CUs), K < 1024: 128x64; also K <= 256 + residual + Cout >= 128
    c += _family("t128x64", (129, 256), (132, 136), (0,), (0, 1, 2, 3))
    c += [_f32_case("t128x64", s, 2, e, n, cin=ci) for e in (0, 1, 2, 3) for s, n, ci in (("ragged", 129, 64), ("pow2", 256, 160))]
    c += [_f32_case("t128x64", s, 2, 4, n, cin=64) for s, n in (("ragged", 132), ("pow2", 136))]
    # underfilled with K >= 1024 and at most `cus` 128x64 tiles: 128x32 with the two-chain sum
    # (the same routes as Cout <= 32 with K >= 1024: one family, further shapes)
    c += [dataclasses.replace(_f32_case("t128x32_split", s, m, e, n, split=True, tap=(3, 1, (1, 1, 1, 1)) if m == 0 else None,
                                        cin=128 if m == 0 else None), shape="underfilled_" + s)
          for m, e in ((2, 0), (0, 1), (2, 2)) for s, n in (("ragged", 129), ("pow2", 256))]
    # underfilled with K >= 1024 and more than `cus` 128x64 tiles: 128x64 with the two-chain sum. 129 columns: two 128-wide
    # tiles, three 64-wide ones, so cus/3 < M tiles < cus/2
    mt = cus // 3 + 2
    mt += mt % 2
    assert 2 * mt < cus < 3 * (mt - 1)
    for m in (0, 2):
        for e in (0, 1, 2):
            omap = _odd_map_for_tiles(mt - 2, mt + 1) if e != 2 else None
            if e == 2:   # even sides, not powers of two
                omap = next((oh, ow) for oh in range(14, 400, 4) for ow in range(10, oh, 4)
                            if mt - 2 < -(-3 * oh * ow // 128) < mt + 1 and (3 * oh * ow) % 128)
            extra = dict(tap=(3, 1, (1, 1, 1, 1)), cin=128) if m == 0 else {}
            c.append(_f32_case("t128x64_split", "ragged", m, e, 129, split=True, omap=omap, **extra))
            c.append(_f32_case("t128x64_split", "pow2", m, e, 129 if e == 0 else 136, split=True, b=mt // 2, **extra))
    # everything else: 128x128 BK 32 — generic K with Cout > 64, or 96 < Cout < 128 (never underfilled)
    c += _family("t128x128_k32", (97, 104), (100, 104), (0, 1, 2), (0, 1, 2, 3, 4))
    c += _family("t128x128_k32_split", (97, 104), None, (0, 2), (0, 1, 2), split=True)
    # ... and Cout = 512 with at least `cus` 128x128 tiles (not underfilled)
    fill = -(-cus // 4)
    c.append(dataclasses.replace(_f32_case("t128x128_k32", "ragged", 0, 0, 513, omap=_odd_map_for_tiles(fill - 1, fill + 4),
                                           tap=(3, 1, (1, 1, 1, 1))), shape="filled_ragged"))
    c.append(dataclasses.replace(_f32_case("t128x128_k32", "pow2", 2, 0, 512, cin=160, b=-(-fill // 2)), shape="filled_pow2"))
    # the streaming 1x1 kernel: M >= 131072 rows, stride 1, no residual, no sigmoid, no scatter
    for fam, cin, (n_odd, n_even) in (("stream_256_64", 256, (33, 64)), ("stream_64_64", 64, (33, 64)), ("stream_64_256", 64, (129, 256))):
        c.append(_f32_case(fam, "ragged", 2, 0, n_odd, cin=cin, omap=(319, 137), tap=(1, 1, (0, 0, 0, 0)), act=1))   # 131072 + 37 rows
        c.append(_f32_case(fam, "pow2", 2, 0, n_even, cin=cin, omap=(256, 256), tap=(1, 1, (0, 0, 0, 0)), act=0, out_mode=2))
    # the k-blocked output on a ragged map
    c.append(dataclasses.replace(_f32_case("t256x64_k16", "ragged_kblocked", 0, 1, 40), out_mode=2))
    c.append(dataclasses.replace(_f32_case("t128x128_k32", "ragged_kblocked", 2, 0, 104), out_mode=2))
    # row groups: empty, partial and full groups of 100 slots; 128-row tiles (81 columns) and 256-row tiles (64 columns)
    counts = (0, 0, 0, 37, 100, 0, 100, 5, 0, 0, 0, 100, 1)
    for fam, cin, cout in (("t128x96", 64, 81), ("t256x64_k16", 32, 64), ("t128x128_k32_split", 1024, 97)):
        c.append(Case(fam, "rows", "f32", len(counts) * 100, 1, 1, cin, cout, act=1, rows=(100, counts), mode=2, epi=0))
    ids = [k.id for k in c]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return c


def route_of(case, cus, ops):
    """The dispatcher's route for an fp32 case."""
    return ops.conv_route(case.b, case.h, case.w, case.cin, case.cout, case.k, case.k, case.stride, case.pad, bool(case.res),
                          max(case.res, 1), case.act, case.out_mode, case.rows is not None, cus)


# ---------------------------------------------------------------------------------------------------------------------
# the fp16 tables (conv_f16.hip's dispatch depends on the arguments only: tile by Cout <= 64, generic by Cin % 32, the
# epilogue, `products`, and the in / out types)
# ---------------------------------------------------------------------------------------------------------------------
def _f16_case(family, shape, op, generic, epi, cout, **kw):
    ragged = shape == "ragged"
    if epi == 4:
        k, stride, pad = 1, 1, (0, 0, 0, 0)
    elif ragged and epi != 2:
        k, stride, pad = 3, 2, (0, 0, 1, 1)
    else:
        k, stride, pad = 3, 1, (1, 1, 1, 1)
    cin = (24 if k == 1 else 8) if generic else 32
    omap = (RAGGED_EVEN if epi == 2 else RAGGED) if ragged else POW2
    h, w = in_hw(*omap, k, stride, pad)
    act = 2 if epi == 3 else int(ragged) if epi in (0, 1, 4) else int(not ragged)
    if kw.get("big_shift"):
        act = 0
    return Case(family, shape, op, 3 if ragged else 2, h, w, cin, cout, k, stride, pad, act, epi if epi in (1, 2) else 0,
                out_mode=1 if epi == 4 else 0, mode=int(generic), epi=epi, **kw)


def f16mfma_cases():
    """conv_bn_act_f16mfma / deconv2x2 with fp32 activations: products 1 (integer data) and 3 (family a on the ragged
    shape, b on the power-of-two one), both tiles, generic and aligned, epilogues 0-4."""
    c = []
    for products in (1, 3):
        for tile, couts, scatter in (("t256x64", (33, 64), (36, 64)), ("t128x128", (129, 136), (132, 136))):
            for generic in (False, True):
                for epi in range(5):
                    for shape, cout in zip(("ragged", "pow2"), scatter if epi == 4 else couts):
                        split = "" if products == 1 else "a" if shape == "ragged" else "b"
                        c.append(_f16_case(f"f16mfma_{tile}", shape, "f16mfma", generic, epi, cout, products=products, split=split))
    return c


def f16io_cases():
    """The io16 forms launch16 instantiates: fp32 -> fp16 (epilogue 0, generic and aligned), fp16 -> fp16 (0, 1, 2, 4),
    fp16 -> fp32 (0, 3); an fp16 output needs an even Cout. The power-of-two shapes without a ReLU carry the big shifts."""
    c = []
    for tile, couts, scatter in (("t256x64", (34, 64), (40, 64)), ("t128x128", (130, 136), (136, 144))):
        forms = [(False, True, g, 0) for g in (False, True)] + [(True, True, False, e) for e in (0, 1, 2, 4)] + \
                [(True, False, False, e) for e in (0, 3)]
        for x16, y16, generic, epi in forms:
            for shape, cout in zip(("ragged", "pow2"), scatter if epi == 4 else couts):
                big = y16 and (shape == "pow2" or epi == 2)
                c.append(_f16_case(f"f16io_{tile}", shape, "f16io", generic, epi, cout, products=1, x16=x16, y16=y16, big_shift=big))
    return c


F16P_TILES = ((128, 256), (160, 256), (192, 256), (256, 256), (128, 128), (256, 128), (128, 64), (256, 64))


def f16p_cases():
    """conv_f16_pipelined on every tile shape: a ragged 3x3 (batch 3, 13 x 11) and a 1x1 with an fp16 residual."""
    c = []
    for tile in F16P_TILES:
        c.append(Case("f16p", "ragged", "f16p", 3, 13, 11, 64, 256, 3, 1, (1, 1, 1, 1), 1, 0, products=1, x16=True, y16=True,
                      tile=tile, mode=0, epi=0))
        c.append(Case("f16p", "pow2", "f16p", 2, 16, 16, 128, 256, 1, 1, (0, 0, 0, 0), 0, 1, products=1, x16=True, y16=True,
                      big_shift=True, tile=tile, mode=2, epi=1))
    return c
