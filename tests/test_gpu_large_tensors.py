"""GPU tests (-m gpu) at the top of the kernels' 32-bit byte-offset range: tensors between 2^31 and 2^32 bytes.

Every kernel addresses memory through buffer descriptors with 32-bit byte offsets, and drops out-of-tile loads and stores
by sending them to the offset OOB = 0xFFFFFFF0 (csrc/conv_common.hpp). These cases call each kernel once at a shape whose
largest tensor lies in the upper half of that range, with ragged tiles in M and N, and check

  (a) sampled output rows (the last M tile, the rows whose output bytes or input receptive fields cross 2^31 bytes, the first
      tile, ~1000 seeded random rows) against a float64 reference, element by element, within the forward-error bound of
      the sum: |got - ref| <= (K + 2) 2^-24 sum|x w| |scale| + 2^-23 |shift|;
  (b) bit identity with the last image run alone, where batch independence is documented;
  (c) guard bands: the output is written through the C ABI into the middle of a larger allocation whose sentinel bytes on
      both sides must be unchanged.

Inputs are generated on the device; only the patches the sampled rows read are copied to the host. Each case frees its
tensors before the next and stays under ~16 GB of device memory.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

OOB = 0xFFFFFFF0
GIB2 = 1 << 31
BAND = 4096  # guard band, elements on each side


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import maskrcnn_amd  # noqa: F401
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _free_between_cases():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _randn(shape, seed, dev, std=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    t = torch.empty(shape, dtype=torch.float32, device=dev)
    t.normal_(0.0, std, generator=g)
    return t


def _scale(n, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.rand(n, generator=g, device=dev) + 0.5


def _guarded(n, dev, fill=7.0):
    buf = torch.full((n + 2 * BAND,), fill, dtype=torch.float32, device=dev)
    return buf, buf[BAND:BAND + n]


def _bands_intact(buf, n, fill=7.0):
    return bool((buf[:BAND] == fill).all()) and bool((buf[BAND + n:] == fill).all())


def _sample_rows(m, tile_m, cross_rows, seed, count=1000):
    """The first tile, the last (ragged) tile, the given crossing rows and `count` seeded random rows, as a sorted long tensor."""
    last0 = ((m - 1) // tile_m) * tile_m
    g = torch.Generator().manual_seed(seed)
    rows = [torch.arange(0, min(tile_m, m)), torch.arange(last0, m), torch.randint(0, m, (count,), generator=g),
            torch.tensor([r for r in cross_rows if 0 <= r < m], dtype=torch.long)]
    return torch.unique(torch.cat(rows))


def _patches(x, rows, kh, kw, stride, pt, pl, oh, ow):
    """im2col rows of x [B,H,W,C] (device) for output pixels `rows`: [S, kh*kw*C] float64 on the host, padding taps zero."""
    b_, h, w, c = x.shape
    r = rows.to(x.device)
    b, rem = r // (oh * ow), r % (oh * ow)
    oy, ox = rem // ow, rem % ow
    ky = torch.arange(kh, device=x.device).view(1, kh, 1)
    kx = torch.arange(kw, device=x.device).view(1, 1, kw)
    iy = (oy * stride - pt).view(-1, 1, 1) + ky
    ix = (ox * stride - pl).view(-1, 1, 1) + kx
    iy, ix = iy.expand(-1, kh, kw), ix.expand(-1, kh, kw)
    ok = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
    p = x[b.view(-1, 1, 1).expand(-1, kh, kw), iy.clamp(0, h - 1), ix.clamp(0, w - 1)]  # [S, kh, kw, C]
    p = p * ok.unsqueeze(-1)
    return p.reshape(len(rows), -1).double().cpu()


def _check_rows(got, patches, w2d, scale, shift, relu, what, res=None):
    """(a): got [S, N] fp32 against the float64 reference of the sampled rows, per element within the forward-error bound;
    res [S, N]: the residual added after the affine."""
    w64 = w2d.double()
    ref = patches @ w64.t()
    absprod = patches.abs() @ w64.abs().t()
    k = w2d.size(1)
    sc = scale.double() if scale is not None else torch.ones(w2d.size(0), dtype=torch.float64)
    sh = shift.double() if shift is not None else torch.zeros(w2d.size(0), dtype=torch.float64)
    ref = ref * sc + sh
    bound = (k + 2) * 2.0 ** -24 * absprod * sc.abs() + 2.0 ** -23 * sh.abs() + 1e-30
    if res is not None:
        ref = ref + res.double()
        bound = bound + 2.0 ** -23 * res.double().abs()
    if relu:
        ref = ref.clamp_min(0)
    err = (got.double() - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), (
        f"{what}: {int(bad.sum())} of {bad.numel()} sampled elements outside the error bound; first at (row {int(bad.nonzero()[0, 0])}, "
        f"col {int(bad.nonzero()[0, 1])}), max err/bound {float((err / bound).max()):.3g}")


def _conv_c_abi(x, w, scale, shift, stride, pad, relu, y, residual=None, res_div=1, y_kblocked=False):
    from maskrcnn_amd._lib import check, lib
    b, h, wd, cin = x.shape
    cout, kh, kw, _ = w.shape
    pt, pl, pb, pr = pad
    check(lib.mrcnn_conv_bn_act_f32(x.data_ptr(), b, h, wd, cin, w.data_ptr(), cout, kh, kw, stride, pt, pl, pb, pr,
                                    scale.data_ptr() if scale is not None else None,
                                    shift.data_ptr() if shift is not None else None,
                                    residual.data_ptr() if residual is not None else None, res_div, 0, 1 if relu else 0,
                                    y.data_ptr(), 1 if y_kblocked else 0, torch.cuda.current_stream().cuda_stream))


# ---------------------------------------------------------------------------------------------------------------------
# the direct fp32 conv (conv.hip)
# ---------------------------------------------------------------------------------------------------------------------
def test_direct_conv_refuses_the_sentinel_window(dev):
    """1x1 conv, 466 x 1103 pixels, Cin 32 -> Cout 2089: M * Cout = 2^30 - 2, an fp32 output of 0xFFFFFFF8 bytes. The dropped
    stores of its ragged tiles (rows 78..127 of the last M tile, columns 2089..2175) go to offset OOB, which would be
    element 2^30 - 4 = y[M-1, 2087] of it: the call is refused with real allocations and writes nothing."""
    from maskrcnn_amd._lib import MaskrcnnHipError
    b, h, w, cin, cout = 1, 466, 1103, 32, 2089
    n = b * h * w * cout
    assert n == (1 << 30) - 2 and 4 * n > OOB
    x = _randn((b, h, w, cin), 11, dev)
    wt = _randn((cout, 1, 1, cin), 12, dev, 0.2)
    buf, y = _guarded(n, dev)
    with pytest.raises(MaskrcnnHipError, match="too large"):
        _conv_c_abi(x, wt, None, None, 1, (0, 0, 0, 0), False, y)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    del buf, y


# (B, H, W, Cin, Cout): the sentinel window's largest accepted neighbour (exactly OOB bytes of output, ragged M: 60 rows of
# the last tile, ragged N: 113 of 128 columns) and a wide ragged-N output (4095 columns, M % 128 = 124) of 0xFFF00000 bytes
@pytest.mark.parametrize("shape", [(4, 113, 1247, 32, 1905), (4, 255, 257, 64, 4095)], ids=lambda s: "x".join(map(str, s)))
def test_direct_conv_1x1_output_at_the_top_of_the_range(dev, shape):
    from maskrcnn_amd import ops
    b, h, w, cin, cout = shape
    m = b * h * w
    n = m * cout
    assert GIB2 <= 4 * n <= OOB and m % 128 and cout % 128, (4 * n, m % 128, cout % 128)
    x = _randn((b, h, w, cin), 21 + cout, dev)
    wt = _randn((cout, 1, 1, cin), 22 + cout, dev, 1.0 / math.sqrt(cin))
    scale = _scale(cout, 24, dev)
    shift = _randn((cout,), 23, dev, 0.1)
    buf, y = _guarded(n, dev)
    _conv_c_abi(x, wt, scale, shift, 1, (0, 0, 0, 0), False, y)
    torch.cuda.synchronize()
    # (c) guard bands
    assert _bands_intact(buf, n), shape
    y2 = y.view(m, cout)
    # (a) sampled rows, the rows whose output bytes cross 2^31 included
    cross = GIB2 // (4 * cout)
    rows = _sample_rows(m, 128, range(cross - 2, cross + 3), seed=cout)
    got = y2[rows.to(dev)].cpu()
    _check_rows(got, _patches(x, rows, 1, 1, 1, 0, 0, h, w), wt.view(cout, cin).cpu(), scale.cpu(), shift.cpu(), False,
                f"conv1x1 {shape}")
    # (b) K < 1024: the last image alone, bit for bit
    alone = ops.conv_bn_act(x[b - 1:].contiguous(), wt, scale, shift)
    torch.cuda.synchronize()
    assert torch.equal(alone.view(-1, cout), y2[(b - 1) * h * w:]), shape
    del buf, y, y2, x, alone


# The direct conv's other epilogues, each with an output past 2^31 bytes (1x1, K = 64 < 1024, so batch independence holds):
#   res1     residual of the output's size (Cout even: the 8-byte pair epilogue), residual and output 2.15 GB each
#   res2     residual at half size (FPN nearest-upsample-add), output 2.15 GB
#   kblocked k-blocked output [Cout/8][M][8], 2.16 GB
#   deconv   2x2 stride-2 transposed-conv scatter, GEMM N = 4 x 520 (ragged), output [B, 2H, 2W, 520] of 2.18 GB
@pytest.mark.parametrize("kind", ["res1", "res2", "kblocked", "deconv"])
def test_direct_conv_epilogues_at_the_top_of_the_range(dev, kind):
    from maskrcnn_amd._lib import check, lib
    b, cin = 4, 64
    h, w = (254, 258) if kind == "res2" else (255, 257)
    cout = {"res1": 2050, "res2": 2050, "kblocked": 2056, "deconv": 4 * 520}[kind]   # GEMM columns
    m = b * h * w
    n = m * cout
    assert GIB2 <= 4 * n <= OOB and m % 128 and cout % 128, (kind, 4 * n)
    x = _randn((b, h, w, cin), 71, dev)
    wt = _randn((cout, 1, 1, cin), 72, dev, 1.0 / math.sqrt(cin))
    scale = None if kind == "deconv" else _scale(cout, 73, dev)
    shift = _randn((cout // 4,), 74, dev, 0.1).repeat(4) if kind == "deconv" else _randn((cout,), 74, dev, 0.1)
    res = None
    if kind == "res1":
        res = _randn((b, h, w, cout), 75, dev)
    elif kind == "res2":
        res = _randn((b, h // 2, w // 2, cout), 75, dev)
    stream = torch.cuda.current_stream().cuda_stream

    def run(xx, yy, rr):
        if kind == "deconv":
            check(lib.mrcnn_deconv2x2_bias_act_nhwc_f32(xx.data_ptr(), xx.size(0), h, w, cin, wt.data_ptr(), cout // 4,
                                                        shift.data_ptr(), 0, yy.data_ptr(), stream))
        else:
            _conv_c_abi(xx, wt, scale, shift, 1, (0, 0, 0, 0), False, yy, residual=rr, res_div=2 if kind == "res2" else 1,
                        y_kblocked=kind == "kblocked")

    buf, y = _guarded(n, dev)
    run(x, y, res)
    torch.cuda.synchronize()
    assert _bands_intact(buf, n), kind

    def gemm_rows(yy, mm, rows):  # output elements of GEMM rows `rows` (input pixels), [S, cout] in GEMM column order
        if kind == "kblocked":
            return yy.view(cout // 8, mm, 8)[:, rows].permute(1, 0, 2).reshape(len(rows), cout)
        if kind == "deconv":
            bb, rem = rows // (h * w), rows % (h * w)
            i, j = rem // w, rem % w
            y4 = yy.view(-1, 2 * h, 2 * w, cout // 4)
            return torch.cat([y4[bb, 2 * i + (q >> 1), 2 * j + (q & 1)] for q in range(4)], 1)
        return yy.view(mm, cout)[rows]

    cross = GIB2 // (4 * cout)
    rows = _sample_rows(m, 128, range(cross - 2, cross + 3), seed=76)
    rd = rows.to(dev)
    got = gemm_rows(y, m, rd).cpu()
    r_rows = None
    if kind == "res1":
        r_rows = res.view(m, cout)[rd].cpu()
    elif kind == "res2":
        bb, rem = rd // (h * w), rd % (h * w)
        r_rows = res[bb, (rem // w) // 2, (rem % w) // 2].cpu()
    _check_rows(got, _patches(x, rows, 1, 1, 1, 0, 0, h, w), wt.view(cout, cin).cpu(),
                None if scale is None else scale.cpu(), shift.cpu(), False, kind, res=r_rows)
    # (b) the last image alone, bit for bit
    ma = h * w
    ya = torch.empty(ma * cout, dtype=torch.float32, device=dev)
    run(x[b - 1:].contiguous(), ya, None if res is None else res[b - 1:].contiguous())
    torch.cuda.synchronize()
    last = torch.arange((b - 1) * ma, m, device=dev)
    assert torch.equal(gemm_rows(ya, ma, torch.arange(ma, device=dev)), gemm_rows(y, m, last)), kind
    del buf, y, ya, x, res


# 3x3 convs on a 3.5 GiB input (B1, 2048^2, Cin 224 -> 64): SAME stride 1 (pad 1), and stride 2 with the (0, 0, 1, 1) SAME
# padding of the trunk's stride-2 layers
@pytest.mark.parametrize("stride,pad", [(1, (1, 1, 1, 1)), (2, (0, 0, 1, 1))], ids=["s1", "s2"])
def test_direct_conv_3x3_input_at_the_top_of_the_range(dev, stride, pad):
    b, h, w, cin, cout = 1, 2048, 2048, 224, 64
    assert GIB2 <= 4 * b * h * w * cin <= OOB
    pt, pl, pb, pr = pad
    oh, ow = (h + pt + pb - 3) // stride + 1, (w + pl + pr - 3) // stride + 1
    m = b * oh * ow
    x = _randn((b, h, w, cin), 31, dev)
    wt = _randn((cout, 3, 3, cin), 32 + stride, dev, 1.0 / math.sqrt(9 * cin))
    scale = _scale(cout, 34, dev)
    shift = _randn((cout,), 33, dev, 0.1)
    buf, y = _guarded(m * cout, dev)
    _conv_c_abi(x, wt, scale, shift, stride, pad, True, y)
    torch.cuda.synchronize()
    assert _bands_intact(buf, m * cout), stride
    # the output pixels whose receptive field holds the input pixel at byte 2^31
    px = GIB2 // (4 * cin)
    iy, ix = px // w, px % w
    cross = [oy * ow + ox for oy in range(oh) if 0 <= iy - (oy * stride - pt) < 3
             for ox in range(ow) if -1 <= ix - (ox * stride - pl) < 4]
    assert len(cross) >= 6
    rows = _sample_rows(m, 256, cross, seed=40 + stride)
    got = buf[BAND:BAND + m * cout].view(m, cout)[rows.to(dev)].cpu()
    del buf, y
    _check_rows(got, _patches(x, rows, 3, 3, stride, pt, pl, oh, ow), wt.view(cout, -1).cpu(), scale.cpu(), shift.cpu(), True,
                f"conv3x3 s{stride}")
    del x


# ---------------------------------------------------------------------------------------------------------------------
# Winograd F(4x4) (conv_wino4.hip) and the NHWC -> k-blocked transpose it reads
# ---------------------------------------------------------------------------------------------------------------------
def test_winograd4_at_the_top_of_the_range(dev):
    """F(4x4) on B8 x 256^2, Cin 1024 -> Cout 960: a 2 GiB k-blocked input and a 1.9 GiB output, unit-scale data. (a) sampled
    pixels against float64 within the 1e-4 absolute bar of the full-size tests, per element; (b) the last image alone,
    bit for bit; (c) guard bands around the NHWC output, written through the C ABI."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import check, lib
    b, h, w, cin, cout = 8, 256, 256, 1024, 960
    m = b * h * w
    assert 4 * m * cin >= GIB2 and 4 * m * cin <= OOB and ops.conv3x3_winograd4_supported(h, w, cin, cout, b)
    x = _randn((b, h, w, cin), 51, dev)
    wt = _randn((cout, 3, 3, cin), 52, dev, math.sqrt(2.0 / (9 * cin)))
    scale = _scale(cout, 54, dev)
    shift = _randn((cout,), 53, dev, 0.1)
    u4 = ops.winograd4_weights(wt)
    xk = ops.nhwc_to_kblocked(x)
    buf, y = _guarded(m * cout, dev)
    check(lib.mrcnn_conv3x3_winograd4_f32(xk.data_ptr(), b, h, w, cin, u4.data_ptr(), cout, scale.data_ptr(), shift.data_ptr(),
                                          0, y.data_ptr(), None, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _bands_intact(buf, m * cout)
    del xk
    y2 = y.view(m, cout)
    alone = ops.conv3x3_winograd4(ops.nhwc_to_kblocked(x[b - 1:].contiguous()), u4, scale, shift)
    torch.cuda.synchronize()
    assert torch.equal(alone.view(-1, cout), y2[(b - 1) * h * w:])
    del alone
    rows = _sample_rows(m, 256, [m - 1, m - w, m - w - 1], seed=54, count=600)
    got = y2[rows.to(dev)].cpu()
    del buf, y, y2
    p = _patches(x, rows, 3, 3, 1, 1, 1, h, w)
    ref = (p @ wt.view(cout, -1).cpu().double().t()) * scale.cpu().double() + shift.cpu().double()
    err = (got.double() - ref).abs()
    assert float(err.max()) <= 1e-4, f"max|err| {float(err.max()):.3e} > 1e-4 abs (max|ref| {float(ref.abs().max()):.2f})"
    del x


def test_winograd4_refuses_the_first_shape_past_its_limit(dev):
    """B16 x 256^2 x 1024 is a 4 GiB input (> OOB): refused by the predicate and by the launch, and nothing is written."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import MaskrcnnHipError, check, lib
    b, h, w, cin, cout = 16, 256, 256, 1024, 64
    assert 4 * b * h * w * cin > OOB and not ops.conv3x3_winograd4_supported(h, w, cin, cout, b)
    assert ops.conv3x3_winograd4_supported(h, w, cin, cout, b - 1)
    xk = torch.zeros(b * h * w * cin, dtype=torch.float32, device=dev)
    u4 = torch.zeros(cin // 4 * 36 * 2 * cout * 2, dtype=torch.float32, device=dev)
    buf, y = _guarded(b * h * w * cout, dev)
    with pytest.raises(MaskrcnnHipError, match="too large|required"):
        check(lib.mrcnn_conv3x3_winograd4_f32(xk.data_ptr(), b, h, w, cin, u4.data_ptr(), cout, None, None, 0, y.data_ptr(),
                                              None, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    del xk, u4, buf, y


def test_nhwc_to_kblocked_past_2_to_the_30_elements(dev):
    """The NHWC -> k-blocked transpose at 2^31 - 256 elements (8 GiB each way), its largest accepted size: sampled pixels,
    the last ones included, are moved exactly; 2^31 elements are refused."""
    from maskrcnn_amd._lib import MaskrcnnHipError, check, lib
    c = 256
    pixels = (1 << 31) // c - 1
    x = _randn((pixels, c), 61, dev)
    y = torch.empty(c // 8, pixels, 8, dtype=torch.float32, device=dev)
    assert x.numel() < 1 << 31 <= x.numel() + c
    check(lib.mrcnn_nhwc_to_kblocked_f32(x.data_ptr(), pixels, c, y.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(62)
    rows = torch.unique(torch.cat([torch.randint(0, pixels, (4096,), generator=g), torch.arange(pixels - 64, pixels),
                                   torch.arange(0, 64)])).to(dev)
    want = x[rows].view(-1, c // 8, 8).permute(1, 0, 2)
    assert torch.equal(y[:, rows], want)
    del x, y
    # the refused call gets allocations of the size it names
    x1 = torch.zeros((pixels + 1) * c, dtype=torch.float32, device=dev)
    buf, y1 = _guarded((pixels + 1) * c, dev)
    with pytest.raises(MaskrcnnHipError):
        check(lib.mrcnn_nhwc_to_kblocked_f32(x1.data_ptr(), pixels + 1, c, y1.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    del x1, buf, y1
