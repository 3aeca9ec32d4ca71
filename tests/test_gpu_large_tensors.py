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
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from crop_staged_cases import _crop_footprint_slots  # noqa: E402  the staged crop kernel's footprint, restated

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


# ---------------------------------------------------------------------------------------------------------------------
# the other kernel families at the top of their range (tests/test_boundary.py checks each one refuses the next shape up)
# ---------------------------------------------------------------------------------------------------------------------
def _guarded_t(n, dev, dtype, fill=7.0):
    buf = torch.full((n + 2 * BAND,), fill, dtype=dtype, device=dev)
    return buf, buf[BAND:BAND + n]


def _f4_rows_bound(p64, w2d, scale, shift, relu=True):
    """float64 reference of relu?(patches @ w^T * scale + shift) for an F(4x4) layer, with its 1e-4 absolute bar."""
    t = (p64 @ w2d.double().t()) * scale.double() + shift.double()
    return t.clamp_min(0) if relu else t


def test_winograd4_conv3_at_the_top_of_the_range(dev):
    """F(4x4) conv2 + the 1x1 conv3 + residual of a Bottleneck in one launch (mrcnn_conv3x3_winograd4_conv3_f32) on B16 x 512 x 508,
    Cin 64 -> 64 -> c3 256: output and residual 3.97 GiB each (4 px c3 <= OOB, 0.99 of it), W ragged in the 32-pixel tiles. (a) sampled pixels, those whose
    output bytes cross 2^31 included, against float64 (the 64-channel intermediate within F(4x4)'s 1e-4 absolute bar, carried
    through conv3's weights, plus the fp32 sum bound); (b) the last image alone and the per-layer launches on it, bit for bit;
    (c) guard bands."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import check, lib
    b, h, w, cin, c3 = 16, 512, 508, 64, 256
    m = b * h * w
    assert 0.95 * OOB <= 4 * m * c3 <= OOB and w % 32 and ops.conv3x3_winograd4_supported(h, w, cin, 64, b)   # ragged 16 x 32 tiles
    x = _randn((b, h, w, cin), 81, dev)
    w2 = _randn((64, 3, 3, cin), 82, dev, math.sqrt(2.0 / (9 * cin)))
    s2, t2 = _scale(64, 83, dev), _randn((64,), 84, dev, 0.1)
    w3 = _randn((c3, 1, 1, 64), 85, dev, 1.0 / 8)
    s3, t3 = _scale(c3, 86, dev), _randn((c3,), 87, dev, 0.1)
    res = _randn((b, h, w, c3), 88, dev)
    u4 = ops.winograd4_weights(w2)
    xk = ops.nhwc_to_kblocked(x)
    buf, y = _guarded(m * c3, dev)
    check(lib.mrcnn_conv3x3_winograd4_conv3_f32(xk.data_ptr(), b, h, w, cin, u4.data_ptr(), s2.data_ptr(), t2.data_ptr(),
                                                w3.data_ptr(), c3, s3.data_ptr(), t3.data_ptr(), res.data_ptr(), y.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _bands_intact(buf, m * c3)
    del xk
    y2 = y.view(m, c3)
    # (b) the last image alone, and the per-layer launches (F(4x4), then the direct 1x1 with the residual) on it
    xl, rl = x[b - 1:].contiguous(), res[b - 1:].contiguous()
    alone = ops.conv3x3_winograd4_conv3(ops.nhwc_to_kblocked(xl), u4, s2, t2, w3, s3, t3, rl)
    mid = ops.conv3x3_winograd4(ops.nhwc_to_kblocked(xl), u4, s2, t2, True)
    layers = ops.conv_bn_act(mid, w3, s3, t3, 1, (0, 0, 0, 0), True, rl)
    torch.cuda.synchronize()
    assert torch.equal(alone.view(-1, c3), y2[(b - 1) * h * w:])
    assert torch.equal(layers, alone)
    del alone, mid, layers, xl, rl
    # (a)
    cross = GIB2 // (4 * c3)
    rows = _sample_rows(m, 256, range(cross - 2, cross + 3), seed=89, count=600)
    rd = rows.to(dev)
    got = y2[rd].cpu().double()
    r64 = res.view(m, c3)[rd].cpu().double()
    del buf, y, y2, res
    t = _f4_rows_bound(_patches(x, rows, 3, 3, 1, 1, 1, h, w), w2.view(64, -1).cpu(), s2.cpu(), t2.cpu())
    w3d, s3d, t3d = w3.view(c3, 64).cpu().double(), s3.cpu().double(), t3.cpu().double()
    ref = ((t @ w3d.t()) * s3d + t3d + r64).clamp_min(0)
    bound = (1e-4 * w3d.abs().sum(1) + 66 * 2.0 ** -24 * (t.abs() @ w3d.abs().t())) * s3d \
        + 2.0 ** -23 * (t3d.abs() + r64.abs()) + 2.0 ** -24 * ref.abs()
    err = (got - ref).abs()
    assert bool((err <= bound).all()), f"max err/bound {float((err / bound).max()):.3g}"
    del x


def _w4_head_rows(bb, yy, xx, h, w):
    """mrcnn_conv3x3_winograd4_heads_rows' row of pixel (b, y, x) (include/maskrcnn_hip.h)."""
    mt = (bb * ((h + 15) // 16) + yy // 16) * ((w + 31) // 32) + xx // 32
    return mt * 512 + (((yy // 4) & 3) * 8 + ((xx // 4) & 7)) * 16 + (yy & 3) * 4 + (xx & 3)


def test_winograd4_heads_at_the_top_of_the_range(dev):
    """The RPN level on F(4x4) with its heads in the epilogue (mrcnn_conv3x3_winograd4_heads_f32) on B16 x 256 x 252, 1024 -> 64:
    a 3.94 GiB input (4 px Cin <= OOB, 0.98 of it), ragged in W (252 = 7 x 32 + 28). (a) sampled pixels, the ones whose input
    bytes cross 2^31 included: the head sums against float64 (the shared activation within F(4x4)'s 1e-4 absolute bar, carried
    through the head weights); (b) the last image alone, bit for bit; (c) guard bands around head_part."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import check, lib
    b, h, w, cin, cout = 16, 256, 252, 1024, 64
    m = b * h * w
    assert 0.95 * OOB <= 4 * m * cin <= OOB and ops.conv3x3_winograd4_supported(h, w, cin, cout, b)
    x = _randn((b, h, w, cin), 91, dev)
    w2 = _randn((cout, 3, 3, cin), 92, dev, math.sqrt(2.0 / (9 * cin)))
    s2, t2 = _scale(cout, 93, dev), _randn((cout,), 94, dev, 0.1)
    wh = torch.zeros(32, cout, device=dev)
    wh[:18] = _randn((18, cout), 95, dev, 1.0 / 8)
    u4 = ops.winograd4_weights(w2)
    # pixels whose 3x3 receptive field holds the input pixel at byte 2^31
    px = GIB2 // (4 * cin)
    cb, cy, cx = px // (h * w), (px % (h * w)) // w, px % w
    cross = [cb * h * w + yy * w + xx for yy in range(cy - 1, cy + 2) for xx in range(cx - 1, cx + 2) if 0 <= yy < h and 0 <= xx < w]
    rows = _sample_rows(m, 4096, cross, seed=96, count=600)
    p64 = _patches(x, rows, 3, 3, 1, 1, 1, h, w)
    xl = x[b - 1:].contiguous()
    xk = ops.nhwc_to_kblocked(x)
    del x
    nrows = int(lib.mrcnn_conv3x3_winograd4_heads_rows(b, h, w))
    assert nrows == b * 16 * 8 * 512
    buf, part = _guarded(nrows * 32, dev)
    check(lib.mrcnn_conv3x3_winograd4_heads_f32(xk.data_ptr(), b, h, w, cin, u4.data_ptr(), cout, s2.data_ptr(), t2.data_ptr(), 1,
                                                wh.data_ptr(), part.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _bands_intact(buf, nrows * 32)
    del xk
    part2 = part.view(nrows, 32)
    # (b) the valid pixels of the last image
    alone = ops.conv3x3_winograd4_heads(ops.nhwc_to_kblocked(xl), u4, s2, t2, wh, True)
    torch.cuda.synchronize()
    yy, xx = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    r1 = _w4_head_rows(0, yy.reshape(-1), xx.reshape(-1), h, w)
    assert torch.equal(alone.part.view(-1, 32)[r1], part2[r1 + (b - 1) * (nrows // b)])
    del alone, xl
    # (a)
    bb, rem = rows // (h * w), rows % (h * w)
    got = part2[_w4_head_rows(bb, rem // w, rem % w, h, w).to(dev)].cpu().double()
    del buf, part, part2
    t = _f4_rows_bound(p64, w2.view(cout, -1).cpu(), s2.cpu(), t2.cpu())
    whd = wh.cpu().double()
    ref = t @ whd.t()
    bound = 1e-4 * whd.abs().sum(1) + (cout + 2) * 2.0 ** -24 * (t.abs() @ whd.abs().t()) + 1e-30
    err = (got - ref).abs()
    assert bool((err <= bound).all()), f"max err/bound {float((err / bound).max()):.3g}"


def test_winograd2_at_the_top_of_the_range(dev):
    """F(2x2) (mrcnn_conv3x3_winograd_f32) on B4 x 512 x 510, 1024 -> 1000 (ragged N): a 3.98 GiB input (4 px max(Cin, Cout) <=
    OOB, 0.996 of it). An NHWC input through the workspace into an NHWC output on the spatial tiles, then the workspace's
    k-blocked copy into a k-blocked output on the linear tiles: both outputs agree bit for bit. (a) sampled pixels, the ones
    whose input bytes cross 2^31 included, against float64 at the 1e-4 absolute bar of the full-size tests (unit-scale data);
    (b) the last image alone, bit for bit; (c) guard bands around both outputs."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import check, lib
    b, h, w, cin, cout = 4, 512, 510, 1024, 1000
    m = b * h * w
    assert 0.95 * OOB <= 4 * m * max(cin, cout) <= OOB
    x = _randn((b, h, w, cin), 101, dev)
    wt = _randn((cout, 3, 3, cin), 102, dev, math.sqrt(2.0 / (9 * cin)))
    scale, shift = _scale(cout, 103, dev), _randn((cout,), 104, dev, 0.1)
    u = ops.winograd_weights(wt)
    px = GIB2 // (4 * cin)
    cb, cy, cx = px // (h * w), (px % (h * w)) // w, px % w
    cross = [cb * h * w + yy * w + xx for yy in range(cy - 1, cy + 2) for xx in range(cx - 1, cx + 2) if 0 <= yy < h and 0 <= xx < w]
    rows = _sample_rows(m, 64, cross, seed=105, count=600)
    p64 = _patches(x, rows, 3, 3, 1, 1, 1, h, w)
    xl = x[b - 1:].contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    wsb = int(lib.mrcnn_conv3x3_winograd_workspace_bytes(b, h, w, cin))
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
    buf, y = _guarded(m * cout, dev)
    try:
        ops.winograd_set_spatial(1)
        check(lib.mrcnn_conv3x3_winograd_f32(x.data_ptr(), 0, b, h, w, cin, u.data_ptr(), cout, scale.data_ptr(), shift.data_ptr(),
                                             1, y.data_ptr(), None, ws.data_ptr(), wsb, stream))
        torch.cuda.synchronize()
        del x
        bufk, yk = _guarded(m * cout, dev)
        ops.winograd_set_spatial(0)
        check(lib.mrcnn_conv3x3_winograd_f32(ws.data_ptr(), 1, b, h, w, cin, u.data_ptr(), cout, scale.data_ptr(), shift.data_ptr(),
                                             1, None, yk.data_ptr(), None, 0, stream))
        torch.cuda.synchronize()
    finally:
        ops.winograd_set_spatial(-1)
    del ws
    assert _bands_intact(buf, m * cout) and _bands_intact(bufk, m * cout)
    y2, yk3 = y.view(m, cout), yk.view(cout // 8, m, 8)
    for g in range(cout // 8):
        assert torch.equal(yk3[g], y2[:, 8 * g:8 * g + 8]), f"k-blocked / linear tiles differ from NHWC / spatial, channels {8 * g}.."
    del bufk, yk, yk3
    alone = ops.conv3x3_winograd(xl, u, scale, shift, True)
    torch.cuda.synchronize()
    assert torch.equal(alone.view(-1, cout), y2[(b - 1) * h * w:])
    del alone, xl
    got = y2[rows.to(dev)].cpu().double()
    del buf, y, y2
    ref = _f4_rows_bound(p64, wt.view(cout, -1).cpu(), scale.cpu(), shift.cpu())
    err = (got - ref).abs()
    assert float(err.max()) <= 1e-4, f"max|err| {float(err.max()):.3e} > 1e-4 abs (max|ref| {float(ref.abs().max()):.2f})"


@pytest.mark.parametrize("out_f16", [False, True], ids=["f32", "f16out"])
def test_stem_at_the_top_of_the_range(dev, out_f16):
    """The stem conv 7x7 s2 on the NCHW image (mrcnn_stem_conv7x7_s2_nchw_f32 / _f16out) on B16 x 2048 x 2040: the fp32 output is
    3.98 GiB (y <= OOB, 0.996 of it; the fp16 form's is half). (a) sampled output pixels, the ones whose output bytes cross 2^31
    included, against float64 within the fp32 sum bound (+ 2^-11 |ref| for the fp16 store); (b) the last image alone, bit for
    bit; (c) guard bands."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import check, lib
    b, h, w = 16, 2048, 2040
    oh, ow = h // 2, w // 2
    m = b * oh * ow
    assert 0.95 * OOB <= 4 * m * 64 <= OOB
    x = _randn((b, 3, h, w), 111, dev)
    wt = torch.zeros(64, 7, 7, 4, device=dev)
    wt[..., :3] = _randn((64, 7, 7, 3), 112, dev, math.sqrt(2.0 / 147))
    scale, shift = _scale(64, 113, dev), _randn((64,), 114, dev, 0.1)
    dtype = torch.float16 if out_f16 else torch.float32
    buf, y = _guarded_t(m * 64, dev, dtype)
    fn = lib.mrcnn_stem_conv7x7_s2_nchw_f16out if out_f16 else lib.mrcnn_stem_conv7x7_s2_nchw_f32
    check(fn(x.data_ptr(), b, h, w, wt.data_ptr(), scale.data_ptr(), shift.data_ptr(), 1, y.data_ptr(),
             torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((buf[:BAND] == 7.0).all()) and bool((buf[BAND + m * 64:] == 7.0).all())
    y2 = y.view(m, 64)
    alone = ops.stem_conv(x[b - 1:].contiguous(), wt, scale, shift, True, nchw=True, out_f16=out_f16)
    torch.cuda.synchronize()
    assert torch.equal(alone.view(-1, 64), y2[(b - 1) * oh * ow:])
    del alone
    cross = GIB2 // (4 * 64)
    rows = _sample_rows(m, 256, range(cross - 2, cross + 3), seed=115)
    got = y2[rows.to(dev)].cpu().double()
    del buf, y, y2
    p64 = _patches(x.permute(0, 2, 3, 1), rows, 7, 7, 2, 3, 3, oh, ow)
    w2d = wt[..., :3].reshape(64, -1).cpu().double()
    sc, sh = scale.cpu().double(), shift.cpu().double()
    ref = ((p64 @ w2d.t()) * sc + sh).clamp_min(0)
    bound = 149 * 2.0 ** -24 * (p64.abs() @ w2d.abs().t()) * sc + 2.0 ** -23 * sh.abs() + 1e-30
    if out_f16:
        bound = bound + 2.0 ** -11 * ref.abs() + 2.0 ** -25
    err = (got - ref).abs()
    assert bool((err <= bound).all()), f"max err/bound {float((err / bound).max()):.3g}"
    del x


def test_conv_f16_pipelined_at_the_top_of_the_range(dev):
    """The pipelined fp16 conv (mrcnn_conv_f16_pipelined) on B8 x 512 x 508, 3x3 256 -> 256: its fp32 output is 1.98 GiB (the check
    is y32 < 2^31 bytes; 0.99 of it), written with the fp16 copy in one call; then with an fp16 residual of the output's size, and
    at half size (res_div 2), into fp16 outputs. (a) sampled pixels, the ones whose fp32 output bytes cross 2^30 and 2^31 - 2^20
    included, against float64 on the fp16-rounded operands: the fp32 sum bound, + 2^-11 |ref| for an fp16 output; (b) the last
    image alone, bit for bit; (c) guard bands. 512 x 512 is refused and writes nothing."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import MaskrcnnHipError, check, lib
    b, h, w, c = 8, 512, 508, 256
    m = b * h * w
    assert 0.95 * GIB2 <= 4 * m * c < GIB2 and ops.conv_f16_pipelined_supported(b, h, w, c, c, 3, 3, (1, 1, 1, 1))
    assert not ops.conv_f16_pipelined_supported(b, h, w + 4, c, c, 3, 3, (1, 1, 1, 1))
    x = _randn((b, h, w, c), 121, dev).half()
    wt = _randn((c, 3, 3, c), 122, dev, math.sqrt(2.0 / (9 * c))).half()
    scale, shift = _scale(c, 123, dev), _randn((c,), 124, dev, 0.1)
    stream = torch.cuda.current_stream().cuda_stream
    cross = [(1 << 30) // (4 * c), (GIB2 - (1 << 20)) // (4 * c), m - 1]
    rows = _sample_rows(m, 256, [r + d for r in cross for d in (-1, 0, 1)], seed=125, count=500)
    rd = rows.to(dev)
    p64 = _patches(x, rows, 3, 3, 1, 1, 1, h, w)
    w2d = wt.view(c, -1).cpu().double()
    sc, sh = scale.cpu().double(), shift.cpu().double()
    base = (p64 @ w2d.t()) * sc + sh
    sum_bound = (9 * c + 2) * 2.0 ** -24 * (p64.abs() @ w2d.abs().t()) * sc + 2.0 ** -23 * sh.abs() + 1e-30

    def call(xx, bb, y16, y32, res, res_div):
        check(lib.mrcnn_conv_f16_pipelined(xx.data_ptr(), bb, h, w, c, wt.data_ptr(), c, 3, 3, 1, 1, 1, 1, 1, scale.data_ptr(),
                                           shift.data_ptr(), None if res is None else res.data_ptr(), res_div, 1,
                                           None if y16 is None else y16.data_ptr(), None if y32 is None else y32.data_ptr(),
                                           0, 0, stream))

    def check_rows(got, ref, bound, what):
        err = (got.double() - ref).abs()
        assert bool((err <= bound).all()), f"{what}: max err/bound {float((err / bound).max()):.3g}"

    # fp32 + fp16 outputs, no residual
    buf32, y32 = _guarded_t(m * c, dev, torch.float32)
    buf16, y16 = _guarded_t(m * c, dev, torch.float16)
    call(x, b, y16, y32, None, 1)
    torch.cuda.synchronize()
    for bf, n in ((buf32, m * c), (buf16, m * c)):
        assert bool((bf[:BAND] == 7.0).all()) and bool((bf[BAND + n:] == 7.0).all())
    ref = base.clamp_min(0)
    check_rows(y32.view(m, c)[rd].cpu(), ref, sum_bound, "fp32 output")
    check_rows(y16.view(m, c)[rd].cpu(), ref, sum_bound + 2.0 ** -11 * ref.abs() + 2.0 ** -25, "fp16 output")
    xl = x[b - 1:].contiguous()
    a16, a32 = ops.conv_f16_pipelined(xl, wt, scale, shift, (1, 1, 1, 1), True, out_f16=True, out_f32=True)
    torch.cuda.synchronize()
    assert torch.equal(a32.view(-1, c), y32.view(m, c)[(b - 1) * h * w:])
    assert torch.equal(a16.view(-1, c), y16.view(m, c)[(b - 1) * h * w:])
    del buf32, y32, a16, a32
    # fp16 residual, full size and half size (FPN nearest-upsample-add), fp16 output
    for res_div in (1, 2):
        res = _randn((b, h // res_div, w // res_div, c), 126 + res_div, dev).half()
        buf16.fill_(7.0)
        call(x, b, y16, None, res, res_div)
        torch.cuda.synchronize()
        assert bool((buf16[:BAND] == 7.0).all()) and bool((buf16[BAND + m * c:] == 7.0).all())
        bb, rem = rd // (h * w), rd % (h * w)
        r64 = res[bb, (rem // w) // res_div, (rem % w) // res_div].cpu().double()
        ref = (base + r64).clamp_min(0)
        check_rows(y16.view(m, c)[rd].cpu(), ref, sum_bound + 2.0 ** -24 * r64.abs() + 2.0 ** -11 * ref.abs() + 2.0 ** -25,
                   f"res_div {res_div}")
        a16 = ops.conv_f16_pipelined(xl, wt, scale, shift, (1, 1, 1, 1), True, res[b - 1:].contiguous(), res_div=res_div)
        torch.cuda.synchronize()
        assert torch.equal(a16.view(-1, c), y16.view(m, c)[(b - 1) * h * w:]), res_div
        del res, a16
    del buf16, y16, xl
    # the first width past the check (512 x 512: y32 = 2^31 bytes) is refused, with allocations of the size it names
    x2 = torch.zeros(b, h, w + 4, c, dtype=torch.float16, device=dev)
    del x
    buf, y = _guarded_t(b * h * (w + 4) * c, dev, torch.float16)
    with pytest.raises(MaskrcnnHipError, match="32-bit byte offsets"):
        check(lib.mrcnn_conv_f16_pipelined(x2.data_ptr(), b, h, w + 4, c, wt.data_ptr(), c, 3, 3, 1, 1, 1, 1, 1, None, None, None,
                                           1, 1, y.data_ptr(), None, 0, 0, stream))
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    del x2, buf, y


def test_crop_staged_past_2_to_the_31_bytes_per_image(dev, oracle):
    """crop_and_resize's staged kernel (csrc/crop.hip) on B2 x 256 x 1536^2: 2.25 GiB per image, 4.5 GiB in all. The path takes
    images of up to 2^32 bytes. A (box, channel slab) whose footprint is at most 256 16-byte slots is moved into LDS by LDS-DMA,
    and each group's source offset there is the signed 32-bit view of first_channel x chan_bytes: negative from channel 228 on.
    Larger footprints take the in-launch gather fallback (64-bit addressing). 14 x 14 crops of small boxes (4 - 60 px, some partly
    outside the map) in both images, which the host restatement of the footprint shows take the DMA path, and of large ones,
    against the oracle bit for bit on channel slabs copied to the host (each channel's crop depends only on that channel): the
    first group, the channels whose bytes cross 2^31, and the last group. Nothing is written outside the crops."""
    from maskrcnn_amd._lib import check, lib
    b, c, h, w, ch, cw = 2, 256, 1536, 1536, 14, 14
    chan = 4 * h * w
    assert GIB2 < c * chan < 1 << 32 and (c - 1) * chan > GIB2
    img = _randn((b, c, h, w), 131, dev)
    g = torch.Generator().manual_seed(132)
    # small boxes: 4 - 60 px by 4 - 16 px (either way round), anywhere on the map and a pixel or two over its edges
    ns = 40
    side = torch.stack([torch.randint(4, 17, (ns,), generator=g), torch.randint(4, 61, (ns,), generator=g)], 1).float()
    side = torch.where(torch.rand(ns, 1, generator=g) < 0.5, side, side.flip(1))
    a = torch.rand(ns, 2, generator=g) * (1535 + 40) - 20
    small = torch.cat([a, a + side], 1) / 1535
    small[:4] = torch.tensor([[-5., 100., 6., 150.], [1530., 1500., 1545., 1520.], [700., -8., 712., 20.],
                              [1520., 1531., 1539., 1540.]]) / 1535     # partly outside: top, bottom-right, left, corner
    n0 = 8
    a, z = torch.rand(n0, 2, generator=g) * 1.2 - 0.1, torch.rand(n0, 2, generator=g) * 0.6 + 0.02
    large = torch.cat([a, a + z], 1)
    large[0] = torch.tensor([0.0, 0.0, 1.0, 1.0])
    large[1] = torch.tensor([-0.3, 0.7, 0.4, 1.3])          # partly outside on two sides
    boxes = torch.cat([small, large]).contiguous()
    n = boxes.size(0)
    ind = (torch.arange(n) % b).to(torch.int32)
    slots = [_crop_footprint_slots(bx.tolist(), h, w, ch, cw) for bx in boxes]
    for im in range(b):
        dma = [i for i in range(n) if ind[i] == im and slots[i] is not None and slots[i] <= 256]
        partly = [i for i in dma if bool(((boxes[i] < 0) | (boxes[i] > 1)).any())]
        assert len(dma) >= 10 and len(partly) >= 1, (im, len(dma), len(partly))
    assert sum(s is not None and s > 256 for s in slots) >= 4
    bd, idd = boxes.to(dev), ind.to(dev)
    buf, crops = _guarded(n * c * ch * cw, dev)
    check(lib.mrcnn_crop_forward_f32(img.data_ptr(), b, c, h, w, bd.data_ptr(), idd.data_ptr(), n, 0.0, ch, cw, crops.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _bands_intact(buf, n * c * ch * cw)
    got = crops.view(n, c, ch, cw).cpu()
    first_neg = -(-GIB2 // chan)
    for lo, hi in ((0, 8), (first_neg - 8, first_neg + 8), (c - 8, c)):
        slab = img[:, lo:hi].contiguous().cpu()
        want = oracle.crop_forward(slab, boxes, ind, 0.0, ch, cw)
        assert torch.equal(got[:, lo:hi], want), f"channels {lo}..{hi - 1}: {int((got[:, lo:hi] != want).sum())} elements differ"
    del img, buf, crops


def test_bottleneck_fused_at_the_top_of_the_range(dev):
    """The fused fp32 identity Bottleneck (mrcnn_bottleneck_fused_f32) on B4 x 1024 x 1008: x and y 3.94 GiB each (4 px 256 <= OOB,
    0.98 of it). (b) the last image alone equals its slice, and the three per-layer launches (direct 1x1, F(2x2), direct 1x1 with
    the residual) on that image equal it, bit for bit; sampled pixels of the batch whose bytes cross 2^31 are compared with the
    per-layer launches on their image, bit for bit as well; (c) guard bands."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import check, lib
    b, h, w, c, p = 4, 1024, 1008, 256, 64
    m = b * h * w
    assert 0.95 * OOB <= 4 * m * c <= OOB and ops.bottleneck_fused_supported(h, w, c, p)
    x = _randn((b, h, w, c), 141, dev)
    w1 = _randn((p, 1, 1, c), 142, dev, math.sqrt(2.0 / c))
    w2 = _randn((p, 3, 3, p), 143, dev, math.sqrt(2.0 / (9 * p)))
    w3 = _randn((c, 1, 1, p), 144, dev, math.sqrt(1.0 / p))
    s1, s2, s3 = _scale(p, 145, dev), _scale(p, 146, dev), _scale(c, 147, dev)
    t1, t2, t3 = _randn((p,), 148, dev, 0.1), _randn((p,), 149, dev, 0.1), _randn((c,), 150, dev, 0.1)
    u2 = ops.winograd_weights(w2)
    buf, y = _guarded(m * c, dev)
    check(lib.mrcnn_bottleneck_fused_f32(x.data_ptr(), b, h, w, c, w1.data_ptr(), s1.data_ptr(), t1.data_ptr(), u2.data_ptr(),
                                         s2.data_ptr(), t2.data_ptr(), w3.data_ptr(), s3.data_ptr(), t3.data_ptr(), p, y.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _bands_intact(buf, m * c)
    y4 = y.view(b, h, w, c)

    def layers(xi):
        t = ops.conv_bn_act(xi, w1, s1, t1, 1, (0, 0, 0, 0), True)
        t = ops.conv3x3_winograd(t, u2, s2, t2, True)
        return ops.conv_bn_act(t, w3, s3, t3, 1, (0, 0, 0, 0), True, xi)

    xl = x[b - 1:].contiguous()
    alone = ops.bottleneck_fused(xl, w1, s1, t1, u2, s2, t2, w3, s3, t3)
    per_layer = layers(xl)
    torch.cuda.synchronize()
    assert torch.equal(alone[0], y4[b - 1]) and torch.equal(per_layer, alone)
    del alone, per_layer, xl
    # the image holding byte 2^31 of x and y
    cb = (GIB2 // (4 * c)) // (h * w)
    ref = layers(x[cb:cb + 1].contiguous())[0]
    torch.cuda.synchronize()
    px = GIB2 // (4 * c) - cb * h * w
    rows = torch.unique(torch.cat([torch.arange(px - 2 * w, px + 2 * w), torch.randint(0, h * w, (2000,),
                                                                                       generator=torch.Generator().manual_seed(151))]))
    rd = rows.to(dev)
    assert torch.equal(y4[cb].view(-1, c)[rd], ref.view(-1, c)[rd]), f"image {cb}: differs from the per-layer launches"
    del buf, y, y4, x, ref


def _f16_round_bound(ref, e):
    """Error bound of fp16(v) against ref, for an fp32 v within e of ref (round to nearest, subnormal floor included)."""
    return e + 2.0 ** -11 * (ref.abs() + e) + 2.0 ** -25


def test_conv_f16_pipelined_heads_at_its_largest_batch(dev):
    """The RPN's shared 3x3 256 -> 512 with its heads in the pipelined fp16 kernel's epilogue (mrcnn_conv_f16_pipelined_heads) at its
    largest accepted batch on configs[4]'s P2, B15 x 208 x 336: the check counts the fp32 activation, 4 * M * 512 bytes = 0.9998 of
    2^31, though only the head sums are written; B16 is refused. (a) sampled pixels, the ones whose counted bytes cross 2^30 and
    2^31 - 2^20 included, per 256-channel plane against float64 on the fp16 operands, the activation rounded to fp16 as the kernel
    rounds it; (b) the last image alone, bit for bit; (c) guard bands around the head sums. The refused batch writes nothing."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import MaskrcnnHipError, check, lib
    b, h, w, cin, cout = 15, 208, 336, 256, 512
    m = b * h * w
    assert 0.99 * GIB2 <= 4 * m * cout < GIB2 and ops.conv_f16_pipelined_supported(b, h, w, cin, cout, 3, 3, (1, 1, 1, 1))
    assert not ops.conv_f16_pipelined_supported(b + 1, h, w, cin, cout, 3, 3, (1, 1, 1, 1))
    x = _randn((b, h, w, cin), 161, dev).half()
    wt = _randn((cout, 3, 3, cin), 162, dev, math.sqrt(2.0 / (9 * cin))).half()
    scale, shift = _scale(cout, 163, dev), _randn((cout,), 164, dev, 0.1)
    wh = torch.zeros(32, cout, dtype=torch.float16, device=dev)
    wh[:18] = _randn((18, cout), 165, dev, 1.0 / 16).half()
    stream = torch.cuda.current_stream().cuda_stream
    n = 2 * m * 32
    buf, part = _guarded(n, dev)
    check(lib.mrcnn_conv_f16_pipelined_heads(x.data_ptr(), b, h, w, cin, wt.data_ptr(), cout, 3, 3, 1, 1, 1, 1, scale.data_ptr(),
                                             shift.data_ptr(), 1, wh.data_ptr(), part.data_ptr(), 0, stream))
    torch.cuda.synchronize()
    assert _bands_intact(buf, n)
    part3 = part.view(2, m, 32)
    alone = ops.conv_f16_pipelined_heads(x[b - 1:].contiguous(), wt, scale, shift, wh)
    torch.cuda.synchronize()
    assert torch.equal(alone.part, part3[:, (b - 1) * h * w:])
    del alone
    cross = [(1 << 30) // (4 * cout), (GIB2 - (1 << 20)) // (4 * cout)]
    rows = _sample_rows(m, 256, [r + d for r in cross for d in (-1, 0, 1)], seed=166, count=500)
    got = part3[:, rows.to(dev)].cpu().double()                  # [2, S, 32]
    p64 = _patches(x, rows, 3, 3, 1, 1, 1, h, w)
    del buf, part, part3
    w2d = wt.view(cout, -1).cpu().double()
    sc, sh = scale.cpu().double(), shift.cpu().double()
    t = ((p64 @ w2d.t()) * sc + sh).clamp_min(0)
    e = (9 * cin + 2) * 2.0 ** -24 * (p64.abs() @ w2d.abs().t()) * sc + 2.0 ** -23 * sh.abs()
    et = _f16_round_bound(t, e)
    whd = wh.cpu().double()
    for j in range(2):
        cs = slice(256 * j, 256 * (j + 1))
        ref = t[:, cs] @ whd[:, cs].t()
        bound = et[:, cs] @ whd[:, cs].abs().t() + 258 * 2.0 ** -24 * (t[:, cs].abs() @ whd[:, cs].abs().t()) + 1e-30
        err = (got[j] - ref).abs()
        assert bool((err <= bound).all()), f"plane {j}: max err/bound {float((err / bound).max()):.3g}"
    # the first batch past the check, with allocations of the size it names
    x2 = torch.zeros(b + 1, h, w, cin, dtype=torch.float16, device=dev)
    buf, part = _guarded(2 * (b + 1) * h * w * 32, dev)
    with pytest.raises(MaskrcnnHipError):
        check(lib.mrcnn_conv_f16_pipelined_heads(x2.data_ptr(), b + 1, h, w, cin, wt.data_ptr(), cout, 3, 3, 1, 1, 1, 1, None, None, 1,
                                                 wh.data_ptr(), part.data_ptr(), 0, stream))
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    del x, x2, buf, part


def test_mask_tail_f16_at_the_top_of_the_range(dev):
    """The fused fp16 mask tail (mrcnn_mask_tail_f16: deconv 2x2 s2 + bias + ReLU -> conv5 1x1 + bias -> sigmoid) on 16 907 RoIs of
    14 x 14 x 256, 81 classes: the fp32 output is 4.0 GiB, the largest that keeps 16 m classes <= OOB - 64 KiB; 16 908 RoIs are
    refused and write nothing. (a) sampled output pixels, the ones whose bytes cross 2^31 included, against float64 on the fp16
    operands with the deconv output rounded to fp16 as the kernel rounds it; (b) the last RoI alone, bit for bit; (c) guard bands."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import MaskrcnnHipError, check, lib
    r, hw, c, classes = 16907, 14, 256, 81
    n = r * (2 * hw) ** 2 * classes
    assert 4 * n <= OOB - 65536 < 4 * (n + (2 * hw) ** 2 * classes) and ops.mask_tail_f16_supported(r, hw, hw, c, 256, classes)
    assert 4 * n >= 0.99 * OOB and not ops.mask_tail_f16_supported(r + 1, hw, hw, c, 256, classes)
    x = _randn((r, hw, hw, c), 171, dev).half()
    wde = _randn((4 * 256, 1, 1, c), 172, dev, 1.0 / 16).half()
    bde = _randn((256,), 173, dev, 0.1).repeat(4).contiguous()
    w5 = torch.zeros(96, 256, dtype=torch.float16, device=dev)
    w5[:classes] = _randn((classes, 256), 174, dev, 1.0 / 16).half()
    b5 = _randn((classes,), 175, dev, 0.1)
    fde, f5 = ops.pack_afrags_f16(wde), ops.pack_afrags_f16(w5)
    stream = torch.cuda.current_stream().cuda_stream
    buf, y = _guarded(n, dev)
    check(lib.mrcnn_mask_tail_f16(x.data_ptr(), r, hw, hw, c, fde.data_ptr(), bde.data_ptr(), 256, f5.data_ptr(), b5.data_ptr(),
                                  classes, y.data_ptr(), stream))
    torch.cuda.synchronize()
    assert _bands_intact(buf, n)
    m = r * (2 * hw) ** 2
    y2 = y.view(m, classes)
    alone = ops.mask_tail_f16(x[r - 1:].contiguous(), fde, bde, f5, b5)
    torch.cuda.synchronize()
    assert torch.equal(alone.view(-1, classes), y2[(r - 1) * (2 * hw) ** 2:])
    del alone
    cross = GIB2 // (4 * classes)
    rows = _sample_rows(m, 784, range(cross - 2, cross + 3), seed=176, count=600)
    got = y2[rows.to(dev)].cpu().double()
    del buf, y, y2
    rr, rem = rows // (4 * hw * hw), rows % (4 * hw * hw)
    yy, xx = rem // (2 * hw), rem % (2 * hw)
    q = (yy % 2) * 2 + xx % 2
    xin = x[rr.to(dev), (yy // 2).to(dev), (xx // 2).to(dev)].cpu().double()          # [S, 256]
    w4, b4 = wde.view(4, 256, c).cpu().double(), bde.view(4, 256).cpu().double()
    d = torch.empty(len(rows), 256, dtype=torch.float64)
    ed = torch.empty(len(rows), 256, dtype=torch.float64)
    for qq in range(4):                                   # the deconv's sub-pixel (dy, dx) of each sampled output pixel
        k = q == qq
        d[k] = xin[k] @ w4[qq].t() + b4[qq]
        ed[k] = 258 * 2.0 ** -24 * (xin[k].abs() @ w4[qq].abs().t()) + 2.0 ** -23 * b4[qq].abs()
    d = d.clamp_min(0)
    e16 = _f16_round_bound(d, ed)
    w5d, b5d = w5[:classes].cpu().double(), b5.cpu().double()
    z = d @ w5d.t() + b5d
    ez = e16 @ w5d.abs().t() + 258 * 2.0 ** -24 * (d.abs() @ w5d.abs().t()) + 2.0 ** -23 * b5d.abs()
    ref = torch.sigmoid(z)
    bound = 0.25 * ez + 2.0 ** -20
    err = (got - ref).abs()
    assert bool((err <= bound).all()), f"max err/bound {float((err / bound).max()):.3g}"
    del x
    x2 = torch.zeros(r + 1, hw, hw, c, dtype=torch.float16, device=dev)
    n2 = (r + 1) * (2 * hw) ** 2 * classes
    buf, y = _guarded(n2, dev)
    with pytest.raises(MaskrcnnHipError):
        check(lib.mrcnn_mask_tail_f16(x2.data_ptr(), r + 1, hw, hw, c, fde.data_ptr(), bde.data_ptr(), 256, f5.data_ptr(),
                                      b5.data_ptr(), classes, y.data_ptr(), stream))
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    del x2, buf, y


def _w2_head_rows(bb, yy, xx, h, w):
    """mrcnn_conv3x3_winograd_heads_rows' row of pixel (b, y, x) in tile mode 2 (include/maskrcnn_hip.h)."""
    mt = (bb * ((h + 15) // 16) + yy // 16) * ((w + 15) // 16) + xx // 16
    return mt * 256 + (((yy // 2) & 7) * 8 + ((xx // 2) & 7)) * 4 + (yy & 1) * 2 + (xx & 1)


def test_winograd2_heads_at_the_top_of_the_range(dev):
    """The RPN level on F(2x2) with its heads in the epilogue (mrcnn_conv3x3_winograd_heads_f32, tile mode 2) on B16 x 512 x 510,
    256 -> 512: a 3.98 GiB input (4 px Cin <= OOB, 0.996 of it), ragged in W (510 = 31 x 16 + 14). (a) sampled pixels, the ones
    whose input bytes cross 2^31 included: the sum of the two k halves against float64 (the shared activation within the 1e-4
    absolute bar, carried through the head weights); (b) the last image alone, bit for bit; (c) guard bands."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import check, lib
    b, h, w, cin, cout = 16, 512, 510, 256, 512
    m = b * h * w
    assert 0.99 * OOB <= 4 * m * cin <= OOB and int(lib.mrcnn_conv3x3_winograd_heads_tile_mode(h, w)) == 2
    x = _randn((b, h, w, cin), 181, dev)
    wt = _randn((cout, 3, 3, cin), 182, dev, math.sqrt(2.0 / (9 * cin)))
    scale, shift = _scale(cout, 183, dev), _randn((cout,), 184, dev, 0.1)
    wh = torch.zeros(32, cout, device=dev)
    wh[:18] = _randn((18, cout), 185, dev, 1.0 / 16)
    u = ops.winograd_weights(wt)
    px = GIB2 // (4 * cin)
    cb, cy, cx = px // (h * w), (px % (h * w)) // w, px % w
    cross = [cb * h * w + yy * w + xx for yy in range(cy - 1, cy + 2) for xx in range(cx - 1, cx + 2) if 0 <= yy < h and 0 <= xx < w]
    rows = _sample_rows(m, 256, cross, seed=186, count=600)
    p64 = _patches(x, rows, 3, 3, 1, 1, 1, h, w)
    xl = x[b - 1:].contiguous()
    xk = ops.nhwc_to_kblocked(x)
    del x
    nrows = int(lib.mrcnn_conv3x3_winograd_heads_rows(b, h, w, 2))
    assert nrows == b * 32 * 32 * 256
    buf, part = _guarded(2 * nrows * 32, dev)
    check(lib.mrcnn_conv3x3_winograd_heads_f32(xk.data_ptr(), b, h, w, cin, u.data_ptr(), cout, scale.data_ptr(), shift.data_ptr(),
                                               1, wh.data_ptr(), 2, part.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _bands_intact(buf, 2 * nrows * 32)
    del xk
    part3 = part.view(2, nrows, 32)
    alone = ops.conv3x3_winograd_heads(ops.nhwc_to_kblocked(xl), u, scale, shift, wh, True)
    torch.cuda.synchronize()
    yy, xx = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    r1 = _w2_head_rows(0, yy.reshape(-1), xx.reshape(-1), h, w)
    assert torch.equal(alone.part.view(2, -1, 32)[:, r1], part3[:, r1 + (b - 1) * (nrows // b)])
    del alone, xl
    bb, rem = rows // (h * w), rows % (h * w)
    got = part3[:, _w2_head_rows(bb, rem // w, rem % w, h, w).to(dev)].cpu().double().sum(0)
    del buf, part, part3
    t = _f4_rows_bound(p64, wt.view(cout, -1).cpu(), scale.cpu(), shift.cpu())
    whd = wh.cpu().double()
    ref = t @ whd.t()
    bound = 1e-4 * whd.abs().sum(1) + (cout + 4) * 2.0 ** -24 * (t.abs() @ whd.abs().t()) + 1e-30
    err = (got - ref).abs()
    assert bool((err <= bound).all()), f"max err/bound {float((err / bound).max()):.3g}"


@pytest.mark.parametrize("form", ["f32", "f16"])
def test_stem_pool_at_the_top_of_the_range(dev, form):
    """The stem conv 7x7 s2 + ReLU + SamePad(3, 2) max-pool in one launch: fp32 (mrcnn_stem_conv7x7_s2_pool_f32) on B32 x 2048 x 2040,
    a 1.99 GiB output (the check is 16 B H W < 2^31; 0.996 of it), and fp16 (_pool_f16) on B85 x 2048^2, a 3.98 GiB input (12 B H W
    <= OOB, 0.996 of it). (a) sampled pooled pixels, the ones whose output or input bytes cross 2^31 included, against the float64
    max over the 3 x 3 conv taps (fp16: on the fp16-rounded image and weights, each tap rounded to fp16), within the largest tap's
    fp32 sum bound; (b) the last image alone, bit for bit; (c) guard bands."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import check, lib
    b, h, w = (32, 2048, 2040) if form == "f32" else (85, 2048, 2048)
    if form == "f32":
        assert 0.99 * GIB2 <= 16 * b * h * w < GIB2
    else:
        assert 0.99 * OOB <= 12 * b * h * w <= OOB
    h2, w2, ph, pw = h // 2, w // 2, h // 4, w // 4
    m = b * ph * pw
    x = _randn((b, 3, h, w), 191, dev)
    wt = torch.zeros(64, 7, 7, 4, device=dev)
    wt[..., :3] = _randn((64, 7, 7, 3), 192, dev, math.sqrt(2.0 / 147))
    scale, shift = _scale(64, 193, dev), _randn((64,), 194, dev, 0.1)
    dtype = torch.float32 if form == "f32" else torch.float16
    buf, y = _guarded_t(m * 64, dev, dtype)
    fn = lib.mrcnn_stem_conv7x7_s2_pool_f32 if form == "f32" else lib.mrcnn_stem_conv7x7_s2_pool_f16
    check(fn(x.data_ptr(), b, h, w, wt.data_ptr(), scale.data_ptr(), shift.data_ptr(), y.data_ptr(),
             torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((buf[:BAND] == 7.0).all()) and bool((buf[BAND + m * 64:] == 7.0).all())
    y2 = y.view(m, 64)
    pool = ops.stem_pool_f32 if form == "f32" else ops.stem_pool_f16
    alone = pool(x[b - 1:].contiguous(), wt, scale, shift)
    torch.cuda.synchronize()
    assert torch.equal(alone.view(-1, 64), y2[(b - 1) * ph * pw:])
    del alone
    cross_out = GIB2 // (64 * y.element_size())
    cross_in = (GIB2 // (4 * h * w)) * ph * pw          # the first pooled pixel of the image that holds input byte 2^31
    rows = _sample_rows(m, 112, [r + d for r in (cross_out, cross_in) for d in range(-2, 3)], seed=195, count=500)
    got = y2[rows.to(dev)].cpu().double()
    del buf, y, y2
    # the 3 x 3 conv taps of each pooled pixel (rows 2py .. 2py + 2; the pool's bottom / right padding reads 0 <= ReLU output)
    bb, rem = rows // (ph * pw), rows % (ph * pw)
    py, pxx = rem // pw, rem % pw
    taps = []
    for dy in range(3):
        for dx in range(3):
            cy, cx = 2 * py + dy, 2 * pxx + dx
            taps.append(((cy < h2) & (cx < w2), bb * h2 * w2 + cy.clamp(max=h2 - 1) * w2 + cx.clamp(max=w2 - 1)))
    wts = wt[..., :3] if form == "f32" else wt[..., :3].half().float()
    w2d = wts.reshape(64, -1).cpu().double()
    sc, sh = scale.cpu().double(), shift.cpu().double()
    ref = torch.zeros(len(rows), 64, dtype=torch.float64)
    bound = torch.zeros(len(rows), 64, dtype=torch.float64)
    for ok, crow in taps:
        p64 = _patches(x.permute(0, 2, 3, 1), crow, 7, 7, 2, 3, 3, h2, w2)
        if form == "f16":                                 # the image rounded to fp16 once, as the kernel reads it
            p64 = p64.float().half().double()
        v = ((p64 @ w2d.t()) * sc + sh).clamp_min(0)
        e = 149 * 2.0 ** -24 * (p64.abs() @ w2d.abs().t()) * sc + 2.0 ** -23 * sh.abs()
        if form == "f16":
            e = _f16_round_bound(v, e)
        okd = ok.view(-1, 1).double()
        ref = torch.maximum(ref, v * okd)
        bound = torch.maximum(bound, e * okd)
    err = (got - ref).abs()
    assert bool((err <= bound + 1e-30).all()), f"max err/bound {float((err / (bound + 1e-30)).max()):.3g}"
    del x


# the fp16 tile kernel (csrc/conv_f16.hip) on the 1x1 conv of test_direct_conv_1x1_output_at_the_top_of_the_range: an fp32-sized
# output of exactly OOB bytes (fill_common counts every tensor at 4 bytes per element), ragged in M and N; the fp16 output, which
# stores channel pairs, has Cout 1904
@pytest.mark.parametrize("form", ["f16mfma_p3", "f16mfma_p1", "f16io_x16", "f16io_y16"])
def test_conv_f16_tile_kernel_at_the_top_of_the_range(dev, form):
    """mrcnn_conv_bn_act_nhwc_f16mfma (products 3 and 1, fp32 in and out) and mrcnn_conv_bn_act_nhwc_f16io (fp16 in / fp32 out,
    fp32 in / fp16 out) on 4 x 113 x 1247 pixels, 32 -> 1905 (1904 for the fp16 output). (a) sampled rows, the ones whose fp32-sized bytes cross 2^31
    included, against float64: on the fp16-rounded operands for the plain-fp16 forms (+ 2^-11 |ref| for an fp16 output), on the
    fp32 input and the hi + lo weights within 2^-20 per product for the 3-product split; (b) the last image alone, bit for bit;
    (c) guard bands."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import check, lib
    b, h, w, cin, cout = 4, 113, 1247, 32, 1904 if form == "f16io_y16" else 1905
    m = b * h * w
    n = m * cout
    assert 0.99 * OOB <= 4 * n <= OOB and m % 128 and cout % 128
    x = _randn((b, h, w, cin), 201, dev)
    wt = _randn((cout, 1, 1, cin), 202, dev, 1.0 / math.sqrt(cin))
    scale, shift = _scale(cout, 203, dev), _randn((cout,), 204, dev, 0.1)
    w_hi, w_lo = ops.split_f16(wt)
    x_in = x.half() if form == "f16io_x16" else x
    y16 = form == "f16io_y16"
    products = 3 if form == "f16mfma_p3" else 1
    stream = torch.cuda.current_stream().cuda_stream
    buf, y = _guarded_t(n, dev, torch.float16 if y16 else torch.float32)
    if form.startswith("f16mfma"):
        check(lib.mrcnn_conv_bn_act_nhwc_f16mfma(x.data_ptr(), b, h, w, cin, w_hi.data_ptr(), w_lo.data_ptr(), cout, 1, 1, 1, 0, 0,
                                                 0, 0, scale.data_ptr(), shift.data_ptr(), None, 1, 0, products, y.data_ptr(), stream))
    else:
        check(lib.mrcnn_conv_bn_act_nhwc_f16io(x_in.data_ptr(), 1 if form == "f16io_x16" else 0, b, h, w, cin, w_hi.data_ptr(), cout,
                                               1, 1, 1, 0, 0, 0, 0, scale.data_ptr(), shift.data_ptr(), None, 1, 0, y.data_ptr(),
                                               1 if y16 else 0, stream))
    torch.cuda.synchronize()
    assert bool((buf[:BAND] == 7.0).all()) and bool((buf[BAND + n:] == 7.0).all())
    y2 = y.view(m, cout)
    alone = ops.conv_bn_act_f16mfma(x_in[b - 1:].contiguous(), w_hi, w_lo if products == 3 else None, scale, shift,
                                    products=products, out_f16=y16)
    torch.cuda.synchronize()
    assert torch.equal(alone.view(-1, cout), y2[(b - 1) * h * w:])
    del alone
    cross = GIB2 // (4 * cout)
    rows = _sample_rows(m, 128, range(cross - 2, cross + 3), seed=205)
    got = y2[rows.to(dev)].cpu().double()
    del buf, y, y2
    sc, sh = scale.cpu().double(), shift.cpu().double()
    if products == 3:
        p64 = _patches(x, rows, 1, 1, 1, 0, 0, h, w)
        w2d = (w_hi.double() + w_lo.double()).view(cout, cin).cpu()
        absprod = p64.abs() @ w2d.abs().t()
        e = ((cin + 2) * 2.0 ** -24 + 2.0 ** -20) * absprod * sc + 2.0 ** -24 * w2d.abs().sum(1) * sc
    else:
        p64 = _patches(x.half().float(), rows, 1, 1, 1, 0, 0, h, w)
        w2d = w_hi.view(cout, cin).cpu().double()
        absprod = p64.abs() @ w2d.abs().t()
        e = (cin + 2) * 2.0 ** -24 * absprod * sc
    ref = (p64 @ w2d.t()) * sc + sh
    e = e + 2.0 ** -23 * sh.abs() + 1e-30
    if y16:
        e = _f16_round_bound(ref, e)
    err = (got - ref).abs()
    assert bool((err <= e).all()), f"{form}: max err/bound {float((err / e).max()):.3g}"
    del x, x_in
