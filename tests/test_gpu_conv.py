"""GPU parity tests (-m gpu) for the fused conv+BN+ReLU implicit-GEMM kernel and its helpers against
a torch CPU fp32 reference of the same op (this is the floating-point kernel: tolerance 1e-4 abs, the
bound BASELINE.json's north_star states, at controlled input scale: x ~ N(0,1), Xavier weights)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import maskrcnn_amd  # noqa: F401
    return torch.device("cuda:0")


def _over_the_clamp(per_cu=1, multiple_of=1):
    """The persistent launchers start min(units, per_cu * CUs) workgroups (CUs rounded down to whole XCDs where the launcher
    says so) and let a workgroup walk the units beyond its own. The small shapes of this file never reach that clamp; each
    launcher has one case with a width (or RoI count) of 0, which stands for "what puts the launcher just over its clamp on
    this device": one row of tiles, as many of them as this returns. The count is taken from the device's CU count, lies
    between one and two times the clamp and is no multiple of 8, so some workgroups walk two units, others one. "Units" are
    the tiles (work items) of the case; the Winograd and Bottleneck launchers round them up to whole groups of 8 (one per
    XCD) before they clamp, which only moves the count further over."""
    clamp = per_cu * torch.cuda.get_device_properties(0).multi_processor_count
    units = (clamp // multiple_of + 1) * multiple_of
    while units % 8 == 0 or units < clamp + 4:
        units += multiple_of
    assert clamp < units < 2 * clamp, (units, clamp)
    return units


def _ref_conv(x_nchw, w_oihw, scale, shift, stride, pad, relu, residual_nchw=None, res_div=1):
    pt, pl, pb, pr = pad
    y = F.conv2d(F.pad(x_nchw, (pl, pr, pt, pb)), w_oihw, None, stride=stride)
    if scale is not None:
        y = y * scale.view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.view(1, -1, 1, 1)
    if residual_nchw is not None:
        r = residual_nchw if res_div == 1 else F.interpolate(residual_nchw, scale_factor=res_div)
        y = y + r
    return F.relu(y) if relu else y


CASES = [
    # (B, H, W, Cin, Cout, k, stride, pad, relu, residual(0/1/2), affine)
    (2, 16, 16, 64, 64, 1, 1, (0, 0, 0, 0), True, 0, True),       # C2 conv1
    (2, 16, 16, 64, 64, 3, 1, (1, 1, 1, 1), True, 0, True),       # C2 conv2
    (2, 16, 16, 64, 256, 1, 1, (0, 0, 0, 0), True, 1, True),      # C2 conv3 + residual
    (2, 16, 16, 256, 128, 1, 2, (0, 0, 0, 0), True, 0, True),     # C3 conv1 stride 2
    (1, 16, 16, 256, 512, 1, 2, (0, 0, 0, 0), False, 0, True),    # C3 downsample
    (1, 8, 8, 512, 512, 3, 1, (1, 1, 1, 1), True, 0, True),       # C5 conv2, K = 4608
    (1, 8, 8, 2048, 512, 1, 1, (0, 0, 0, 0), True, 0, True),      # C5 conv1, K = 2048
    (1, 8, 8, 2048, 256, 1, 1, (0, 0, 0, 0), False, 0, False),    # P5 lateral (bias only)
    (2, 16, 16, 1024, 256, 1, 1, (0, 0, 0, 0), False, 2, False),  # P4 lateral + 2x-upsampled residual
    (1, 32, 32, 256, 256, 3, 1, (1, 1, 1, 1), False, 0, False),   # FPN smoothing
    (1, 16, 16, 256, 512, 3, 1, (1, 1, 1, 1), True, 0, False),    # RPN shared
    (1, 16, 16, 512, 18, 1, 1, (0, 0, 0, 0), False, 0, False),    # RPN class+bbox heads fused, N = 18
    (2, 64, 64, 4, 64, 7, 2, (3, 3, 3, 3), True, 0, True),        # stem, Cin padded 3 -> 4 (generic K)
    (3, 13, 11, 32, 48, 3, 1, (1, 1, 1, 1), True, 1, True),       # ragged: odd sizes, N % 32 != 0
    (1, 9, 7, 32, 40, 3, 2, (0, 0, 1, 1), False, 0, True),        # asymmetric SAME pad (0,0,1,1)
    (37, 1, 1, 12544, 1024, 1, 1, (0, 0, 0, 0), True, 0, True),   # classifier conv1 as GEMM (K = 7*7*256)
    (300, 1, 1, 1024, 405, 1, 1, (0, 0, 0, 0), False, 0, False),  # class + bbox FC fused (N = 81 + 324)
    (1, 5, 5, 32, 8, 3, 1, (1, 1, 1, 1), False, 0, False),        # tiny M = 25
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c[:7]))
def test_conv_bn_act_vs_torch_cpu(dev, case):
    from maskrcnn_amd import ops
    b, h, w, cin, cout, k, stride, pad, relu, res, affine = case
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    x = torch.randn(b, cin, h, w, generator=g)
    fan = cin * k * k
    wt = (torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * math.sqrt(6.0 / (fan + cout * k * k))
    scale = (torch.rand(cout, generator=g) + 0.5) if affine else None
    shift = torch.randn(cout, generator=g) * 0.1
    oh = (h + pad[0] + pad[2] - k) // stride + 1
    ow = (w + pad[1] + pad[3] - k) // stride + 1
    residual = None
    if res:
        residual = torch.randn(b, cout, oh // res, ow // res, generator=g)
    want = _ref_conv(x, wt, scale, shift, stride, pad, relu, residual, max(res, 1))
    to_nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev)
    got = ops.conv_bn_act(to_nhwc(x), to_nhwc(wt), None if scale is None else scale.to(dev),
                          shift.to(dev), stride, pad, relu,
                          None if residual is None else to_nhwc(residual), max(res, 1))
    got = got.permute(0, 3, 1, 2).cpu()
    assert got.shape == want.shape
    err = (got - want).abs().max().item()
    assert err <= TOL, f"max abs err {err:.3e}"


def test_conv_exactness_identity(dev):
    """A = I check with asymmetric data: a 1x1 conv with identity weights must copy x bit for bit, and
    a permutation weight must permute channels exactly (catches fragment/row-col mapping slips)."""
    from maskrcnn_amd import ops
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 9, 10, 64, generator=g).to(dev)
    eye = torch.eye(64).view(64, 1, 1, 64).contiguous().to(dev)
    assert torch.equal(ops.conv_bn_act(x, eye, None, None), x)
    perm = torch.randperm(64, generator=g)
    pw = torch.eye(64)[perm].view(64, 1, 1, 64).contiguous().to(dev)
    assert torch.equal(ops.conv_bn_act(x, pw, None, None), x[..., perm.to(dev)])
    # integer-valued data: every product/sum exact in fp32 → must match the CPU bit for bit
    xi = torch.randint(-4, 5, (1, 64, 12, 12), generator=g).float()
    wi = torch.randint(-3, 4, (96, 64, 3, 3), generator=g).float()
    want = F.conv2d(xi, wi, padding=1)
    got = ops.conv_bn_act(xi.permute(0, 2, 3, 1).contiguous().to(dev),
                          wi.permute(0, 2, 3, 1).contiguous().to(dev), None, None, 1, (1, 1, 1, 1))
    assert torch.equal(got.permute(0, 3, 1, 2).cpu(), want)


def test_bottleneck_golden(dev):
    """Reference Bottleneck modules (weights stored in the fixture) vs the fused op."""
    from maskrcnn_amd import modules
    z = load_golden("graph_small")
    for i in range(int(z["n_bottleneck"])):
        sd = {k[len(f"b{i}_sd_"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"b{i}_sd_")}
        x = torch.from_numpy(z[f"b{i}_x"])
        cin = x.size(1)
        if cin % 4:
            continue
        for precision in ("f32", "f16x3"):
            if precision != "f32" and cin % 8:
                continue
            blk = modules.FusedBottleneck.from_state_dict(sd, "", int(z[f"b{i}_stride"]), dev, precision)
            y = blk(x.permute(0, 2, 3, 1).contiguous().to(dev)).permute(0, 3, 1, 2).cpu()
            err = (y - torch.from_numpy(z[f"b{i}_y"])).abs().max().item()
            assert err <= TOL, (i, precision, err)


def test_maxpool_and_layout(dev):
    from maskrcnn_amd import ops
    g = torch.Generator().manual_seed(2)
    for (b, c, h, w) in [(2, 64, 16, 16), (1, 8, 9, 12), (1, 4, 7, 7)]:
        x = torch.randn(b, c, h, w, generator=g)  # signed: the zero pad must take part in the max
        pad = ops.same_pad(h, w, 3, 2)
        want = F.max_pool2d(F.pad(x, (pad[1], pad[3], pad[0], pad[2])), 3, 2)
        xn = ops.nchw_to_nhwc(x.to(dev))
        assert torch.equal(xn.cpu(), x.permute(0, 2, 3, 1))
        got = ops.nhwc_to_nchw(ops.maxpool(xn, 3, 2, pad)).cpu()
        assert torch.equal(got, want)
        p6 = ops.nhwc_to_nchw(ops.maxpool(xn, 1, 2)).cpu()
        assert torch.equal(p6, x[:, :, ::2, ::2])
    x3 = torch.randn(2, 3, 10, 6, generator=g)
    y = ops.nchw_to_nhwc(x3.to(dev), 4).cpu()
    assert torch.equal(y[..., :3], x3.permute(0, 2, 3, 1)) and bool((y[..., 3] == 0).all())
    assert ops.same_pad(8, 8, 3, 2) == (0, 0, 1, 1) and ops.same_pad(8, 8, 3, 1) == (1, 1, 1, 1)


F16_CASES = [c for c in CASES if c[3] % 8 == 0] + [(2, 32, 32, 8, 64, 7, 2, (3, 3, 3, 3), True, 0, True)]


@pytest.mark.parametrize("case", F16_CASES, ids=lambda c: "x".join(str(v) for v in c[:7]))
def test_conv_f16mfma_vs_torch_cpu(dev, case):
    """fp16-operand MFMA kernel. products=3 (error-compensated split) must meet the SAME 1e-4 abs bar as the
    fp32 kernel; products=1 (plain fp16 operands, config 5) is held to its own stated tolerance:
    2e-3 * sqrt(K) * max|w| * max|x| (fp16 has 11 significand bits)."""
    from maskrcnn_amd import ops
    b, h, w, cin, cout, k, stride, pad, relu, res, affine = case
    g = torch.Generator().manual_seed((hash(case) + 17) % (2 ** 31))
    x = torch.randn(b, cin, h, w, generator=g)
    fan = cin * k * k
    wt = (torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * math.sqrt(6.0 / (fan + cout * k * k))
    scale = (torch.rand(cout, generator=g) + 0.5) if affine else None
    shift = torch.randn(cout, generator=g) * 0.1
    oh = (h + pad[0] + pad[2] - k) // stride + 1
    ow = (w + pad[1] + pad[3] - k) // stride + 1
    residual = torch.randn(b, cout, oh // res, ow // res, generator=g) if res else None
    want = _ref_conv(x, wt, scale, shift, stride, pad, relu, residual, max(res, 1))
    to_nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev)
    w_hi, w_lo = ops.split_f16(to_nhwc(wt))
    for products, tol in ((3, TOL), (1, 2e-3 * math.sqrt(fan) * wt.abs().max().item() * x.abs().max().item())):
        got = ops.conv_bn_act_f16mfma(to_nhwc(x), w_hi, w_lo, None if scale is None else scale.to(dev),
                                      shift.to(dev), stride, pad, relu,
                                      None if residual is None else to_nhwc(residual), max(res, 1), products)
        err = (got.permute(0, 3, 1, 2).cpu() - want).abs().max().item()
        assert err <= tol, f"products={products}: max abs err {err:.3e} > {tol:.3e}"


def test_conv_f16x3_is_fp32_grade_at_large_magnitude(dev):
    """The split keeps 22 significand bits per operand: relative error stays ~1e-6 for |x| up to 1e4."""
    from maskrcnn_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 12, 12, 256, generator=g) * 3000.0
    wt = torch.randn(128, 3, 3, 256, generator=g) * 0.02
    want = F.conv2d(x.permute(0, 3, 1, 2).double(), wt.permute(0, 3, 1, 2).double(), padding=1)
    w_hi, w_lo = ops.split_f16(wt.to(dev))
    got = ops.conv_bn_act_f16mfma(x.to(dev), w_hi, w_lo, None, None, 1, (1, 1, 1, 1), False, None, 1, 3)
    f32 = ops.conv_bn_act(x.to(dev), wt.to(dev), None, None, 1, (1, 1, 1, 1))
    ref_scale = want.abs().max().item()
    e3 = (got.permute(0, 3, 1, 2).cpu().double() - want).abs().max().item() / ref_scale
    e32 = (f32.permute(0, 3, 1, 2).cpu().double() - want).abs().max().item() / ref_scale
    assert e3 < 5e-6, e3
    assert e3 < 20 * max(e32, 1e-8), (e3, e32)   # within a small factor of the exact-fp32 kernel's own error


def test_bottleneck_module_dropin(dev):
    """`Bottleneck(inplanes, planes, stride, downsample)` nn.Module: reference constructor and state-dict keys,
    NCHW in/out, reloads its folded parameters when the weights change."""
    from maskrcnn_amd import modules
    z = load_golden("graph_small")
    i = 2  # (32 -> 16 planes, stride 2, with downsample)
    sd = {k[len(f"b{i}_sd_"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"b{i}_sd_")}
    down = torch.nn.Sequential(torch.nn.Conv2d(32, 64, kernel_size=1, stride=2),
                               torch.nn.BatchNorm2d(64, eps=0.001, momentum=0.01))
    blk = modules.Bottleneck(32, 16, 2, down)
    assert sorted(blk.state_dict().keys()) == sorted(sd.keys())
    blk.load_state_dict(sd)
    blk = blk.to(dev).eval()
    x = torch.from_numpy(z[f"b{i}_x"]).to(dev)
    with torch.no_grad():
        y = blk(x)
        assert (y.cpu() - torch.from_numpy(z[f"b{i}_y"])).abs().max().item() <= TOL
        blk.conv3.bias.add_(1.0)          # parameter change must invalidate the folded copy
        y2 = blk(x)
    assert (y2 - y).abs().max().item() > 1e-3
    blk.train()
    with pytest.raises(RuntimeError):
        blk(x)


# --------------------------------------------------------------------------------------------------
# Winograd F(2x2,3x3) kernel (csrc/conv_wino.hip): same 1e-4 bar against torch CPU, x ~ N(0,1), Xavier weights
# --------------------------------------------------------------------------------------------------
WINO_CASES = [
    # (B, H, W, Cin, Cout, relu, affine)
    (2, 16, 16, 64, 64, True, True),      # C2 conv2
    (2, 32, 32, 256, 256, True, True),    # FPN smoothing / C4 conv2
    (1, 32, 32, 256, 512, True, False),   # RPN conv_shared (bias only)
    (7, 14, 14, 256, 256, True, True),    # mask head: 49 tile positions per RoI, ragged last workgroup
    (2, 14, 14, 64, 96, False, True),     # Cout not a multiple of 64
    (1, 2, 2, 8, 5, False, False),        # one tile position, one k tile
    (1, 32, 48, 24, 40, True, True),      # non-square, three k tiles
    (3, 16, 16, 512, 64, True, True),     # long K
    (1, 6, 10, 16, 70, True, True),       # FPN P5 of the 192x320 configuration
    (1, 8, 0, 8, 64, True, True),         # over the clamp (width 0: _over_the_clamp), 4 positions high: always linear tiles
    (1, 16, 0, 8, 64, True, True),        # over the clamp, 8 positions high: one row of 8 x 8 blocks (or as many linear tiles)
]


@pytest.mark.parametrize("case", WINO_CASES, ids=lambda c: "x".join(str(v) for v in c[:5]))
def test_conv3x3_winograd_vs_torch_cpu(dev, case):
    from maskrcnn_amd import ops
    b, h, w, cin, cout, relu, affine = case
    if w == 0:   # 64 positions per M tile either way: 4 x 16 (linear) or 8 x 8 (a block, or 64 consecutive positions of 8 rows)
        w = (32 if h == 8 else 16) * _over_the_clamp()
        case = (b, h, w, cin, cout, relu, affine)
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
    scale = (torch.rand(cout, generator=g) + 0.5) if affine else None
    shift = torch.randn(cout, generator=g) * 0.1
    ref = _ref_conv(x, wt, scale, shift, 1, (1, 1, 1, 1), relu).permute(0, 2, 3, 1)
    u = ops.winograd_weights(wt.permute(0, 2, 3, 1).contiguous().to(dev))
    y = ops.conv3x3_winograd(x.permute(0, 2, 3, 1).contiguous().to(dev), u,
                             None if scale is None else scale.to(dev), shift.to(dev), relu)
    err = (y.cpu() - ref).abs().max().item()
    assert err <= TOL, f"max abs err {err:.3e} (|ref|max {ref.abs().max().item():.2f})"


def test_conv3x3_winograd_matches_direct_kernel_full_size(dev):
    """BASELINE shapes (P3-level FPN smoothing at batch 8; the mask head's 400 x 14 x 14): within 1e-4 of the exact
    direct kernel relative to the activation scale, and bit-identical run to run."""
    from maskrcnn_amd import ops
    g = torch.Generator().manual_seed(77)
    for (b, h, w, cin, cout) in ((8, 128, 128, 256, 256), (400, 14, 14, 256, 256)):
        x = torch.randn(b, h, w, cin, generator=g).to(dev)
        wt = (torch.randn(cout, 3, 3, cin, generator=g) * math.sqrt(2.0 / (9 * cin))).to(dev)
        sh = (torch.randn(cout, generator=g) * 0.1).to(dev)
        u = ops.winograd_weights(wt)
        y = ops.conv3x3_winograd(x, u, None, sh, True)
        yd = ops.conv_bn_act(x, wt, None, sh, 1, (1, 1, 1, 1), True)
        assert (y - yd).abs().max().item() <= TOL * max(1.0, yd.abs().max().item())
        assert torch.equal(y, ops.conv3x3_winograd(x, u, None, sh, True))


def test_winograd_spatial_and_linear_tiles_are_bit_identical(dev):
    """The two Winograd kernels (8 x 8 position blocks with a per-lane transform out of a raw LDS region; 64 consecutive
    positions with a staged transform) use the same transforms, MFMA order and epilogue: equal bit for bit, on full and
    ragged maps (positions not a multiple of 8), NHWC and k-blocked inputs and outputs."""
    from maskrcnn_amd import ops
    g = torch.Generator().manual_seed(404)
    try:
        for (b, h, w, cin, cout) in ((2, 32, 48, 64, 64), (1, 128, 128, 256, 256), (3, 20, 36, 24, 72), (1, 16, 16, 512, 128)):
            x = torch.randn(b, h, w, cin, generator=g).to(dev)
            wt = (torch.randn(cout, 3, 3, cin, generator=g) * math.sqrt(2.0 / (9 * cin))).to(dev)
            sc, sh = (torch.rand(cout, generator=g) + 0.5).to(dev), (torch.randn(cout, generator=g) * 0.1).to(dev)
            u = ops.winograd_weights(wt)
            xk = ops.nhwc_to_kblocked(x)
            outs = []
            for mode in (1, 0):
                ops.winograd_set_spatial(mode)
                y = ops.conv3x3_winograd(x, u, sc, sh, True)
                outs.append((y, ops.conv3x3_winograd(xk, u, sc, sh, True, out="both" if cout % 8 == 0 else "nhwc")))
            (ys, ks), (yl, kl) = outs
            assert torch.equal(ys, yl), (b, h, w, cin, cout)
            if cout % 8 == 0:
                assert torch.equal(ks[0], kl[0]) and torch.equal(ks[1], kl[1]) and torch.equal(ks[0], ys)
            else:
                assert torch.equal(ks, kl)
    finally:
        ops.winograd_set_spatial(-1)


def test_conv3x3_winograd_bad_arguments(dev):
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import MaskrcnnHipError
    u = ops.winograd_weights(torch.zeros(8, 3, 3, 8, device=dev))
    with pytest.raises(MaskrcnnHipError):
        ops.conv3x3_winograd(torch.zeros(1, 5, 4, 8, device=dev), u, None, None)      # odd height
    u12 = torch.zeros(16, 8, 12, device=dev)
    with pytest.raises(MaskrcnnHipError):
        ops.conv3x3_winograd(torch.zeros(1, 4, 4, 12, device=dev), u12, None, None)   # Cin % 8 != 0
    with pytest.raises(RuntimeError):
        ops.conv3x3_winograd(torch.zeros(1, 4, 4, 8), u.cpu(), None, None)            # CPU tensors


def test_winograd_switch_off_restores_direct_path(dev):
    """MRCNN_WINOGRAD=0 (modules.WINOGRAD False): ConvWeight keeps 3x3 layers on the exact direct kernel."""
    from maskrcnn_amd import modules, ops
    g = torch.Generator().manual_seed(3)
    w = torch.randn(64, 3, 3, 64, generator=g).to(dev) * 0.05
    x = torch.randn(1, 8, 8, 64, generator=g).to(dev)
    saved = modules.WINOGRAD
    try:
        modules.WINOGRAD = False
        cw = modules.ConvWeight(w)
        assert cw.u is None
        assert torch.equal(cw.conv(x, None, None, 1, (1, 1, 1, 1)), ops.conv_bn_act(x, w, None, None, 1, (1, 1, 1, 1)))
        modules.WINOGRAD = True
        cw = modules.ConvWeight(w)
        assert cw.u is not None
        assert torch.equal(cw.conv(x, None, None, 1, (1, 1, 1, 1)), ops.conv3x3_winograd(x, cw.u, None, None))
        # strided / padded-differently / odd-sized calls still take the direct kernel
        assert torch.equal(cw.conv(x, None, None, 2, (0, 1, 0, 1)), ops.conv_bn_act(x, w, None, None, 2, (0, 1, 0, 1)))
    finally:
        modules.WINOGRAD = saved


def test_kblocked_layout_chain(dev):
    """The k-blocked tensors that let Winograd convs chain without a transposition pass: direct conv -> k-blocked,
    Winograd reading k-blocked, Winograd writing NHWC + k-blocked; every path gives the same numbers as NHWC."""
    from maskrcnn_amd import ops
    g = torch.Generator().manual_seed(31)
    b, h, w, c0, c1, c2 = 2, 12, 20, 32, 72, 40
    x = torch.randn(b, h, w, c0, generator=g).to(dev)
    w1 = (torch.randn(c1, 1, 1, c0, generator=g) * 0.2).to(dev)
    w2 = (torch.randn(c2, 3, 3, c1, generator=g) * 0.05).to(dev)
    sh1, sh2 = torch.randn(c1, generator=g).to(dev) * 0.1, torch.randn(c2, generator=g).to(dev) * 0.1
    u2 = ops.winograd_weights(w2)
    y1 = ops.conv_bn_act(x, w1, None, sh1, relu=True)
    y1k = ops.conv_bn_act(x, w1, None, sh1, relu=True, out_kblocked=True)
    assert tuple(y1k.shape) == (c1 // 8, b, h, w, 8)
    assert torch.equal(y1k.permute(1, 2, 3, 0, 4).reshape(b, h, w, c1), y1)          # same values, other layout
    assert torch.equal(ops.nhwc_to_kblocked(y1), y1k)
    ref = ops.conv3x3_winograd(y1, u2, None, sh2, True)
    assert torch.equal(ops.conv3x3_winograd(y1k, u2, None, sh2, True), ref)           # k-blocked input
    yn, yk = ops.conv3x3_winograd(y1k, u2, None, sh2, True, out="both")
    assert torch.equal(yn, ref) and torch.equal(yk.permute(1, 2, 3, 0, 4).reshape(b, h, w, c2), ref)
    assert torch.equal(ops.conv3x3_winograd(y1, u2, None, sh2, True, out="kblocked"), yk)
    # residual + k-blocked output of the direct kernel
    r = torch.randn(b, h, w, c1, generator=g).to(dev)
    a = ops.conv_bn_act(x, w1, None, sh1, relu=True, residual=r)
    ak = ops.conv_bn_act(x, w1, None, sh1, relu=True, residual=r, out_kblocked=True)
    assert torch.equal(ak.permute(1, 2, 3, 0, 4).reshape(b, h, w, c1), a)
    # k-blocked residual, same size and half size (the FPN laterals' nearest-upsample + add)
    rk = ops.nhwc_to_kblocked(r)
    assert torch.equal(ops.conv_bn_act(x, w1, None, sh1, relu=True, residual=rk), a)
    r2 = torch.randn(b, h // 2, w // 2, c1, generator=g).to(dev)
    a2 = ops.conv_bn_act(x, w1, None, sh1, residual=r2, res_div=2)
    a2k = ops.conv_bn_act(x, w1, None, sh1, residual=ops.nhwc_to_kblocked(r2), res_div=2, out_kblocked=True)
    assert torch.equal(a2k.permute(1, 2, 3, 0, 4).reshape(b, h, w, c1), a2)


def test_stem_kernel_vs_generic_and_torch(dev):
    """csrc/stem.hip against the generic implicit-GEMM kernel on the same layer (same fp32 MFMA products; the k order
    inside a tap differs, so equality is to rounding) and against torch CPU (1e-4), incl. ragged tiles and batch > 1."""
    from maskrcnn_amd import ops
    g = torch.Generator().manual_seed(41)
    for (b, h, w) in ((2, 64, 64), (1, 38, 70), (3, 32, 16), (1, 2, 2), (1, 32, 0)):
        if w == 0:   # one row of 16 x 16-output tiles, over the clamp of two workgroups per CU
            w = 32 * _over_the_clamp(per_cu=2)
        x = torch.randn(b, h, w, 4, generator=g)
        x[..., 3] = 0
        wt = torch.randn(64, 7, 7, 4, generator=g) * math.sqrt(2.0 / 147)
        wt[..., 3] = 0
        sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
        y = ops.stem_conv(x.to(dev), wt.to(dev), sc.to(dev), sh.to(dev), True)
        yd = ops.conv_bn_act(x.to(dev), wt.to(dev), sc.to(dev), sh.to(dev), 2, (3, 3, 3, 3), True)
        ref = _ref_conv(x.permute(0, 3, 1, 2), wt.permute(0, 3, 1, 2), sc, sh, 2, (3, 3, 3, 3), True).permute(0, 2, 3, 1)
        assert tuple(y.shape) == (b, h // 2, w // 2, 64)
        assert (y - yd).abs().max().item() <= 2e-5
        assert (y.cpu() - ref).abs().max().item() <= TOL
        # the NCHW form (what the pipeline runs: the molded image itself, no layout pass) is the same computation
        yn = ops.stem_conv(x[..., :3].permute(0, 3, 1, 2).contiguous().to(dev), wt.to(dev), sc.to(dev), sh.to(dev), True, nchw=True)
        assert torch.equal(yn, y)
        # the fp16-output form ("f16" mode): the fp32 result rounded once
        yh = ops.stem_conv(x[..., :3].permute(0, 3, 1, 2).contiguous().to(dev), wt.to(dev), sc.to(dev), sh.to(dev), True, nchw=True,
                           out_f16=True)
        assert yh.dtype == torch.float16 and torch.equal(yh, y.half())
    # the headline shape, against the generic kernel
    x = torch.randint(0, 256, (2, 1024, 1024, 4), generator=g).float() - 120.0
    x[..., 3] = 0
    wt = torch.randn(64, 7, 7, 4, generator=g) * math.sqrt(2.0 / 147)
    wt[..., 3] = 0
    sh = torch.randn(64, generator=g) * 0.1
    y = ops.stem_conv(x.to(dev), wt.to(dev), None, sh.to(dev), True)
    yd = ops.conv_bn_act(x.to(dev), wt.to(dev), None, sh.to(dev), 2, (3, 3, 3, 3), True)
    assert (y - yd).abs().max().item() <= 1e-4 * max(1.0, yd.abs().max().item())
    yn = ops.stem_conv(x[..., :3].permute(0, 3, 1, 2).contiguous().to(dev), wt.to(dev), None, sh.to(dev), True, nchw=True)
    assert torch.equal(yn, y)


# --------------------------------------------------------------------------------------------------
# whole-block fused Bottleneck (csrc/bottleneck.hip): stride-1 identity blocks with planes = 64
# --------------------------------------------------------------------------------------------------
def _identity_block_sd(g, cin=256, planes=64):
    sd = {}
    for name, co, ci, k in (("conv1", planes, cin, 1), ("conv2", planes, planes, 3), ("conv3", 4 * planes, planes, 1)):
        sd[f"{name}.weight"] = torch.randn(co, ci, k, k, generator=g) * math.sqrt(2.0 / (ci * k * k))
        sd[f"{name}.bias"] = torch.randn(co, generator=g) * 0.1
        bn = "bn" + name[-1]
        sd[f"{bn}.weight"] = torch.rand(co, generator=g) + 0.5
        sd[f"{bn}.bias"] = torch.randn(co, generator=g) * 0.1
        sd[f"{bn}.running_mean"] = torch.randn(co, generator=g) * 0.1
        sd[f"{bn}.running_var"] = torch.rand(co, generator=g) + 0.5
    return sd


def _ref_bottleneck(x, sd):
    """Bottleneck.forward (model.py:190-211) in torch-CPU fp32, BN in eval mode (eps 1e-3)."""
    def bn(y, n):
        return F.batch_norm(y, sd[f"{n}.running_mean"], sd[f"{n}.running_var"], sd[f"{n}.weight"], sd[f"{n}.bias"],
                            False, 0.0, 1e-3)
    y = F.relu(bn(F.conv2d(x, sd["conv1.weight"], sd["conv1.bias"]), "bn1"))
    y = F.relu(bn(F.conv2d(F.pad(y, (1, 1, 1, 1)), sd["conv2.weight"], sd["conv2.bias"]), "bn2"))
    y = bn(F.conv2d(y, sd["conv3.weight"], sd["conv3.bias"]), "bn3")
    return F.relu(y + x)


@pytest.mark.parametrize("shape", [(2, 32, 48), (1, 16, 16), (3, 64, 16), (1, 256, 256), (1, 16, 0)],
                         ids=lambda s: "x".join(str(v) for v in s))
def test_bottleneck_fused_whole_block(dev, shape):
    """One launch for conv1 → conv2 → conv3 + residual (C2 identity blocks): bit-identical to the three-launch path
    (same summation orders and transforms), within 1e-4 abs of torch-CPU on unit-scale data, tiles on every image
    border and in the interior, at sizes from one tile to the full C2 resolution of a 1024^2 image."""
    from maskrcnn_amd import modules, ops
    b, h, w = shape
    if w == 0:   # one row of 16 x 16-pixel tiles, over the clamp
        w = 16 * _over_the_clamp()
    g = torch.Generator().manual_seed(900 + h + w)
    sd = _identity_block_sd(g)
    x = torch.randn(b, 256, h, w, generator=g)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    assert ops.bottleneck_fused_supported(h, w, 256, 64)
    saved4 = modules.WINOGRAD4_TRUNK
    try:
        modules.WINOGRAD4_TRUNK = False      # the fused launch holds F(2x2): compare it with the F(2x2) three-launch path
        blk = modules.FusedBottleneck.from_state_dict(sd, "", 1, dev)
        modules.WINOGRAD4_TRUNK = True
        blk4 = modules.FusedBottleneck.from_state_dict(sd, "", 1, dev)
    finally:
        modules.WINOGRAD4_TRUNK = saved4
    c1, c2, c3, cd = blk.convs
    assert cd is None
    fused = ops.bottleneck_fused(xd, c1.w.w, c1.scale, c1.shift, c2.w.u, c2.scale, c2.shift, c3.w.w, c3.scale, c3.shift)
    saved = modules.FUSED_BOTTLENECK
    try:
        modules.FUSED_BOTTLENECK = False
        unfused = blk(xd)
        modules.FUSED_BOTTLENECK = True
        assert torch.equal(blk(xd), fused)                       # the module takes the fused launch
    finally:
        modules.FUSED_BOTTLENECK = saved
    assert torch.equal(fused, unfused), f"max diff {(fused - unfused).abs().max().item():.3e}"
    assert torch.equal(fused, ops.bottleneck_fused(xd, c1.w.w, c1.scale, c1.shift, c2.w.u, c2.scale, c2.shift,
                                                   c3.w.w, c3.scale, c3.shift))          # run to run
    want = _ref_bottleneck(x, sd)
    err = (fused.permute(0, 3, 1, 2).cpu() - want).abs().max().item()
    assert err <= TOL, f"max abs err {err:.3e} (|ref|max {want.abs().max().item():.2f})"
    # the three-launch path with conv2 on the F(4x4) kernel (where the map is large enough) meets the same bar
    saved = modules.FUSED_BOTTLENECK
    try:
        modules.FUSED_BOTTLENECK = False
        got4 = blk4(xd)
    finally:
        modules.FUSED_BOTTLENECK = saved
    err4 = (got4.permute(0, 3, 1, 2).cpu() - want).abs().max().item()
    assert err4 <= TOL, f"F(4x4): max abs err {err4:.3e} (|ref|max {want.abs().max().item():.2f})"
    # the registered op with the reference-shaped argument list is ONE call of the C ABI (mrcnn_bottleneck_forward_f32): by
    # default what the pipeline launches (conv2 from cached Winograd transforms, conv2 + conv3 fused where the map is large
    # enough), the exact direct-kernel composite when Winograd is switched off (it must not slip a Winograd conv2 into the
    # "every conv on the direct kernel" mode), the whole-block launch only when that is switched on
    args = (xd, c1.w.w, c1.scale, c1.shift, c2.w.w, c2.scale, c2.shift, c3.w.w, c3.scale, c3.shift, None, None, None, 1)
    saved_op, saved_w = ops.BOTTLENECK_OP_FUSED, modules.WINOGRAD
    try:
        ops.BOTTLENECK_OP_FUSED = False
        assert torch.equal(torch.ops.maskrcnn.bottleneck_forward(*args), got4)
        assert torch.equal(torch.ops.maskrcnn.bottleneck_forward(*args), got4)           # second call: cached conv2 transforms
        modules.WINOGRAD = False
        y = torch.ops.maskrcnn.bottleneck_forward(*args)
        h1 = ops.conv_bn_act(xd, c1.w.w, c1.scale, c1.shift, relu=True)
        h2 = ops.conv_bn_act(h1, c2.w.w, c2.scale, c2.shift, pad=(1, 1, 1, 1), relu=True)
        direct = ops.conv_bn_act(h2, c3.w.w, c3.scale, c3.shift, relu=True, residual=xd)
        assert torch.equal(y, direct)
        modules.WINOGRAD = saved_w
        ops.BOTTLENECK_OP_FUSED = True
        assert torch.equal(torch.ops.maskrcnn.bottleneck_forward(*args), fused)
        assert torch.equal(torch.ops.maskrcnn.bottleneck_forward(*args), fused)      # second call: cached conv2 transform
    finally:
        ops.BOTTLENECK_OP_FUSED, modules.WINOGRAD = saved_op, saved_w


def _block_sd(g, inplanes, planes, downsample):
    """state dict of one reference Bottleneck (model.py:174-188 names), Xavier-scale weights, non-trivial BN statistics"""
    sd = {}
    def conv(name, co, ci, k):
        sd[name + ".weight"] = torch.randn(co, ci, k, k, generator=g) * math.sqrt(2.0 / (ci * k * k))
        sd[name + ".bias"] = torch.randn(co, generator=g) * 0.1
    def bn(name, c):
        sd[name + ".weight"] = torch.rand(c, generator=g) + 0.5
        sd[name + ".bias"] = torch.randn(c, generator=g) * 0.1
        sd[name + ".running_mean"] = torch.randn(c, generator=g) * 0.1
        sd[name + ".running_var"] = torch.rand(c, generator=g) + 0.5
    conv("conv1", planes, inplanes, 1); bn("bn1", planes)
    conv("conv2", planes, planes, 3); bn("bn2", planes)
    conv("conv3", 4 * planes, planes, 1); bn("bn3", 4 * planes)
    if downsample:
        conv("downsample.0", 4 * planes, inplanes, 1); bn("downsample.1", 4 * planes)
    return sd


# (batch, H, W, inplanes, planes, stride, downsample): the block kinds of ResNet-50/101 (model.py:214-270) on maps that take
# each of the three conv2 kernels — F(4x4) with conv3 fused (C2 size), F(4x4) alone, F(2x2), and odd sizes (direct kernel)
NATIVE_BLOCKS = [
    (2, 64, 64, 64, 64, 1, True),      # C2 block 0: downsample branch, fused conv2 + conv3
    (2, 64, 64, 256, 64, 1, False),    # C2 identity: two launches
    (1, 128, 128, 256, 128, 2, True),  # C3 block 0: stride 2, F(4x4) conv2 (64 x 64 output = 8 tiles)
    (2, 64, 64, 512, 128, 1, False),   # C3 identity, F(4x4)
    (1, 32, 32, 512, 256, 2, True),    # C4 block 0 on a small map: F(2x2)
    (2, 16, 16, 1024, 256, 1, False),  # C4 identity, F(2x2)
    (1, 16, 16, 1024, 512, 2, True),   # C5 block 0
    (1, 8, 8, 2048, 512, 1, False),    # C5 identity
    (1, 14, 10, 256, 64, 1, False),    # H, W not multiples of 4: F(2x2)
    (1, 13, 11, 256, 64, 1, False),    # odd sizes: the direct kernel for conv2
    (1, 13, 11, 64, 64, 2, True),      # odd input, stride 2: 7 x 6 output
]


@pytest.mark.parametrize("blk", NATIVE_BLOCKS, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_bottleneck_native_call_equals_launch_by_launch(dev, blk):
    """mrcnn_bottleneck_forward_f32 (one C call per block: the library plans and enqueues the launches; it backs both
    modules.FusedBottleneck and torch.ops.maskrcnn.bottleneck_forward) gives bit for bit what the same launches give as separate
    binding calls, for every block kind of the trunk and every conv2 kernel, and stays within 1e-4 of the reference module's
    arithmetic in torch-CPU fp32 (model.py:190-211,254-262)."""
    from maskrcnn_amd import modules, ops
    b, h, w, cin, planes, stride, ds = blk
    g = torch.Generator().manual_seed(1000 + h * 7 + cin + planes + stride)
    sd = _block_sd(g, cin, planes, ds)
    x = torch.randn(b, cin, h, w, generator=g)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    m = modules.FusedBottleneck.from_state_dict(sd, "", stride, dev)
    native = m(xd)
    assert torch.equal(native, m.launch_by_launch(xd))
    assert torch.equal(native, m(xd))
    c1, c2, c3, cd = m.convs
    # the plan is the one modules.py's own rules give
    oh, ow = -(-h // stride), -(-w // stride)
    plan = ops.bottleneck_plan(b, h, w, cin, planes, stride, c2.w.u is not None, c2.w.u4 is not None,
                               modules.WINOGRAD4_MIN_TILES, modules.FUSED_CONV3)
    t4 = c2.w.takes_winograd4(oh, ow, 1, (1, 1, 1, 1), None, True, b)
    assert bool(plan & 1) == bool(t4) and bool(plan & 2) == bool(c2.takes_winograd(oh, ow) and not t4)
    assert bool(plan & 4) == bool(t4 and planes == 64 and modules.FUSED_CONV3)
    # the torch op with the reference-shaped argument list (raw conv2 weight: transforms cached per weight tensor)
    args = (xd, c1.w.w, c1.scale, c1.shift, c2.w.w, c2.scale, c2.shift, c3.w.w, c3.scale, c3.shift,
            None if cd is None else cd.w.w, None if cd is None else cd.scale, None if cd is None else cd.shift, stride)
    assert torch.equal(torch.ops.maskrcnn.bottleneck_forward(*args), native)
    # the reference arithmetic
    def bn(y, n):
        return F.batch_norm(y, sd[f"{n}.running_mean"], sd[f"{n}.running_var"], sd[f"{n}.weight"], sd[f"{n}.bias"], False, 0.0, 1e-3)
    r = F.relu(bn(F.conv2d(x, sd["conv1.weight"], sd["conv1.bias"], stride=stride), "bn1"))
    r = F.relu(bn(F.conv2d(F.pad(r, (1, 1, 1, 1)), sd["conv2.weight"], sd["conv2.bias"]), "bn2"))
    r = bn(F.conv2d(r, sd["conv3.weight"], sd["conv3.bias"]), "bn3")
    res = bn(F.conv2d(x, sd["downsample.0.weight"], sd["downsample.0.bias"], stride=stride), "downsample.1") if ds else x
    want = F.relu(r + res)
    err = (native.permute(0, 3, 1, 2).cpu() - want).abs().max().item()
    assert err <= TOL, f"max abs err {err:.3e} (|ref|max {want.abs().max().item():.2f})"
    # a workspace that is too small is refused, not overrun
    with pytest.raises(RuntimeError, match="workspace"):
        import ctypes
        from maskrcnn_amd._lib import check, lib
        ptrs = (ctypes.c_void_p * 14)(*[None if t is None else t.data_ptr() for t in
                                        (c1.w.w, c1.scale, c1.shift, c2.w.w, c2.w.u, c2.w.u4, c2.scale, c2.shift, c3.w.w, c3.scale,
                                         c3.shift, None if cd is None else cd.w.w, None if cd is None else cd.scale,
                                         None if cd is None else cd.shift)])
        ws = torch.empty(256, dtype=torch.uint8, device=dev)
        check(lib.mrcnn_bottleneck_forward_f32(xd.data_ptr(), b, h, w, cin, planes, stride, ptrs, 8, 1, ws.data_ptr(), 256,
                                               native.data_ptr(), torch.cuda.current_stream().cuda_stream))


# (batch, H, W, first block?): the C2 stage in the plain-fp16 mode — one launch per block (csrc/bottleneck_f16.hip)
F16_C2_BLOCKS = [(2, 64, 64, False), (2, 64, 64, True), (1, 8, 16, False), (1, 8, 16, True), (3, 21, 37, False), (3, 21, 37, True),
                 (1, 5, 3, False), (2, 208, 336, False), (2, 208, 336, True), (1, 8, 0, False)]


@pytest.mark.parametrize("blk", F16_C2_BLOCKS, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_bottleneck_c2_f16_one_launch(dev, blk):
    """The ResNet C2 block of the "f16" mode as ONE launch (mrcnn_bottleneck_c2_f16; model.py:190-211, residual :254-262)
    against (a) the per-layer fp16 launches it replaces — same fp16 operands, both intermediates rounded to fp16 at the same
    places: the two may differ where an fp32 sum lands within an fp16 rounding boundary (another MFMA shape sums in another order),
    i.e. by one fp16 ulp on a few elements: asserted <= 2 fp16 ulps of the output range and <= 0.5 % of the elements differing —,
    (b) the reference module's arithmetic in torch-CPU fp32 at the fp16 mode's bar (2e-2 of the range), and (c) itself: image i of
    a batch == image i alone, a repeat == bit for bit. Ragged tiles (8 x 16 pixels), one-tile and sub-tile maps, configs[4]'s size."""
    from maskrcnn_amd import modules, ops
    b, h, w, first = blk
    if w == 0:   # one row of 8 x 16-pixel tiles, over the clamp
        w = 16 * _over_the_clamp()
    cin = 64 if first else 256
    g = torch.Generator().manual_seed(2000 + h * 7 + w + cin)
    sd = _block_sd(g, cin, 64, first)
    x = torch.randn(b, cin, h, w, generator=g).half()
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    m = modules.FusedBottleneck.from_state_dict(sd, "", 1, dev, "f16")
    assert m.f16_block is not None and ops.bottleneck_c2_f16_supported(b, h, w, cin, 64, first)
    got = m(xd)
    assert got.dtype == torch.float16 and tuple(got.shape) == (b, h, w, 256)
    assert torch.equal(got, m(xd))
    for i in range(b):
        assert torch.equal(m(xd[i:i + 1].contiguous())[0], got[i]), i
    per_layer = m.launch_by_launch(xd)
    rng = per_layer.float().abs().max().item()
    ulp = 2.0 ** (math.floor(math.log2(rng)) - 10)                     # fp16 spacing at the top of the range
    diff = (got.float() - per_layer.float()).abs()
    assert diff.max().item() <= 2 * ulp, (diff.max().item(), ulp)
    assert (diff > 0).float().mean().item() <= 5e-3
    # the reference arithmetic (fp32, on the fp16-rounded input)
    xf = x.float()
    def bn(y, n):
        return F.batch_norm(y, sd[f"{n}.running_mean"], sd[f"{n}.running_var"], sd[f"{n}.weight"], sd[f"{n}.bias"], False, 0.0, 1e-3)
    r = F.relu(bn(F.conv2d(xf, sd["conv1.weight"], sd["conv1.bias"]), "bn1"))
    r = F.relu(bn(F.conv2d(F.pad(r, (1, 1, 1, 1)), sd["conv2.weight"], sd["conv2.bias"]), "bn2"))
    r = bn(F.conv2d(r, sd["conv3.weight"], sd["conv3.bias"]), "bn3")
    res = bn(F.conv2d(xf, sd["downsample.0.weight"], sd["downsample.0.bias"]), "downsample.1") if first else xf
    want = F.relu(r + res)
    err = (got.float().permute(0, 3, 1, 2).cpu() - want).abs().max().item()
    assert err <= 2e-2 * want.abs().max().item(), (err, want.abs().max().item())


def test_bottleneck_c2_f16_rejects_other_blocks(dev):
    from maskrcnn_amd import modules, ops
    assert not ops.bottleneck_c2_f16_supported(1, 64, 64, 512, 128, False)      # C3: planes 128
    assert not ops.bottleneck_c2_f16_supported(1, 64, 64, 64, 64, False)        # Cin 64 without the downsample branch
    assert not ops.bottleneck_c2_f16_supported(1, 64, 64, 256, 64, True)
    assert not ops.bottleneck_c2_f16_supported(64, 1024, 1024, 256, 64, False)  # past the 32-bit offsets
    g = torch.Generator().manual_seed(7)
    assert modules.FusedBottleneck.from_state_dict(_block_sd(g, 512, 128, False), "", 1, dev, "f16").f16_block is None
    assert modules.FusedBottleneck.from_state_dict(_block_sd(g, 256, 64, False), "", 1, dev, "f32").f16_block is None
    m = modules.FusedBottleneck.from_state_dict(_block_sd(g, 256, 64, False), "", 1, dev, "f16")
    f1, f2, f3, _ = m.f16_block
    c1, c2, c3, _ = m.convs
    with pytest.raises(RuntimeError, match="fragments"):
        ops.bottleneck_c2_f16(torch.zeros(1, 8, 8, 64, dtype=torch.float16, device=dev), f1, c1.scale, c1.shift, f2, c2.scale,
                              c2.shift, f3, c3.scale, c3.shift)


@pytest.mark.parametrize("shape", [(3, 14, 14, 81), (1, 5, 3, 81), (400, 14, 14, 81), (7, 14, 14, 2), (2, 9, 14, 96),
                                   (0, 16, 16, 81)], ids=lambda s: "x".join(str(v) for v in s))
def test_mask_tail_f16_one_launch(dev, shape):
    """The "f16" mode's mask-head tail — deconv 2x2 s2 + bias + ReLU -> conv5 1x1 + bias -> sigmoid (model.py:906-914) — as ONE
    launch (mrcnn_mask_tail_f16: the deconv's fp16 map is conv5's MFMA operand in registers) against (a) the two launches it
    replaces on the same fp16 operands (they round the same values to fp16 at the same place; another MFMA shape sums in another
    order, so a few deconv values land one fp16 ulp apart: <= 2e-3 abs on the sigmoid outputs), (b) torch-CPU fp32 on the
    fp16-rounded operands at the mode's mask bar (3e-2 abs), (c) itself: RoI i of a batch == RoI i alone, repeats bit for bit.
    Ragged pixel sets (256 pixels per work item), 400 RoIs (configs[4]), 2 and 96 classes (the store tails)."""
    from maskrcnn_amd import modules, ops
    r, h, w, classes = shape
    if r == 0:   # a RoI of 16 x 16 pixels is one set of 256 pixels, four work items: over the clamp
        r = _over_the_clamp(multiple_of=4) // 4
    g = torch.Generator().manual_seed(3000 + r + classes)
    xi = torch.randn(r, 256, h, w, generator=g).half()
    wt = torch.randn(256, 256, 2, 2, generator=g) * math.sqrt(2.0 / 256)     # [Cin, Cout, 2, 2]
    bde = torch.randn(256, generator=g) * 0.1
    w5 = torch.randn(classes, 256, 1, 1, generator=g) * math.sqrt(2.0 / 256)
    b5 = torch.randn(classes, generator=g) * 0.1
    x = xi.permute(0, 2, 3, 1).contiguous().to(dev)
    w4 = wt.permute(2, 3, 1, 0).reshape(4 * 256, 1, 1, 256).contiguous().to(dev)
    w4_hi, _ = ops.split_f16(w4)
    w5_hi, _ = ops.split_f16(w5.permute(0, 2, 3, 1).contiguous().to(dev))
    b4, b5d = bde.repeat(4).contiguous().to(dev), b5.to(dev)
    w5p = torch.cat([w5_hi.reshape(classes, 256), w5_hi.new_zeros(96 - classes, 256)], 0).contiguous()
    fde, f5 = ops.pack_afrags_f16(w4_hi), ops.pack_afrags_f16(w5p)
    assert ops.mask_tail_f16_supported(r, h, w, 256, 256, classes)
    got = ops.mask_tail_f16(x, fde, b4, f5, b5d)
    assert got.dtype == torch.float32 and tuple(got.shape) == (r, 2 * h, 2 * w, classes)
    assert torch.equal(got, ops.mask_tail_f16(x, fde, b4, f5, b5d))
    for i in (0, r - 1):
        assert torch.equal(ops.mask_tail_f16(x[i:i + 1].contiguous(), fde, b4, f5, b5d)[0], got[i]), i
    # the two launches
    y = ops.deconv2x2(x, (w4_hi, None), b4, 1, 1)
    two = ops.conv_bn_act_f16mfma(y, w5_hi, None, None, b5d, 1, (0, 0, 0, 0), 2, None, 1, products=1, out_f16=False)
    assert (got - two).abs().max().item() <= 2e-3
    # the reference arithmetic
    want = torch.sigmoid(F.conv2d(F.relu(F.conv_transpose2d(xi.float(), wt.half().float(), bde, stride=2)), w5.half().float(), b5))
    assert (got.permute(0, 3, 1, 2).cpu() - want).abs().max().item() <= 3e-2


def test_mask_tail_f16_rejects_other_shapes(dev):
    from maskrcnn_amd import ops
    assert not ops.mask_tail_f16_supported(4, 14, 14, 128, 256, 81)
    assert not ops.mask_tail_f16_supported(4, 14, 14, 256, 128, 81)
    assert not ops.mask_tail_f16_supported(4, 14, 14, 256, 256, 97)
    assert not ops.mask_tail_f16_supported(30000, 14, 14, 256, 256, 81)     # past the 32-bit offsets


def test_bottleneck_fused_rejects_other_shapes(dev):
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import MaskrcnnHipError
    assert not ops.bottleneck_fused_supported(128, 128, 512, 128)     # C3: planes 128
    assert not ops.bottleneck_fused_supported(24, 16, 256, 64)        # H % 16 != 0
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(MaskrcnnHipError):
        ops.bottleneck_fused(z(1, 24, 16, 256), z(64, 1, 1, 256), None, None, z(16, 64, 64), None, None,
                             z(256, 1, 1, 64), None, None)


# --------------------------------------------------------------------------------------------------
# RPN heads inside the Winograd kernel (conv3x3_wino8s_f32<heads>)
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 16, 16, 64, 128), (2, 32, 48, 256, 512), (3, 14, 18, 32, 64), (1, 128, 128, 256, 512),
                                   (1, 16, 0, 8, 64)], ids=lambda s: "x".join(str(v) for v in s))
def test_winograd_fused_rpn_heads(dev, shape):
    from maskrcnn_amd import ops as _ops
    if shape[2] == 0:   # one row of 8 x 8-position blocks, over the clamp
        shape = (shape[0], shape[1], 16 * _over_the_clamp()) + shape[3:]
    if min(shape[1], shape[2]) < 16:
        # maps under 8 x 8 tile positions have no spatial tiles, and the heads exist in the spatial-tile kernel only
        xk = torch.zeros(shape[3] // 8, shape[0], shape[1], shape[2], 8, device=dev)
        u = _ops.winograd_weights(torch.zeros(shape[4], 3, 3, shape[3], device=dev))
        with pytest.raises(RuntimeError, match=r"at least 16 x 16 pixels .* \(tile_mode 2\) are required"):
            _ops.conv3x3_winograd_heads(xk, u, None, None, torch.zeros(32, shape[4], device=dev), True)
        return
    _winograd_fused_rpn_heads(dev, shape)


def _winograd_fused_rpn_heads(dev, shape):
    """RPN.forward on one level (model.py:609-649) with the heads inside the Winograd kernel: relu(conv_shared) is
    never stored; the head sums come back in position-major order. Against torch-CPU (1e-4 abs, unit-scale data) and
    against the unfused path (Winograd conv + 18-channel 1x1 conv), incl. ragged last M tiles and several N tiles."""
    from maskrcnn_amd import ops
    b, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(300 + h + cin)
    x = torch.randn(b, cin, h, w, generator=g)
    ws = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
    bs = torch.randn(cout, generator=g) * 0.1
    wh = torch.randn(18, cout, 1, 1, generator=g) * math.sqrt(1.0 / cout)
    bh = torch.randn(18, generator=g) * 0.1
    shared = F.relu(F.conv2d(x, ws, bs, padding=1))
    want = F.conv2d(shared, wh, bh).permute(0, 2, 3, 1)
    xk = ops.nhwc_to_kblocked(x.permute(0, 2, 3, 1).contiguous().to(dev))
    u = ops.winograd_weights(ws.permute(0, 2, 3, 1).contiguous().to(dev))
    w32 = torch.zeros(32, cout)
    w32[:18] = wh.view(18, cout)
    sums = ops.conv3x3_winograd_heads(xk, u, None, bs.to(dev), w32.to(dev), True)
    assert sums.tile_mode == 2
    got = sums.to_nhwc(bh.to(dev)).cpu()
    err = (got - want).abs().max().item()
    assert err <= TOL, f"max abs err {err:.3e} (|ref|max {want.abs().max().item():.2f})"
    # the unfused path on the same inputs (different summation grouping over the 512 channels: not bit-identical)
    y = ops.conv3x3_winograd(xk, u, None, bs.to(dev), True)
    un = ops.conv_bn_act(y, wh.permute(0, 2, 3, 1).contiguous().to(dev), None, bh.to(dev)).cpu()
    assert (got - un).abs().max().item() <= 2e-5
    again = ops.conv3x3_winograd_heads(xk, u, None, bs.to(dev), w32.to(dev), True)
    assert torch.equal(again.to_nhwc(bh.to(dev)).cpu(), got)                          # deterministic
    # the consumer: scores / deltas from head sums == from NHWC heads of the same values
    lv = [got.to(dev)] + [torch.randn(b, max(h >> i, 1), max(w >> i, 1), 18, generator=g).to(dev) for i in (1, 2, 3, 4)]
    s0, d0 = ops.rpn_scores_deltas(lv)
    s1, d1 = ops.rpn_scores_deltas([sums] + lv[1:], bh.to(dev))
    assert torch.equal(s0, s1) and torch.equal(d0, d1)


# --------------------------------------------------------------------------------------------------
# fp16 ACTIVATIONS in HBM (plain-fp16 mode, BASELINE config 5's "fp16 MFMA path")
# --------------------------------------------------------------------------------------------------
def test_conv_f16_pipelined_full_size_layers_repeat_bitwise(dev):
    """Race screen for the counted-vmcnt / raw-barrier pipeline: configs[4]-size layers (every CU busy, several tiles per CU,
    one tile per CU, long K), each run six times — every run equals the 128 x 128 tile kernel's result bit for bit."""
    from maskrcnn_amd import ops
    g = torch.Generator().manual_seed(5)
    shapes = [  # (B, H, W, Cin, Cout, k, residual)
        (8, 104, 168, 256, 512, 3, False),   # RPN shared conv on P3: 5 tiles per CU
        (8, 52, 84, 256, 256, 3, False),     # C4 conv2: one 160-row tile per CU
        (8, 52, 84, 256, 1024, 1, True),     # C4 conv3: short K + residual
        (1, 80, 100, 12544, 1024, 1, False), # classifier GEMM: 196 k tiles
    ]
    for b, h, w, cin, cout, k, res in shapes:
        x = torch.randn(b, h, w, cin, generator=g).half().to(dev)
        wt = (torch.randn(cout, k, k, cin, generator=g) * math.sqrt(2.0 / (cin * k * k))).half().to(dev)
        r = torch.randn(b, h, w, cout, generator=g).half().to(dev) if res else None
        pad = (1, 1, 1, 1) if k == 3 else (0, 0, 0, 0)
        ref = ops.conv_bn_act_f16mfma(x, wt, None, None, None, 1, pad, True, r, 1, products=1, out_f16=True)
        for _ in range(6):
            got = ops.conv_f16_pipelined(x, wt, None, None, pad, True, r)
            assert torch.equal(got, ref), (b, h, w, cin, cout, k)


@pytest.mark.parametrize("shape", [(1, 16, 16, 64, 0), (2, 26, 22, 256, 0), (1, 40, 56, 256, 160), (3, 32, 48, 128, 256)],
                         ids=lambda c: "x".join(str(v) for v in c))
def test_conv_f16_pipelined_heads_vs_two_launches(dev, shape):
    """The RPN's shared conv with both 1x1 heads inside the pipelined fp16 kernel against the two launches it replaces (the
    fp16 shared activation, then the 18-channel head conv on fp16 operands): the same fp16 activation values meet the same
    fp16 head weights, only the fp32 summation is grouped differently (per 64 channels, then four partials, then two planes).
    Also through the consumer: scores / deltas from the head sums == from the NHWC heads to that tolerance, and the result
    does not depend on the tile height or on the batch (image i alone == slice i)."""
    from maskrcnn_amd import ops
    b, h, w, cin, rows = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(b, h, w, cin, generator=g).half().to(dev)
    wt = (torch.randn(512, 3, 3, cin, generator=g) * math.sqrt(2.0 / (9 * cin))).half().to(dev)
    sc, sh = (torch.rand(512, generator=g) + 0.5).to(dev), (torch.randn(512, generator=g) * 0.1).to(dev)
    wh = torch.randn(18, 512, generator=g) * math.sqrt(1.0 / 512)
    bh = (torch.randn(18, generator=g) * 0.1).to(dev)
    wh32 = torch.zeros(32, 512)
    wh32[:18] = wh
    wh16 = wh32.half().to(dev)
    fused = ops.conv_f16_pipelined_heads(x, wt, sc, sh, wh16, (1, 1, 1, 1), True, tile_rows=rows)
    assert fused.tile_mode == 4 and tuple(fused.part.shape) == (2, b * h * w, 32)
    got = fused.to_nhwc(bh)
    shared = ops.conv_f16_pipelined(x, wt, sc, sh, (1, 1, 1, 1), True)                       # fp16 activation
    want = ops.conv_bn_act_f16mfma(shared, wh.half().view(18, 1, 1, 512).contiguous().to(dev), None, None, bh, 1,
                                   (0, 0, 0, 0), False, None, 1, products=1, out_f16=False)
    scale = max(1.0, want.abs().max().item())
    assert (got - want).abs().max().item() <= 2e-5 * scale, (got - want).abs().max().item()
    assert torch.equal(fused.part[:, :, 18:], torch.zeros_like(fused.part[:, :, 18:]))       # the padded head columns
    # tile height and batch do not change a bit
    for r2 in (128, 192):
        assert torch.equal(ops.conv_f16_pipelined_heads(x, wt, sc, sh, wh16, (1, 1, 1, 1), True, tile_rows=r2).part, fused.part)
    one = ops.conv_f16_pipelined_heads(x[b - 1:].contiguous(), wt, sc, sh, wh16, (1, 1, 1, 1), True)
    assert torch.equal(one.part, fused.part[:, (b - 1) * h * w:])
    # the consumer
    lv = [torch.randn(b, max(h >> i, 1), max(w >> i, 1), 18, generator=g).to(dev) for i in (1, 2, 3, 4)]
    s0, d0 = ops.rpn_scores_deltas([got] + lv)
    s1, d1 = ops.rpn_scores_deltas([fused] + lv, bh)
    assert torch.equal(s0, s1) and torch.equal(d0, d1)


F16IO_CASES = [
    # (B, H, W, Cin, Cout, k, stride, relu, residual(0/1/2), x16, y16)
    (2, 16, 16, 64, 64, 1, 1, True, 0, True, True),
    (2, 16, 16, 64, 256, 1, 1, True, 1, True, True),      # bottleneck conv3 + fp16 residual
    (2, 16, 16, 256, 128, 1, 2, True, 0, True, True),     # stride 2
    (1, 16, 16, 64, 64, 3, 1, True, 0, True, True),       # 3x3
    (2, 16, 16, 1024, 256, 1, 1, False, 2, True, True),   # FPN lateral + half-size fp16 residual
    (1, 32, 32, 256, 256, 3, 1, False, 0, True, False),   # FPN smoothing: fp16 in, fp32 out
    (1, 16, 16, 256, 512, 3, 1, True, 0, False, True),    # RPN shared: fp32 in, fp16 out
    (1, 16, 16, 512, 18, 1, 1, False, 0, True, False),    # RPN heads: fp16 in, fp32 out
    (2, 64, 64, 8, 64, 7, 2, True, 0, False, True),       # stem (generic K), fp32 in, fp16 out
    (37, 1, 1, 12544, 1024, 1, 1, True, 0, False, True),  # classifier conv1 as GEMM
    (3, 13, 11, 32, 48, 3, 1, True, 1, True, True),       # ragged
]


F16P_CASES = [
    # (B, H, W, Cin, Cout, k, stride, pad, relu, residual(0/1/2), out16, out32, tile_rows, tile_cols)
    (1, 16, 16, 64, 256, 1, 1, (0, 0, 0, 0), True, 0, True, False, 0, 0),      # one k tile, M = one tile (auto: 128 x 128)
    (1, 16, 16, 128, 256, 1, 1, (0, 0, 0, 0), True, 1, True, False, 128, 256), # two k tiles + fp16 residual
    (2, 13, 11, 64, 256, 3, 1, (1, 1, 1, 1), True, 0, True, True, 160, 256),   # ragged M (286), both outputs, 9 taps
    (1, 24, 40, 192, 512, 3, 1, (1, 1, 1, 1), False, 0, False, True, 192, 256),  # odd k-tile count (27), two N tiles, fp32 only
    (2, 32, 32, 256, 256, 3, 1, (1, 1, 1, 1), True, 0, True, False, 256, 256), # FPN-smoothing shape, 8 M tiles
    (3, 20, 28, 256, 1024, 1, 1, (0, 0, 0, 0), True, 1, True, False, 0, 0),    # bottleneck conv3 shape (K = 256: auto 128 x 128)
    (3, 20, 28, 256, 1024, 1, 1, (0, 0, 0, 0), True, 1, True, False, 192, 256),  # the same on the large tile
    (1, 9, 7, 64, 256, 3, 1, (0, 0, 1, 1), False, 0, True, False, 0, 0),       # asymmetric SAME pad (0,0,1,1)
    (1, 12, 12, 64, 256, 5, 1, (2, 2, 2, 2), False, 0, True, False, 0, 0),     # 25 taps
    (70, 1, 1, 3136, 1024, 1, 1, (0, 0, 0, 0), True, 0, True, False, 0, 0),    # GEMM (classifier shape, K = 49 k tiles)
    (2, 26, 22, 256, 128, 1, 2, (0, 0, 0, 0), True, 0, True, False, 0, 0),     # stride 2 (C3 conv1 of a first block), 128 columns
    (2, 26, 22, 256, 512, 1, 2, (0, 0, 0, 0), False, 0, True, False, 0, 0),    # stride-2 downsample
    (1, 17, 15, 64, 64, 3, 1, (1, 1, 1, 1), True, 0, True, False, 0, 0),       # C2 conv2: 64 columns (8-byte stores)
    (2, 12, 20, 128, 128, 3, 1, (1, 1, 1, 1), True, 0, True, False, 256, 128), # C3 conv2 on the 256 x 128 tile
    (2, 12, 20, 128, 64, 1, 1, (0, 0, 0, 0), True, 1, True, True, 256, 64),    # 256 x 64 tile, residual, both outputs
    (2, 16, 24, 512, 256, 1, 1, (0, 0, 0, 0), False, 2, True, False, 0, 0),    # FPN lateral + half-size residual
    (1, 9, 7, 64, 128, 3, 2, (0, 0, 1, 1), True, 0, False, True, 0, 0),        # 3x3 stride 2 with SAME pad (0,0,1,1)
]


@pytest.mark.parametrize("case", F16P_CASES, ids=lambda c: "x".join(str(v) for v in c[:7]) + f"_t{c[-2]}x{c[-1]}")
def test_conv_f16_pipelined_vs_torch_cpu(dev, case):
    """csrc/conv_f16p.hip (eight waves, LDS-DMA across barriers) against an fp32 torch-CPU conv of the fp16-ROUNDED operands:
    same bar as the fp16-storage kernel below (summation order + one rounding to fp16 for an fp16 output). Every tile shape,
    odd / even k-tile counts, padding taps, strides, ragged M, several N tiles, both residual forms, both output types, and
    equality of the two outputs up to the fp16 rounding when both are written."""
    from maskrcnn_amd import ops
    b, h, w, cin, cout, k, stride, pad, relu, res, o16, o32, rows, cols = case
    g = torch.Generator().manual_seed(sum(int(v) for v in case[:7]) + rows + cols)
    x = torch.randn(b, cin, h, w, generator=g).half()
    wt = (torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))).half()
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.1
    oh, ow = (h + pad[0] + pad[2] - k) // stride + 1, (w + pad[1] + pad[3] - k) // stride + 1
    residual = torch.randn(b, cout, oh // res, ow // res, generator=g).half() if res else None
    want = _ref_conv(x.float(), wt.float(), scale, shift, stride, pad, relu, None if residual is None else residual.float(),
                     max(res, 1))
    to_nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev)
    assert ops.conv_f16_pipelined_supported(b, h, w, cin, cout, k, k, pad, stride)
    got = ops.conv_f16_pipelined(to_nhwc(x), to_nhwc(wt), scale.to(dev), shift.to(dev), pad, relu,
                                 None if residual is None else to_nhwc(residual), out_f16=o16, out_f32=o32, tile_rows=rows,
                                 stride=stride, res_div=max(res, 1), tile_cols=cols)
    outs = got if isinstance(got, tuple) else (got,)
    for y in outs:
        y16 = y.dtype == torch.float16
        yc = y.float().permute(0, 3, 1, 2).cpu()
        tol = 2e-4 + (2.0 ** -11) * want.abs() if y16 else torch.full_like(want, 2e-4)
        bad = ((yc - want).abs() > tol).sum().item()
        assert bad == 0, f"{bad} elements off ({y.dtype}); max abs err {(yc - want).abs().max().item():.3e}"
    if len(outs) == 2:  # the fp16 output is the fp32 output rounded once
        assert torch.equal(outs[0], outs[1].half())
    # unsupported shapes are refused, not mis-computed
    assert not ops.conv_f16_pipelined_supported(b, h, w, cin + 32, cout, k, k, pad, stride)
    assert not ops.conv_f16_pipelined_supported(b, h, w, cin, cout + 32, k, k, pad, stride)


def test_conv_f16_pipelined_equals_the_tile_kernel_bitwise(dev):
    """Same fp16 operands, same k order per output element, fp32 accumulation on both: the pipelined kernel and conv_igemm_f16
    agree bit for bit (the 'f16' mode gives the same numbers with MRCNN_F16_PIPELINED=0), on every tile shape."""
    from maskrcnn_amd import ops
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, 24, 20, 128, generator=g).half().to(dev)
    r = torch.randn(2, 24, 20, 256, generator=g).half().to(dev)
    for k, pad in ((1, (0, 0, 0, 0)), (3, (1, 1, 1, 1))):
        wt = (torch.randn(256, k, k, 128, generator=g) * math.sqrt(2.0 / (128 * k * k))).half().to(dev)
        sc, sh = (torch.rand(256, generator=g) + 0.5).to(dev), (torch.randn(256, generator=g) * 0.1).to(dev)
        ref = ops.conv_bn_act_f16mfma(x, wt, None, sc, sh, 1, pad, True, r, 1, products=1, out_f16=True)
        for rows, cols in ((128, 256), (160, 256), (192, 256), (256, 256), (128, 128), (256, 128), (128, 64), (256, 64)):
            got = ops.conv_f16_pipelined(x, wt, sc, sh, pad, True, r, tile_rows=rows, tile_cols=cols)
            assert torch.equal(got, ref), (k, rows, cols)


@pytest.mark.parametrize("case", F16IO_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_conv_f16_activations_vs_torch_cpu(dev, case):
    """The reference computes in fp32; the fp16-storage path is held to fp16's own resolution: against an fp32 torch-CPU
    conv of the fp16-ROUNDED operands (exact products, fp32 sums) the result may differ by the summation order plus, for
    an fp16 output, one rounding to 11 significand bits (2^-11 relative)."""
    from maskrcnn_amd import ops
    b, h, w, cin, cout, k, stride, relu, res, x16, y16 = case
    g = torch.Generator().manual_seed(sum(int(v) for v in case))
    pad = (3, 3, 3, 3) if k == 7 else (1, 1, 1, 1) if k == 3 else (0, 0, 0, 0)
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.1
    oh = (h + pad[0] + pad[2] - k) // stride + 1
    ow = (w + pad[1] + pad[3] - k) // stride + 1
    residual = torch.randn(b, cout, oh // max(res, 1), ow // max(res, 1), generator=g).half() if res else None
    want = _ref_conv(x.half().float(), wt.half().float(), scale, shift, stride, pad, relu,
                     None if residual is None else residual.float(), max(res, 1))
    to_nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev)
    xd = to_nhwc(x.half() if x16 else x)
    w_hi, _ = ops.split_f16(to_nhwc(wt))
    got = ops.conv_bn_act_f16mfma(xd, w_hi, None, scale.to(dev), shift.to(dev), stride, pad, relu,
                                  None if residual is None else to_nhwc(residual), max(res, 1), products=1, out_f16=y16)
    assert got.dtype == (torch.float16 if y16 else torch.float32)
    got = got.float().permute(0, 3, 1, 2).cpu()
    tol = 2e-4 + (2.0 ** -11) * want.abs() if y16 else torch.full_like(want, 2e-4)
    bad = ((got - want).abs() > tol).sum().item()
    assert bad == 0, f"{bad} elements off; max abs err {(got - want).abs().max().item():.3e}"


def test_maxpool_and_deconv_f16(dev):
    from maskrcnn_amd import ops
    g = torch.Generator().manual_seed(17)
    x = torch.randn(2, 13, 10, 64, generator=g).half().to(dev)
    for kern, stride, pad in ((3, 2, (0, 0, 1, 1)), (1, 2, (0, 0, 0, 0))):
        assert torch.equal(ops.maxpool(x, kern, stride, pad), ops.maxpool(x.float(), kern, stride, pad).half())
    # 2x2 stride-2 transposed conv, fp16 in/out, against torch-CPU on the rounded operands
    xi = torch.randn(3, 32, 7, 7, generator=g)
    wt = torch.randn(32, 64, 2, 2, generator=g) * 0.1      # [Cin, Cout, 2, 2]
    bias = torch.randn(64, generator=g) * 0.1
    want = F.relu(F.conv_transpose2d(xi.half().float(), wt.half().float(), bias, stride=2))
    w4 = wt.permute(2, 3, 1, 0).reshape(4 * 64, 1, 1, 32).contiguous().to(dev)
    w_hi, _ = ops.split_f16(w4)
    y = ops.deconv2x2(xi.half().permute(0, 2, 3, 1).contiguous().to(dev), (w_hi, None), bias.repeat(4).to(dev), 1, 1)
    assert y.dtype == torch.float16 and tuple(y.shape) == (3, 14, 14, 64)
    err = (y.float().permute(0, 3, 1, 2).cpu() - want).abs()
    assert bool((err <= 2e-4 + 2.0 ** -11 * want.abs()).all()), err.max().item()


def test_deconv_scatter_ragged_tiles_keep_their_guard_bands(dev):
    """The 2x2 transposed-conv epilogue stores 8-byte channel pairs through a buffer descriptor and drops out-of-range rows /
    channels by pushing their offset past the descriptor's range (conv_common.hpp oob_add). Tiles ragged in BOTH M (105 and
    78400 input pixels: not multiples of 128) and N (4 * 24 = 96 and 4 * 6 = 24 columns of a 128-wide tile), called through
    the C ABI on an output that sits between guard bands: the result equals torch-CPU and no byte of either band changes —
    a dropped store whose offset + 8 wrapped would land inside the buffer or the band."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import check, lib
    g = torch.Generator().manual_seed(171)
    for (b, h, w, cin, cout, f16) in ((3, 5, 7, 32, 24, False), (1, 7, 15, 16, 6, False), (3, 5, 7, 32, 24, True),
                                      (400, 14, 14, 8, 6, False)):
        xi = torch.randn(b, cin, h, w, generator=g)
        wt = torch.randn(cin, cout, 2, 2, generator=g) * 0.2
        bias = torch.randn(cout, generator=g) * 0.1
        w4 = wt.permute(2, 3, 1, 0).reshape(4 * cout, 1, 1, cin).contiguous().to(dev)
        b4 = bias.repeat(4).contiguous().to(dev)
        n_out = b * 2 * h * 2 * w * cout
        band = 4096
        if f16:
            x = xi.half().permute(0, 2, 3, 1).contiguous().to(dev)
            w_hi, _ = ops.split_f16(w4)
            buf = torch.full((n_out + 2 * band,), 7.0, dtype=torch.float16, device=dev)
            y = buf[band:band + n_out]
            check(lib.mrcnn_deconv2x2_bias_act_nhwc_f16io(x.data_ptr(), b, h, w, cin, w_hi.data_ptr(), cout, b4.data_ptr(), 1,
                                                          y.data_ptr(), torch.cuda.current_stream().cuda_stream))
            want = F.relu(F.conv_transpose2d(xi.half().float(), wt.half().float(), bias, stride=2))
            tol = 2e-4 + 2.0 ** -11 * want.abs()
        else:
            x = xi.permute(0, 2, 3, 1).contiguous().to(dev)
            buf = torch.full((n_out + 2 * band,), 7.0, dtype=torch.float32, device=dev)
            y = buf[band:band + n_out]
            check(lib.mrcnn_deconv2x2_bias_act_nhwc_f32(x.data_ptr(), b, h, w, cin, w4.data_ptr(), cout, b4.data_ptr(), 1,
                                                        y.data_ptr(), torch.cuda.current_stream().cuda_stream))
            want = F.relu(F.conv_transpose2d(xi, wt, bias, stride=2))
            tol = torch.full_like(want, 1e-4)
        torch.cuda.synchronize()
        got = y.view(b, 2 * h, 2 * w, cout).float().permute(0, 3, 1, 2).cpu()
        assert bool(((got - want).abs() <= tol).all()), (b, h, w, cin, cout, f16, (got - want).abs().max().item())
        assert bool((buf[:band] == 7.0).all()) and bool((buf[band + n_out:] == 7.0).all()), (b, h, w, cin, cout, f16)


# ---------------------------------------------------------------------------------------------------------------------
# Winograd F(4x4,3x3) (conv3x3_wino4_f32) against torch-CPU, absolute 1e-4 at unit scale
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,h,w,cin,cout,relu", [
    (1, 16, 32, 8, 64, False),      # exactly one M tile, one k plane
    (2, 16, 32, 16, 64, True),
    (1, 32, 64, 32, 128, True),     # several M and N tiles
    (2, 20, 28, 24, 64, True),      # ragged blocks: 5 x 7 positions
    (1, 4, 4, 8, 64, False),        # a single position
    (3, 64, 64, 256, 256, True),    # the FPN smoothing shape at P4 size
    (1, 4, 0, 8, 64, True),         # over the clamp (width 0: _over_the_clamp): one row of M tiles, 4 of their 16 rows used
])
def test_conv3x3_winograd4_vs_torch_cpu(dev, b, h, w, cin, cout, relu):
    from maskrcnn_amd import ops
    w = w or 32 * _over_the_clamp()
    g = torch.Generator().manual_seed(b * 1000 + h + cin)
    x = torch.randn(b, h, w, cin, generator=g).clamp_(min=0)          # post-ReLU activations, unit scale
    wt = torch.randn(cout, 3, 3, cin, generator=g) / (9 * cin * 0.5) ** 0.5
    sc = torch.rand(cout, generator=g) + 0.5
    sh = torch.randn(cout, generator=g) * 0.1
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), wt.permute(0, 3, 1, 2).double(), padding=1)
    ref = ref * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    if relu:
        ref = ref.clamp_(min=0)
    ref = ref.permute(0, 2, 3, 1).float()
    xk = ops.nhwc_to_kblocked(x.to(dev))
    u4 = ops.winograd4_weights(wt.to(dev).contiguous())
    y, yk = ops.conv3x3_winograd4(xk, u4, sc.to(dev), sh.to(dev), relu, out="both")
    err = (y.cpu() - ref).abs().max().item()
    assert err <= TOL, f"max|err| {err:.3g} at max|ref| {ref.abs().max().item():.3g}"
    assert torch.equal(ops.nhwc_to_kblocked(y), yk)
    y2 = ops.conv3x3_winograd4(xk, u4, sc.to(dev), sh.to(dev), relu, out="nhwc")
    assert torch.equal(y2, y)                                         # deterministic


@pytest.mark.parametrize("b,h,w,cout", [(1, 16, 32, 128), (2, 32, 64, 128), (2, 20, 28, 128), (1, 64, 64, 128),
                                        (1, 16, 32, 64), (2, 36, 40, 256),    # one, two and four N tiles
                                        (1, 4, 0, 64)])                       # over the clamp: one row of M tiles
def test_winograd4_fused_rpn_heads(dev, b, h, w, cout):
    """F(4x4) shared conv + both 1x1 heads in one launch (model.py:605-641) against torch-CPU, then through the
    scores/deltas kernel in its input form 3 against the NHWC form."""
    from maskrcnn_amd import ops
    w = w or 32 * _over_the_clamp()
    g = torch.Generator().manual_seed(h * 7 + w + cout)
    cin = 64
    x = torch.randn(b, h, w, cin, generator=g).clamp_(min=0)
    wt = torch.randn(cout, 3, 3, cin, generator=g) / (9 * cin * 0.5) ** 0.5
    bs = torch.randn(cout, generator=g) * 0.1
    wh = torch.randn(18, cout, generator=g) / (cout * 0.5) ** 0.5
    bh = torch.randn(18, generator=g) * 0.1
    shared = F.relu(F.conv2d(x.permute(0, 3, 1, 2).double(), wt.permute(0, 3, 1, 2).double(), bs.double(), padding=1))
    ref = (torch.einsum("bchw,oc->bhwo", shared, wh.double()) + bh.double()).float()
    w32 = torch.zeros(32, cout)
    w32[:18] = wh
    xk = ops.nhwc_to_kblocked(x.to(dev))
    u4 = ops.winograd4_weights(wt.to(dev).contiguous())
    sums = ops.conv3x3_winograd4_heads(xk, u4, None, bs.to(dev), w32.to(dev), True)
    assert sums.tile_mode == 3
    got = sums.to_nhwc(bh.to(dev)).cpu()
    err = (got - ref).abs().max().item()
    assert err <= TOL, f"max|err| {err:.3g} at max|ref| {ref.abs().max().item():.3g}"
    again = ops.conv3x3_winograd4_heads(xk, u4, None, bs.to(dev), w32.to(dev), True)
    assert torch.equal(again.to_nhwc(bh.to(dev)).cpu(), got)                          # deterministic
    # the consumer reads the M-tile-major rows directly: same scores / deltas as from the NHWC form
    small = [torch.randn(b, 4, 4, 18, generator=g).to(dev) for _ in range(4)]
    s_a, d_a = ops.rpn_scores_deltas([sums] + small, bh.to(dev))
    s_b, d_b = ops.rpn_scores_deltas([got.to(dev)] + small, bh.to(dev))
    assert torch.equal(s_a, s_b) and torch.equal(d_a, d_b)


@pytest.mark.parametrize("b,h,w,cin,c3", [(1, 16, 32, 64, 256), (2, 32, 64, 64, 256), (1, 20, 44, 32, 96), (3, 64, 64, 64, 256),
                                          (1, 256, 256, 64, 256), (1, 4, 0, 32, 64)])     # the last: over the clamp, one row of M tiles
def test_winograd4_fused_conv3(dev, b, h, w, cin, c3):
    """conv2 (F(4x4) Winograd, 64 output channels) + conv3 (1x1 expansion + affine + residual + ReLU) in one launch
    (model.py:197-209): the 64-channel map stays in the kernel's epilogue. Bit-identical to conv3x3_winograd4 followed by
    the direct kernel's conv_bn_act with the same residual — one M tile, ragged position blocks (20 x 44), several images,
    the full C2 size — and within 1e-4 abs of torch-CPU; run to run identical."""
    from maskrcnn_amd import ops
    w = w or 32 * _over_the_clamp()
    g = torch.Generator().manual_seed(4000 + h + w + c3)
    x = torch.randn(b, cin, h, w, generator=g)
    w2 = torch.randn(64, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
    s2, t2 = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    w3 = torch.randn(c3, 64, 1, 1, generator=g) * math.sqrt(2.0 / 64)
    s3, t3 = torch.rand(c3, generator=g) + 0.5, torch.randn(c3, generator=g) * 0.1
    res = torch.randn(b, c3, h, w, generator=g)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev)
    xk = ops.nhwc_to_kblocked(nhwc(x))
    u4 = ops.winograd4_weights(nhwc(w2))
    w3d, resd = nhwc(w3), nhwc(res)
    fused = ops.conv3x3_winograd4_conv3(xk, u4, s2.to(dev), t2.to(dev), w3d, s3.to(dev), t3.to(dev), resd)
    mid = ops.conv3x3_winograd4(xk, u4, s2.to(dev), t2.to(dev), True)
    two = ops.conv_bn_act(mid, w3d, s3.to(dev), t3.to(dev), relu=True, residual=resd)
    assert torch.equal(fused, two), f"max diff {(fused - two).abs().max().item():.3e}"
    assert torch.equal(fused, ops.conv3x3_winograd4_conv3(xk, u4, s2.to(dev), t2.to(dev), w3d, s3.to(dev), t3.to(dev), resd))
    t = F.relu(F.conv2d(x, w2, padding=1) * s2.view(1, -1, 1, 1) + t2.view(1, -1, 1, 1))
    want = F.relu(F.conv2d(t, w3) * s3.view(1, -1, 1, 1) + t3.view(1, -1, 1, 1) + res)
    err = (fused.permute(0, 3, 1, 2).cpu() - want).abs().max().item()
    assert err <= TOL, f"max abs err {err:.3e} (|ref|max {want.abs().max().item():.2f})"
    # no scale / shift vectors
    f0 = ops.conv3x3_winograd4_conv3(xk, u4, None, None, w3d, None, None, resd)
    m0 = ops.conv3x3_winograd4(xk, u4, None, None, True)
    assert torch.equal(f0, ops.conv_bn_act(m0, w3d, None, None, relu=True, residual=resd))


@pytest.mark.parametrize("cin,cout,relu,kblocked,m_extra", [(256, 64, True, True, 0), (64, 64, True, False, 0),
                                                            (64, 256, False, False, 0), (256, 48, True, False, 37)],
                         ids=["c2_conv1_kblocked", "c2_block1_conv1", "c2_downsample", "ragged_M_and_N"])
def test_streaming_1x1_kernel_bit_identical_to_tiled(dev, cin, cout, relu, kblocked, m_extra):
    """conv.hip's streaming 1x1 kernel (conv_pw_stream_f32: weights resident in LDS, every wave streams its own A fragments from
    global memory; taken from M >= 131072 rows) runs the same MFMA sequence per output as the tiled kernel, which the same call
    takes below that size: the big call must equal the row-chunked calls bit for bit, ragged last block and padded columns
    included, and stay within 1e-4 of torch (model.py:179-180,254-262: ResNet C2's conv1 / downsample at batch 8)."""
    from maskrcnn_amd import ops
    g = torch.Generator().manual_seed(11)
    m = 131072 + 32 * 8 + m_extra          # past the threshold; m_extra: a last block of fewer than 32 rows
    x = torch.randn(1, m, 1, cin, generator=g).to(dev)
    wt = (torch.randn(cout, 1, 1, cin, generator=g) / math.sqrt(cin)).to(dev)
    sc = (torch.rand(cout, generator=g) + 0.5).to(dev)
    sh = torch.randn(cout, generator=g).to(dev)
    canary = torch.full((1, m + 64, 1, cout), 7.0, device=dev)
    if kblocked:
        y = ops.conv_bn_act(x, wt, sc, sh, relu=relu, out_kblocked=True)                      # [Cout/8, 1, m, 1, 8]
        parts = [ops.conv_bn_act(x[:, lo:lo + 65536].contiguous(), wt, sc, sh, relu=relu, out_kblocked=True)
                 for lo in range(0, m, 65536)]
        ref = torch.cat(parts, dim=2)
        y_nhwc = y.permute(1, 2, 3, 0, 4).reshape(1, m, 1, cout)
    else:
        out = canary[:, :m]                                                                   # guard rows behind the output
        assert out.is_contiguous()
        y = ops.conv_bn_act(x, wt, sc, sh, relu=relu, out=out)
        ref = torch.cat([ops.conv_bn_act(x[:, lo:lo + 65536].contiguous(), wt, sc, sh, relu=relu)
                         for lo in range(0, m, 65536)], dim=1)
        assert torch.all(canary[:, m:] == 7.0), "the streaming kernel wrote past its last row"
        y_nhwc = y
    assert torch.equal(y, ref)
    want = _ref_conv(x.permute(0, 3, 1, 2).cpu(), wt.permute(0, 3, 1, 2).cpu(), sc.cpu(), sh.cpu(), 1, (0, 0, 0, 0), relu)
    assert (y_nhwc.permute(0, 3, 1, 2).cpu() - want).abs().max().item() <= TOL


@pytest.mark.parametrize("shape", [(2, 64, 96), (1, 256, 256), (1, 72, 40), (3, 16, 16), (1, 4, 4), (1, 832, 1344),
                                   (1, 4, 0)], ids=lambda s: "x".join(str(v) for v in s))
def test_stem_pool_f16_one_launch(shape):
    """Round 4, the "f16" mode's stem: conv 7x7 s2 + affine + ReLU + SamePad(3,2) + MaxPool(3,2) (model.py:223-229) as ONE launch
    on the fp16 MFMA (stem7x7_s2_pool_f16). Against torch-CPU on the SAME fp16-rounded image and weights (fp32 accumulation,
    one rounding of the conv output to fp16, then the max): equal up to the summation order — at most one fp16 ulp on a few
    values; and against the two-launch form it replaces (exact-fp32 products + fp16 store, then the fp16 max-pool): within the
    fp16 mode's tolerance, 2e-2 of the range. Ragged tiles, odd pooled sizes, several images; H or W not a multiple of 4 is refused
    (odd conv sizes give SamePad2d(3, 2) a top / left pad: the pipeline keeps the two launches there)."""
    from maskrcnn_amd import ops
    dev = torch.device("cuda:0")
    b, h, w = shape
    w = w or 64 * _over_the_clamp()   # width 0: one row of tiles (16 pooled pixels wide), over the clamp
    g = torch.Generator().manual_seed(h * 7 + w)
    img = torch.randint(0, 256, (b, 3, h, w), generator=g).float() - torch.tensor([123.7, 116.8, 103.9]).view(1, 3, 1, 1)
    wt = torch.randn(64, 3, 7, 7, generator=g) * 0.05
    scale = torch.rand(64, generator=g) + 0.5
    shift = torch.randn(64, generator=g) * 0.1
    w_ohwi = torch.zeros(64, 7, 7, 4)
    w_ohwi[..., :3] = wt.permute(0, 2, 3, 1)
    got = ops.stem_pool_f16(img.to(dev), w_ohwi.to(dev), scale.to(dev), shift.to(dev)).float().cpu()
    # reference on the operands the kernel sees
    x16, w16 = img.half().float(), wt.half().float()
    conv = F.conv2d(x16.double(), w16.double(), None, stride=2, padding=3).float()
    conv = F.relu(conv * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).half().float()
    oh, ow = conv.shape[2:]
    from oracle import oracle
    ref = F.max_pool2d(oracle.same_pad(conv, 3, 2), kernel_size=3, stride=2).permute(0, 2, 3, 1)
    assert tuple(got.shape) == tuple(ref.shape) == (b, (oh + 1) // 2, (ow + 1) // 2, 64)
    rng = ref.abs().max().item()
    # one fp16 ulp at the value — or 1e-4 absolute where the 147-term sum cancels to almost nothing (measured at 832 x 1344: five
    # values of 4.5 M, all below 1e-2, differ by up to 8e-6: the fp32 summation order against terms of magnitude ~30)
    ulp = torch.maximum(ref.abs() * 2.0 ** -10, torch.tensor(1e-4))
    diff = (got - ref).abs()
    assert bool((diff <= ulp).all()), f"max diff {diff.max().item():.3e} at range {rng:.1f}"
    assert float((diff > 0).float().mean()) < 0.02          # the rounding boundary is crossed rarely
    # the two launches it replaces
    two = ops.maxpool(ops.stem_conv(img.to(dev), w_ohwi.to(dev), scale.to(dev), shift.to(dev), True, nchw=True, out_f16=True), 3, 2,
                      ops.same_pad(oh, ow, 3, 2)).float().cpu()
    assert tuple(two.shape) == tuple(got.shape)
    assert (got - two).abs().max().item() <= 2e-2 * rng
    with pytest.raises(Exception):
        ops.stem_pool_f16(torch.zeros(1, 3, 70, 40, device=dev), w_ohwi.to(dev), None, None)


@pytest.mark.parametrize("shape", [(2, 64, 96), (1, 256, 256), (1, 72, 40), (3, 16, 16), (1, 4, 4), (1, 60, 132), (2, 1024, 1024),
                                   (1, 832, 1344), (1, 4, 0)], ids=lambda s: "x".join(str(v) for v in s))
def test_stem_pool_f32_one_launch(shape):
    """Round 5, the exact-fp32 stem: conv 7x7 s2 + affine + ReLU + SamePad(3,2) + MaxPool(3,2) (model.py:223-229) as ONE launch on
    the fp32 MFMA with K = 7 x 21 real values (stem7x7_s2_pool_f32). Against the two launches it replaces (stem7x7_s2_f32 +
    maxpool_nhwc: the same exact fp32 products summed in another order, then the same exact max): equal to rounding of the
    147-term sums; against torch-CPU fp32 conv + BN + ReLU + pad + max-pool at the pipeline's bar 1e-4 * max(1, max|act|) and
    against a float64 evaluation at a few ulps of the range. Ragged tiles (pooled heights that are not multiples of 7, widths
    not multiples of 16), several images, the 1 x 1 pooled map; H or W not a multiple of 4 is refused."""
    from maskrcnn_amd import ops
    from oracle import oracle
    dev = torch.device("cuda:0")
    b, h, w = shape
    w = w or 64 * _over_the_clamp()   # width 0: one row of tiles (16 pooled pixels wide), over the clamp
    g = torch.Generator().manual_seed(h * 7 + w)
    img = torch.randint(0, 256, (b, 3, h, w), generator=g).float() - torch.tensor([123.7, 116.8, 103.9]).view(1, 3, 1, 1)
    wt = torch.randn(64, 3, 7, 7, generator=g) * 0.05
    scale = torch.rand(64, generator=g) + 0.5
    shift = torch.randn(64, generator=g) * 0.1
    w_ohwi = torch.zeros(64, 7, 7, 4)
    w_ohwi[..., :3] = wt.permute(0, 2, 3, 1)
    got = ops.stem_pool_f32(img.to(dev), w_ohwi.to(dev), scale.to(dev), shift.to(dev))
    oh, ow = h // 2, w // 2
    two = ops.maxpool(ops.stem_conv(img.to(dev), w_ohwi.to(dev), scale.to(dev), shift.to(dev), True, nchw=True), 3, 2,
                      ops.same_pad(oh, ow, 3, 2))
    torch.cuda.synchronize()
    assert tuple(got.shape) == tuple(two.shape) == (b, (oh + 1) // 2, (ow + 1) // 2, 64)
    rng = two.abs().max().item()
    assert (got - two).abs().max().item() <= 4e-6 * max(1.0, rng), ((got - two).abs().max().item(), rng)
    if b * h * w <= 2 * 1024 * 1024:
        conv = F.conv2d(img, wt, None, stride=2, padding=3)
        ref = F.relu(conv * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
        ref = F.max_pool2d(oracle.same_pad(ref, 3, 2), kernel_size=3, stride=2).permute(0, 2, 3, 1)
        assert (got.cpu() - ref).abs().max().item() <= 1e-4 * max(1.0, ref.abs().max().item())
    if b * h * w <= 256 * 256:
        c64 = F.conv2d(img.double(), wt.double(), None, stride=2, padding=3)
        r64 = F.relu(c64 * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
        r64 = F.max_pool2d(oracle.same_pad(r64, 3, 2), kernel_size=3, stride=2).permute(0, 2, 3, 1)
        assert (got.cpu().double() - r64).abs().max().item() <= 8 * 2.0 ** -23 * max(1.0, r64.abs().max().item())
    # nothing is written outside the output (guard rows) and a second call gives the same bits (persistent tiles, prefetch)
    again = ops.stem_pool_f32(img.to(dev), w_ohwi.to(dev), scale.to(dev), shift.to(dev))
    assert torch.equal(again, got)
    # without the affine vectors
    plain = ops.stem_pool_f32(img.to(dev), w_ohwi.to(dev), None, None)
    two_p = ops.maxpool(ops.stem_conv(img.to(dev), w_ohwi.to(dev), None, None, True, nchw=True), 3, 2, ops.same_pad(oh, ow, 3, 2))
    assert (plain - two_p).abs().max().item() <= 4e-6 * max(1.0, two_p.abs().max().item())
    with pytest.raises(Exception):
        ops.stem_pool_f32(torch.zeros(1, 3, 70, 40, device=dev), w_ohwi.to(dev), None, None)
