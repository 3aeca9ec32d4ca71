"""GPU sweep (-m gpu) of the hand-written fused kernels on exact data (tests/fused_exact_cases.py; the twin of
tests/test_gpu_conv_exact.py): Winograd F(2x2) plain and with the RPN heads, conv_f16_pipelined_heads, the whole-block fp32
Bottleneck, the three stem kernels, the one-launch fp16 C2 block and the fp16 mask tail. The data are small integers times
powers of two for which every sum is exact in fp32 and every fp16 intermediate is the exact value rounded once, so each kernel
must equal a float64 evaluation BIT FOR BIT in any summation order. Every operand sits between NaN bands and every output
between 0xFF bands (the outputs go to the C entry points, as the bindings allocate their own); a second call gives the same
bits; image (RoI) i of a batch equals image i alone. The last test runs the file once more on the schedule-fuzzing build:
there a hand-placed barrier that orders too little contradicts a bit pattern.

What this proves is indexing, padding, tails, layouts, the place of every rounding and of the residual. It does not measure
accumulation accuracy on real-valued data: that stays with the tolerance tests of tests/test_gpu_conv.py. The F(4x4) kernels
(csrc/conv_wino4.hip) have a sweep of their own, tests/test_gpu_wino4_exact.py: their G holds 64/81, 32/81 and 8/27, so U = G g G^T
is not dyadic for integer g and no convolution is exact; but they take U as an operand, and on a synthetic integer U the bilinear
form A^T [sum U .* (B^T d B)] A is."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fused_exact_cases as C
from test_gpu_conv_exact import TOL, _banded, _bands_intact, _bits, _poisoned

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ_LIB = os.path.join(ROOT, "maskrcnn_amd", "csrc", "build", "variants", "sync_fuzz", "libmaskrcnn_hip.so")
_ID = lambda c: c.id
F32, F16 = torch.float32, torch.float16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import maskrcnn_amd  # noqa: F401
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _rebanded(t):
    """A device tensor (a transformed filter, weight fragments) moved between NaN bands."""
    buf = torch.full((t.numel() + 2048,), float("nan"), dtype=t.dtype, device=t.device)
    buf[1024:1024 + t.numel()] = t.reshape(-1)
    return buf[1024:1024 + t.numel()].view(t.shape)


def _assert_bits(got, want, dev, what):
    want = torch.from_numpy(np.ascontiguousarray(want)).to(dev)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)     # as bits: +0 where the reference's zeros are
    if bool(bad.any()):
        at = tuple(int(v[0]) for v in torch.nonzero(bad, as_tuple=True))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {list(at)}: "
                             f"got {got[at].item()!r}, want {want[at].item()!r}")


def _exact(what, dev, launch, shapes, dtype, wants):
    """launch(outs) writes the outputs of these shapes: each between 0xFF bands that must stay intact, equal to its `want` as
    bits (None: not compared here), and the same bits on a second call. -> the outputs of the first call."""
    pairs = [_poisoned(s, dtype, dev) for s in shapes]
    outs = [o for _, o in pairs]
    launch(outs)
    torch.cuda.synchronize()
    for buf, o in pairs:
        assert _bands_intact(buf, o), f"{what}: a byte of an output's guard bands changed"
    first = [o.clone() for o in outs]
    for f, w in zip(first, wants):
        if w is not None:
            _assert_bits(f, w, dev, what)
    for o in outs:
        _bits(o).fill_(-1)      # every byte 0xFF again (the outputs are contiguous: _bits is a view)
    launch(outs)
    for (buf, o), f in zip(pairs, first):
        assert torch.equal(_bits(o), _bits(f)), f"{what}: a second call differs"
        assert _bands_intact(buf, o), what
    return first


def _images(n):
    return range(n) if n <= 3 else (0, n - 1)


# ---------------------------------------------------------------------------------------------------------------------
# F(2x2) plain
# ---------------------------------------------------------------------------------------------------------------------
def _wino_call(x, layout, shape, u, cout, scale, shift, relu, y, yk):
    from maskrcnn_amd._lib import check, lib
    b, h, w, cin = shape
    nbytes, ws = 0, None
    if layout == 0:
        nbytes = int(lib.mrcnn_conv3x3_winograd_workspace_bytes(b, h, w, cin))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    check(lib.mrcnn_conv3x3_winograd_f32(x.data_ptr(), layout, b, h, w, cin, u.data_ptr(), cout, _p(scale), _p(shift), int(relu),
                                         _p(y), _p(yk), _p(ws), nbytes, _stream()))


WINO_RUNS = [(c, xin, out) for c in C.WINO_CASES for xin in ("nhwc", "kblocked")
             for out in (("nhwc", "kblocked", "both") if c.cout % 8 == 0 else ("nhwc",))]


@pytest.mark.parametrize("case,xin,out", WINO_RUNS, ids=lambda v: v.id if hasattr(v, "id") else v)
def test_winograd_f2x2_is_exact(dev, case, xin, out):
    """ops.conv3x3_winograd's entry point: NHWC and k-blocked inputs, the three output forms, with and without scale and ReLU,
    on the linear-tile kernel (forced: winograd_set_spatial(0)) and on the default choice — linear tiles under 16 x 16 pixels,
    8 x 8-position blocks from there on —, which give the same bits."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import lib
    d = C.build(case)
    b, h, w, cin, cout = case.b, case.h, case.w, case.cin, case.cout
    assert (int(lib.mrcnn_conv3x3_winograd_heads_tile_mode(h, w)) == 2) == (case.tiles == "spatial")
    lay = (lambda a: C.kblocked(a)) if xin == "kblocked" else (lambda a: a)
    x = _banded(lay(d.x), F32, dev)
    ones = [_banded(lay(d.x[i:i + 1]), F32, dev) for i in _images(b)]
    u = _rebanded(ops.winograd_weights(_banded(d.w, F32, dev)))
    scale, shift = _banded(d.scale, F32, dev), _banded(d.shift, F32, dev)
    nhwc, kb = out != "kblocked", out != "nhwc"

    def shapes(n):
        return ([(n, h, w, cout)] if nhwc else []) + ([(cout // 8, n, h, w, 8)] if kb else [])

    def launch(xt, n, with_scale, with_relu):
        def go(outs):
            y, yk = (outs[0] if nhwc else None), (outs[-1] if kb else None)
            _wino_call(xt, int(xin == "kblocked"), (n, h, w, cin), u, cout, scale if with_scale else None, shift, with_relu, y, yk)
        return go

    try:
        for with_scale, with_relu in C.WINO_VARIANTS:
            want = d.want[(with_scale, with_relu)]
            wants = ([want] if nhwc else []) + ([C.kblocked(want)] if kb else [])
            what = f"{case.id} {xin}->{out} scale={with_scale} relu={with_relu}"
            got = {}
            for mode in (0, -1):
                ops.winograd_set_spatial(mode)
                got[mode] = _exact(f"{what} spatial={mode}", dev, launch(x, b, with_scale, with_relu), shapes(b), F32, wants)
                for i, xi in zip(_images(b), ones):
                    one = _exact(f"{what} spatial={mode} image {i}", dev, launch(xi, 1, with_scale, with_relu), shapes(1), F32,
                                 [None] * len(wants))
                    for o1, whole in zip(one, got[mode]):
                        part = whole[i:i + 1] if whole.dim() == 4 else whole[:, i:i + 1]
                        assert torch.equal(_bits(o1), _bits(part)), f"{what}: image {i} alone differs from image {i} of the batch"
            for a, bb in zip(got[0], got[-1]):
                assert torch.equal(_bits(a), _bits(bb)), f"{what}: linear and default tiles differ"
    finally:
        ops.winograd_set_spatial(-1)


# ---------------------------------------------------------------------------------------------------------------------
# the RPN heads inside a conv
# ---------------------------------------------------------------------------------------------------------------------
def _valid_head_rows(part, case, mode):
    """part [2, rows, 32] -> [2, B, H, W, 32]: the rows of real pixels, in image order (HeadSums.to_nhwc's own map)."""
    b, h, w = case.b, case.h, case.w
    if mode == 4:
        return part.view(2, b, h, w, 32)
    tyb, txb = -(-(h // 2) // 8), -(-(w // 2) // 8)
    v = part.view(2, b, tyb, txb, 8, 8, 2, 2, 32).permute(0, 1, 2, 4, 6, 3, 5, 7, 8).reshape(2, b, tyb * 16, txb * 16, 32)
    return v[:, :, :h, :w]


@pytest.mark.parametrize("case", C.HEADS_CASES, ids=_ID)
def test_rpn_heads_inside_the_conv_are_exact(dev, case):
    """ops.conv3x3_winograd_heads (fp32) and ops.conv_f16_pipelined_heads (fp16 operands; the ReLU'd tile rounded to fp16 once):
    to_nhwc(bias) equals float64 bit for bit, and the 14 padded head columns of every pixel's row are +0."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._binding import HeadSums
    from maskrcnn_amd._lib import check, lib
    d = C.build(case)
    b, h, w, cin, cout = case.b, case.h, case.w, case.cin, case.cout
    scale, shift, bias = _banded(d.scale, F32, dev), _banded(d.shift, F32, dev), _banded(d.bias, F32, dev)
    if case.op == "wino":
        mode = int(lib.mrcnn_conv3x3_winograd_heads_tile_mode(h, w))
        assert mode == 2
        u = _rebanded(ops.winograd_weights(_banded(d.w, F32, dev)))
        wh = _banded(d.w_head32, F32, dev)
        rows = lambda n: int(lib.mrcnn_conv3x3_winograd_heads_rows(n, h, w, mode))
        xs = lambda a: _banded(C.kblocked(a), F32, dev)

        def launch(xt, n):
            return lambda outs: check(lib.mrcnn_conv3x3_winograd_heads_f32(
                xt.data_ptr(), n, h, w, cin, u.data_ptr(), cout, scale.data_ptr(), shift.data_ptr(), 1, wh.data_ptr(), mode,
                outs[0].data_ptr(), _stream()))
    else:
        mode = 4
        assert ops.conv_f16_pipelined_supported(b, h, w, cin, cout, 3, 3, (1, 1, 1, 1))
        wt, wh = _banded(d.w, F16, dev), _banded(d.w_head32, F16, dev)
        rows = lambda n: n * h * w
        xs = lambda a: _banded(a, F16, dev)

        def launch(xt, n):
            return lambda outs: check(lib.mrcnn_conv_f16_pipelined_heads(
                xt.data_ptr(), n, h, w, cin, wt.data_ptr(), cout, 3, 3, 1, 1, 1, 1, scale.data_ptr(), shift.data_ptr(), 1,
                wh.data_ptr(), outs[0].data_ptr(), 0, _stream()))

    part, = _exact(case.id, dev, launch(xs(d.x), b), [(2, rows(b), 32)], F32, [None])
    got = HeadSums(part, b, h, w, mode).to_nhwc(bias)
    _assert_bits(got, d.want, dev, case.id)
    valid = _valid_head_rows(part, case, mode)
    assert not bool(_bits(valid[..., 18:]).any()), f"{case.id}: a padded head column is not +0"
    want_sums = torch.from_numpy(d.sums.astype(np.float32)).to(dev)
    assert torch.equal(valid[0] + valid[1], want_sums), f"{case.id}: the two planes do not add up to the head sums"
    for i in _images(b):
        one = dataclasses.replace(case, b=1)
        p1, = _exact(f"{case.id} image {i}", dev, launch(xs(d.x[i:i + 1]), 1), [(2, rows(1), 32)], F32, [None])
        assert torch.equal(_bits(_valid_head_rows(p1, one, mode)), _bits(valid[:, i:i + 1])), \
            f"{case.id}: image {i} alone differs from image {i} of the batch"


# ---------------------------------------------------------------------------------------------------------------------
# whole-block fp32 Bottleneck
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.BLOCK_CASES, ids=_ID)
def test_bottleneck_fused_is_exact(dev, case):
    """ops.bottleneck_fused's entry point against three float64 layers with the identity residual."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import check, lib
    d = C.build(case)
    b, h, w = case.b, case.h, case.w
    assert ops.bottleneck_fused_supported(h, w, 256, 64)
    t = {k: _banded(getattr(d, k), F32, dev) for k in ("w1", "s1", "t1", "s2", "t2", "w3", "s3", "t3")}
    u2 = _rebanded(ops.winograd_weights(_banded(d.w2, F32, dev)))

    def launch(xt, n):
        return lambda outs: check(lib.mrcnn_bottleneck_fused_f32(
            xt.data_ptr(), n, h, w, 256, t["w1"].data_ptr(), t["s1"].data_ptr(), t["t1"].data_ptr(), u2.data_ptr(), t["s2"].data_ptr(),
            t["t2"].data_ptr(), t["w3"].data_ptr(), t["s3"].data_ptr(), t["t3"].data_ptr(), 64, outs[0].data_ptr(), _stream()))

    got, = _exact(case.id, dev, launch(_banded(d.x, F32, dev), b), [(b, h, w, 256)], F32, [d.want])
    for i in _images(b):
        one, = _exact(f"{case.id} image {i}", dev, launch(_banded(d.x[i:i + 1], F32, dev), 1), [(1, h, w, 256)], F32, [None])
        assert torch.equal(_bits(one), _bits(got[i:i + 1])), f"{case.id}: image {i} alone differs from image {i} of the batch"


# ---------------------------------------------------------------------------------------------------------------------
# stem
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.STEM_CASES, ids=_ID)
def test_stem_kernels_are_exact(dev, case):
    """ops.stem_conv in its NHWC, NCHW and fp16-output forms, ops.stem_pool_f32 and ops.stem_pool_f16 (whose fp32 -> fp16
    conversion of the image rounds, ties included): conv, affine, ReLU, (one rounding to fp16,) zero pad at the bottom / right,
    max-pool 3/2. The `dead` cases: a ReLU map of zeros, where the padding zero and the real zeros both give +0."""
    from maskrcnn_amd._lib import check, lib
    d = C.build(case)
    b, h, w = case.b, case.h, case.w
    wt, scale, shift = _banded(d.w, F32, dev), _banded(d.scale, F32, dev), _banded(d.shift, F32, dev)
    pool = case.op.startswith("pool")
    fn = {"conv_nhwc": lib.mrcnn_stem_conv7x7_s2_nhwc_f32, "conv_nchw": lib.mrcnn_stem_conv7x7_s2_nchw_f32,
          "conv_f16": lib.mrcnn_stem_conv7x7_s2_nchw_f16out, "pool_f32": lib.mrcnn_stem_conv7x7_s2_pool_f32,
          "pool_f16": lib.mrcnn_stem_conv7x7_s2_pool_f16}[case.op]

    def image(a):
        if case.op == "conv_nhwc":      # RGB + a zero channel
            return _banded(np.concatenate([a, np.zeros(a.shape[:3] + (1,))], 3), F32, dev)
        return _banded(a.transpose(0, 3, 1, 2), F32, dev)

    def launch(xt, n):
        relu = () if pool else (1,)
        return lambda outs: check(fn(xt.data_ptr(), n, h, w, wt.data_ptr(), scale.data_ptr(), shift.data_ptr(), *relu,
                                     outs[0].data_ptr(), _stream()))

    dt = F16 if case.out16 else F32
    oh, ow = (h // 4, w // 4) if pool else (h // 2, w // 2)
    assert d.want.shape == (b, oh, ow, 64)
    got, = _exact(case.id, dev, launch(image(d.img), b), [(b, oh, ow, 64)], dt, [d.want])
    for i in _images(b):
        one, = _exact(f"{case.id} image {i}", dev, launch(image(d.img[i:i + 1]), 1), [(1, oh, ow, 64)], dt, [None])
        assert torch.equal(_bits(one), _bits(got[i:i + 1])), f"{case.id}: image {i} alone differs from image {i} of the batch"


# ---------------------------------------------------------------------------------------------------------------------
# the one-launch fp16 C2 block
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.C2_CASES, ids=_ID)
def test_bottleneck_c2_f16_is_exact(dev, case):
    """ops.bottleneck_c2_f16's entry point, identity and first block: both 64-channel maps and the downsample branch rounded to
    fp16 once, the residual added in fp32 BEFORE the ReLU and the one rounding of the output."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import check, lib
    d = C.build(case)
    b, h, w, cin = case.b, case.h, case.w, case.cin
    assert ops.bottleneck_c2_f16_supported(b, h, w, cin, 64, case.first)
    frag = lambda a: _rebanded(ops.pack_afrags_f16(_banded(a, F16, dev)))
    f1, f2, f3 = frag(d.w1), frag(d.w2), frag(d.w3)
    fd = frag(d.wd) if case.first else None
    t = {k: _banded(getattr(d, k), F32, dev) for k in ("s1", "t1", "s2", "t2", "s3", "t3") + (("sd", "td") if case.first else ())}

    def launch(xt, n):
        return lambda outs: check(lib.mrcnn_bottleneck_c2_f16(
            xt.data_ptr(), n, h, w, cin, f1.data_ptr(), t["s1"].data_ptr(), t["t1"].data_ptr(), f2.data_ptr(), t["s2"].data_ptr(),
            t["t2"].data_ptr(), f3.data_ptr(), t["s3"].data_ptr(), t["t3"].data_ptr(), _p(fd), _p(t.get("sd")), _p(t.get("td")),
            outs[0].data_ptr(), _stream()))

    got, = _exact(case.id, dev, launch(_banded(d.x, F16, dev), b), [(b, h, w, 256)], F16, [d.want])
    for i in _images(b):
        one, = _exact(f"{case.id} image {i}", dev, launch(_banded(d.x[i:i + 1], F16, dev), 1), [(1, h, w, 256)], F16, [None])
        assert torch.equal(_bits(one), _bits(got[i:i + 1])), f"{case.id}: image {i} alone differs from image {i} of the batch"


# ---------------------------------------------------------------------------------------------------------------------
# the fp16 mask tail
# ---------------------------------------------------------------------------------------------------------------------
def _check_sigmoid(what, pre, want, got):
    """The sigmoid's argument is exact: outputs with one argument hold one bit pattern, and the outputs are non-decreasing in
    the argument — both exact. The values themselves are held to tests/test_gpu_conv_exact.py's TOL against float64."""
    pre = pre.reshape(-1)
    y = got.reshape(-1).double().cpu().numpy()
    order = np.argsort(pre, kind="stable")
    ps, ys = pre[order], y[order]
    same = ps[1:] == ps[:-1]
    assert np.array_equal(ys[1:][same], ys[:-1][same]), f"{what}: one argument, two outputs"
    assert bool((ys[1:] >= ys[:-1]).all()), f"{what}: the outputs are not monotonic in the exact argument"
    err = float(np.abs(y - want.reshape(-1)).max())
    assert err <= TOL, f"{what}: sigmoid off by {err:.3e}"


@pytest.mark.parametrize("case", C.TAIL_CASES, ids=_ID)
def test_mask_tail_f16_is_exact(dev, case):
    """ops.mask_tail_f16's entry point: the deconv's map rounded to fp16 once (a third of its elements change, a tenth on a
    tie), conv5's sum — the sigmoid's argument — exact."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import check, lib
    d = C.build(case)
    r, h, w, classes = case.r, case.h, case.w, case.classes
    assert ops.mask_tail_f16_supported(r, h, w, 256, 256, classes)
    fde = _rebanded(ops.pack_afrags_f16(_banded(d.wde, F16, dev)))
    w5p = np.concatenate([d.w5.reshape(classes, 256), np.zeros((96 - classes, 256))], 0)
    f5 = _rebanded(ops.pack_afrags_f16(_banded(w5p, F16, dev)))
    bde4, b5 = _banded(np.tile(d.bde, 4), F32, dev), _banded(d.b5, F32, dev)

    def launch(xt, n):
        return lambda outs: check(lib.mrcnn_mask_tail_f16(xt.data_ptr(), n, h, w, 256, fde.data_ptr(), bde4.data_ptr(), 256,
                                                          f5.data_ptr(), b5.data_ptr(), classes, outs[0].data_ptr(), _stream()))

    got, = _exact(case.id, dev, launch(_banded(d.x, F16, dev), r), [(r, 2 * h, 2 * w, classes)], F32, [None])
    _check_sigmoid(case.id, d.pre, d.want64, got)
    for i in _images(r):
        one, = _exact(f"{case.id} RoI {i}", dev, launch(_banded(d.x[i:i + 1], F16, dev), 1), [(1, 2 * h, 2 * w, classes)], F32, [None])
        assert torch.equal(_bits(one), _bits(got[i:i + 1])), f"{case.id}: RoI {i} alone differs from RoI {i} of the batch"


def test_the_case_table_is_complete():
    assert C.coverage_problems() == []


# ---------------------------------------------------------------------------------------------------------- schedule fuzzing
# The child's time limit: four times the wall time measured on the fuzzed library, rounded up to 30 s: 5.5 s (62 tests; 3.3 s of
# it inside pytest, the rest start-up), so 21.8 s -> 30 s.
FUZZ_TIMEOUT = 30


@pytest.mark.skipif(os.environ.get("MRCNN_SYNC_FUZZ_CHILD") == "1", reason="this IS the fuzzed child run")
def test_this_file_passes_under_schedule_fuzzing():
    """These kernels hand tiles from wave to wave through LDS behind hand-placed barriers (the Winograd transforms, the
    Bottleneck's two on-chip maps, the stems' conv image under the pool, T1 of the fp16 block, the mask tail's weight halves, the
    pipelined conv's partial head sums). On the schedule-fuzzing build every wave sleeps a random time behind each barrier: a
    hand-off that the barrier does not order gives other bits there, and every comparison above is a comparison of bits."""
    assert os.path.exists(FUZZ_LIB), f"{FUZZ_LIB} is missing: run __graft_entry__.build()"
    env = dict(os.environ, MRCNN_LIB=FUZZ_LIB, MRCNN_SYNC_FUZZ_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_fused_exact.py", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=FUZZ_TIMEOUT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
