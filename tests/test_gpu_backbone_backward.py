"""GPU tests (-m gpu) of the backbone backward: ops.conv_bn_act_backward with a stride (csrc/conv_backward.hip), ops.dilate2_sum and
ops.maxpool_backward (csrc/pool_backward.hip), and the differentiable front ends layers.conv_bn_act(stride=2), layers.maxpool and
layers.bottleneck.

Exact data (backbone_backward_cases): every result equals the float64 autograd result of the stock-torch graph bit for bit, whatever
the chunking of the weight gradient; tests/test_backbone_backward_host.py asserts, without a GPU, the conditions that make this a
theorem. Rounded data: the max-pool backward and dilate2_sum against their rules restated in numpy bit for bit, dw against a float64
evaluation within the forward error bound of a recursive fp32 sum of the chunk's length. The shapes are the smallest at which each
mechanism can go wrong. The file runs once more in a child pytest on the schedule-fuzz library."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import backbone_backward_cases as bb

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ_LIB = os.path.join(ROOT, "maskrcnn_amd", "csrc", "build", "variants", "sync_fuzz", "libmaskrcnn_hip.so")
F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from maskrcnn_amd import ops as o
    return o


@pytest.fixture(scope="module")
def layers():
    from maskrcnn_amd import layers as m
    return m


def dev(t, dtype=F32):
    return None if t is None else t.to(dtype).contiguous().to(DEV)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def assert_same_bits(got, want64, what, signed_zero=False):
    """got (fp32, GPU) against a float64 expectation that fp32 holds exactly. -0 and +0 are the same number unless signed_zero."""
    assert got is not None, what
    got, want = got.detach().cpu(), want64.to(F32)
    assert torch.equal(want.to(F64), want64.to(F64)), f"{what}: the expectation is not an fp32 number"
    assert got.shape == want.shape and got.dtype == F32, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    if not signed_zero:
        got, want = got + 0.0, want + 0.0
    same = got.contiguous().view(torch.int32) == want.contiguous().view(torch.int32)
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} elements differ in their bits"


def nan_like(shape):
    return torch.full(shape, float("nan"), dtype=F32, device=DEV)


def assert_odd_positions_are_plus_zero(dx, what):
    raw = bits(dx)
    assert not bool(raw[:, 1::2].any()) and not bool(raw[:, :, 1::2].any()), f"{what}: an odd row or column is not +0"


# ------------------------------------------------------------------------------------------------------------- strided convs
def conv_call(ops, c, d, needs=None):
    needs = (c.pointwise, True, True, False) if needs is None else needs
    r = ops.conv_bn_act_backward(dev(d.dy), dev(d.x), dev(d.w), dev(d.y), dev(d.scale), c.pad, c.act, needs=needs, stride=c.stride)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("name", [c.id for c in bb.CONVS])
def test_strided_dw_dshift_and_z_equal_float64_bit_for_bit(ops, name):
    c = bb.conv_case(name)
    d = bb.build_conv(c)
    r = conv_call(ops, c, d)
    assert_same_bits(r.z, d.z, f"{name}: z")
    assert_same_bits(r.dw, d.dw, f"{name}: dw")
    assert_same_bits(r.dshift, d.dshift, f"{name}: dshift")
    assert (r.dx is not None) == c.pointwise
    if name == bb.MULTI_CHUNK:
        L = ops.conv_backward_chunk(c.b, c.h, c.w, c.cin, c.cout, *c.k, c.pad, stride=2)
        assert L == 128 and -(-c.m // L) == 4, L


@pytest.mark.parametrize("name", [c.id for c in bb.CONVS if c.pointwise])
def test_strided_dx_is_written_everywhere_and_equals_float64_bit_for_bit(ops, name):
    c = bb.conv_case(name)
    d = bb.build_conv(c)
    r = conv_call(ops, c, d)
    oh, ow = c.out_hw
    assert r.dx.shape == (c.b, oh, ow, c.cin), "the op returns the compact gradient"
    assert_same_bits(r.dx, d.dx[:, ::2, ::2], f"{name}: compact dx")
    out = nan_like((c.b, c.h, c.w, c.cin))
    got = ops.dilate2_sum(r.dx, None, c.h, c.w, out=out)
    torch.cuda.synchronize()
    assert got is out
    assert_same_bits(out, d.dx, f"{name}: dx")
    assert_odd_positions_are_plus_zero(out, name)
    # the compact gradient IS the forward launch on z with the transposed weight
    wt = r.z.new_zeros(c.cin, 1, 1, c.cout4)
    wt[:, 0, 0, :c.cout] = dev(d.w)[:, 0, 0, :].t()
    fwd = ops.conv_bn_act(r.z, wt.contiguous(), None, None)
    assert torch.equal(bits(fwd), bits(r.dx)), f"{name}: dx is not the forward on z bit for bit"


@pytest.mark.parametrize("shape", bb.DILATE_SHAPES)
def test_dilate2_sum_with_two_operands_equals_the_float64_sum(ops, shape):
    _, h, w, _ = shape
    a, b = bb.dilate_operands(shape)
    for second in (None, b):
        out = nan_like(shape)
        ops.dilate2_sum(dev(a), dev(second), h, w, out=out)
        torch.cuda.synchronize()
        assert_same_bits(out, bb.dilate2_sum64(a, second, h, w), f"{shape}: {'a + b' if second is not None else 'a'}")
        assert_odd_positions_are_plus_zero(out, shape)
    # rounded operands: one fp32 add, as numpy makes it; a lone operand keeps its bits, -0 included
    a, b = bb.dilate_operands(shape, rounded=True)
    a[0, 0, 0, 0], b[0, 0, 0, 0] = -0.0, -0.0
    got = ops.dilate2_sum(dev(a), dev(b), h, w)
    assert torch.equal(bits(got), torch.from_numpy(bb.dilate2_sum_np(a.numpy(), b.numpy(), h, w)).view(torch.int32))
    got = ops.dilate2_sum(dev(a), None, h, w)
    assert torch.equal(bits(got), torch.from_numpy(bb.dilate2_sum_np(a.numpy(), None, h, w)).view(torch.int32))


# ---------------------------------------------------------------------------------------------------------- max-pool backward
@pytest.mark.parametrize("name", [p.id for p in bb.POOLS])
def test_maxpool_backward_equals_float64_and_the_numpy_rule_bit_for_bit(ops, name):
    p = bb.pool_case(name)
    x, dy = bb.pool_operands(p)
    y = ops.maxpool(dev(x), p.kernel, p.stride, p.pad)
    assert_same_bits(y, bb.pool64(x, p.kernel, p.stride, p.pad), f"{name}: the forward")
    out = nan_like((p.b, p.h, p.w, p.c))
    got = ops.maxpool_backward(dev(dy), dev(x), p.kernel, p.stride, p.pad, out=out)
    torch.cuda.synchronize()
    assert got is out
    assert_same_bits(out, bb.pool_grad64(p, x, dy), f"{name}: integer gradients")
    # rounded gradients: the ascending-order fp32 sum, sign of zero included (+0 where nothing is taken)
    x, dy = bb.pool_operands(p, rounded=True)
    want, _ = bb.maxpool_backward_np(x.numpy(), dy.numpy(), p.kernel, p.stride, p.pad)
    got = ops.maxpool_backward(dev(dy), dev(x), p.kernel, p.stride, p.pad)
    assert torch.equal(bits(got), torch.from_numpy(want).view(torch.int32)), f"{name}: rounded gradients"
    again = ops.maxpool_backward(dev(dy), dev(x), p.kernel, p.stride, p.pad)
    assert torch.equal(bits(got), bits(again))


def test_maxpool_backward_nan_takes_the_gradient_as_in_torch(ops):
    x = torch.tensor([0.0, 1.0, float("nan"), 1.0, 2.0, float("nan"), 2.0, 2.0, -1.0]).reshape(1, 3, 3, 1).expand(1, 3, 3, 4).contiguous()
    dy = torch.full((1, 1, 1, 4), 5.0)
    got = ops.maxpool_backward(dy.to(DEV), x.to(DEV), 3, 1).cpu()
    want, _ = bb.maxpool_backward_np(x.numpy(), dy.numpy(), 3, 1, (0, 0, 0, 0))
    assert torch.equal(bits(got), torch.from_numpy(want).view(torch.int32)) and float(got[0, 1, 2, 0]) == 5.0


def test_layers_maxpool_reaches_both_backwards(ops, layers):
    for name in ("3x3_s2_odd", "1x1_s2"):
        p = bb.pool_case(name)
        x, dy = bb.pool_operands(p)
        xg = dev(x).requires_grad_(True)
        y = layers.maxpool(xg, p.kernel, p.stride, p.pad)
        assert y.grad_fn is not None and torch.equal(y.detach(), ops.maxpool(xg.detach(), p.kernel, p.stride, p.pad))
        y.backward(dev(dy))
        assert_same_bits(xg.grad, bb.pool_grad64(p, x, dy), f"{name}: dx")
    assert ops.maxpool(xg, p.kernel, p.stride, p.pad).grad_fn is None                 # the inference call is unchanged


# ----------------------------------------------------------------------------------------------------------------- bottleneck
def block_on_gpu(layers, k, d, x_grad=True, frozen=()):
    p = {n: dev(v) for n, v in d.p.items()}
    for n in bb.BLOCK_PARAMS:
        if p[n] is not None and n not in frozen:
            p[n].requires_grad_(True)
    x = dev(d.x).requires_grad_(x_grad)
    y = layers.bottleneck(x, p["w1"], p["s1"], p["t1"], p["w2"], p["s2"], p["t2"], p["w3"], p["s3"], p["t3"], p["wd"], p["sd"], p["td"],
                          stride=k.stride)
    return x, p, y


@pytest.mark.parametrize("name", [k.id for k in bb.BLOCKS])
def test_bottleneck_forward_and_gradients_equal_float64_bit_for_bit(ops, layers, name):
    k = bb.block_case(name)
    d = bb.build_block(k)
    x, p, y = block_on_gpu(layers, k, d)
    assert y.grad_fn is not None
    # the forward is the composition of ops.conv_bn_act, bit for bit
    q = {n: (None if v is None else v.detach()) for n, v in p.items()}
    res = x.detach() if q["wd"] is None else ops.conv_bn_act(x.detach(), q["wd"], q["sd"], q["td"], k.stride)
    h1 = ops.conv_bn_act(x.detach(), q["w1"], q["s1"], q["t1"], k.stride, relu=True)
    h2 = ops.conv_bn_act(h1, q["w2"], q["s2"], q["t2"], 1, (1, 1, 1, 1), True)
    comp = ops.conv_bn_act(h2, q["w3"], q["s3"], q["t3"], 1, relu=True, residual=res)
    assert torch.equal(bits(y), bits(comp)), f"{name}: the forward is not the composition of ops.conv_bn_act"
    assert_same_bits(y, d.y, f"{name}: forward")
    y.backward(dev(d.dy))
    torch.cuda.synchronize()
    assert_same_bits(x.grad, d.grads["x"], f"{name}: dx")
    for n in bb.BLOCK_PARAMS:
        if p[n] is not None:
            assert_same_bits(p[n].grad, d.grads[n], f"{name}: gradient of {n}")
    for n in ("s1", "s2", "s3", "sd"):
        assert p[n] is None or p[n].grad is None, "the scales are frozen"
    if k.stride == 2:
        assert_odd_positions_are_plus_zero(x.grad, name)


@pytest.mark.parametrize("name", [k.id for k in bb.BLOCKS])
def test_bottleneck_without_an_input_gradient_returns_none_and_keeps_the_other_bits(ops, layers, name, monkeypatch):
    k = bb.block_case(name)
    d = bb.build_block(k)
    calls = []
    real = ops.conv_bn_act_backward
    monkeypatch.setattr(ops, "conv_bn_act_backward", lambda *a, **kw: calls.append(tuple(kw["needs"])) or real(*a, **kw))
    monkeypatch.setattr(ops, "dilate2_sum", lambda *a, **kw: pytest.fail("no dx: nothing to dilate"))
    x, p, y = block_on_gpu(layers, k, d, x_grad=False, frozen=("w2",))
    y.backward(dev(d.dy))
    torch.cuda.synchronize()
    assert x.grad is None and p["w2"].grad is None
    for n in bb.BLOCK_PARAMS:
        if p[n] is not None and n != "w2":
            assert_same_bits(p[n].grad, d.grads[n], f"{name}: gradient of {n}")
    # conv3, conv2, conv1 (, downsample): no dx of the block's input, no dw of the frozen weight
    assert calls[1][1] is False and calls[2][0] is False and (len(calls) == 3 or calls[3][0] is False), calls


def test_a_chain_of_blocks_pool_and_strided_conv_gives_the_float64_graphs_gradients(ops, layers):
    d = bb.build_chain()
    ka, kb = bb.CHAIN_BLOCKS
    x = dev(d.x).requires_grad_(True)
    on = lambda p: {n: (None if v is None else (dev(v).requires_grad_(True) if n in bb.BLOCK_PARAMS else dev(v))) for n, v in p.items()}
    pa, pb = on(d.pa), on(d.pb)
    wc, tc = dev(d.wc).requires_grad_(True), dev(d.tc).requires_grad_(True)
    order = ("w1", "s1", "t1", "w2", "s2", "t2", "w3", "s3", "t3", "wd", "sd", "td")
    ya = layers.bottleneck(x, *[pa[n] for n in order], stride=2)
    yb = layers.bottleneck(ya, *[pb[n] for n in order])
    p6 = layers.maxpool(yb, 1, 2)
    y = layers.conv_bn_act(p6, wc, None, tc, stride=2)
    for got, want, what in ((ya, d.mids[0], "block a"), (yb, d.mids[1], "block b"), (p6, d.mids[2], "P6"), (y, d.y, "the output")):
        assert_same_bits(got, want, what)
    y.backward(dev(d.dy))
    torch.cuda.synchronize()
    got = {"x": x.grad, "wc": wc.grad, "tc": tc.grad}
    got.update({f"a.{n}": pa[n].grad for n in bb.BLOCK_PARAMS if pa[n] is not None})
    got.update({f"b.{n}": pb[n].grad for n in bb.BLOCK_PARAMS if pb[n] is not None})
    assert set(got) == set(d.grads)
    for n, want in d.grads.items():
        assert_same_bits(got[n], want, f"gradient of {n}")


# --------------------------------------------------------------------------------------------------------------- rounded data
@pytest.mark.parametrize("name", bb.ROUNDED)
def test_rounded_data_within_the_bound_of_a_recursive_fp32_sum(ops, name):
    """No activation and no scale: z is dy, so dw is a function of (x, dy) alone. A chunk's element is a recursive fp32 sum of L
    products (error <= L u sum |z||x| to first order, one u more for each product's fused rounding being the sum's own), the fp64
    sum of the chunks is exact to 2^-53 and the narrowing adds one u: (L + 2) u sum |z||x|, as tests/test_gpu_conv_backward.py
    derives it."""
    c = bb.conv_case(name)
    d = bb.build_conv_rounded(c)
    r = ops.conv_bn_act_backward(dev(d["dy"]), dev(d["x"]), dev(d["w"]), None, None, c.pad, 0, needs=(c.pointwise, True, True, False),
                                 stride=2)
    torch.cuda.synchronize()
    x64, w64, z64 = d["x"].to(F64), d["w"].to(F64), d["dy"].to(F64)
    dx64, dw64 = bb.conv_grads64(x64, w64, z64, c.pad, 2)
    sum_zw, sum_zx = bb.conv_grads64(x64.abs(), w64.abs(), z64.abs(), c.pad, 2)
    L = bb.chunk_of(c)
    dw_err, dw_bound = (r.dw.cpu().to(F64) - dw64).abs(), (L + 2) * U * sum_zx
    print(f"{name}: L {L}, chunks {-(-c.m // L)}; max |dw - dw64| / bound {float((dw_err / dw_bound).max()):.4f}")
    assert float(sum_zx.min()) > 0
    assert bool((dw_err <= dw_bound).all()), f"{name}: dw outside (L + 2) u sum|z||x| at {int((dw_err > dw_bound).sum())} elements"
    g64 = z64.reshape(-1, c.cout)
    s = g64.sum(0)
    ds_err, ds_bound = (r.dshift.cpu().to(F64) - s).abs(), U * s.abs() + g64.shape[0] * 2.0 ** -53 * g64.abs().sum(0)
    assert bool((ds_err <= ds_bound).all()), f"{name}: dshift outside u |s| + n 2^-53 sum|g|"
    if c.pointwise:      # a chain of Cout4 fmaf per element, then the dilation's copy
        full = ops.dilate2_sum(r.dx, None, c.h, c.w).cpu().to(F64)
        dx_err, dx_bound = (full - dx64).abs(), (c.cout4 + 2) * U * sum_zw
        assert bool((dx_err <= dx_bound).all()), f"{name}: dx outside (Cout4 + 2) u sum|z||w|"


# ----------------------------------------------------------------------------------------------------------------- properties
def rounded_call(ops, c, d, rows=slice(None)):
    r = ops.conv_bn_act_backward(dev(d["dy"][rows]), dev(d["x"][rows]), dev(d["w"]), None, None, c.pad, 0, stride=2)
    full = ops.dilate2_sum(r.dx, None, c.h, c.w)
    torch.cuda.synchronize()
    return r, full


def test_two_calls_give_equal_bits(ops):
    c = bb.conv_case(bb.MULTI_CHUNK)
    d = bb.build_conv_rounded(c)
    (a, fa), (b, fb) = rounded_call(ops, c, d), rounded_call(ops, c, d)
    for name in ("dx", "dw", "dshift"):
        assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    assert torch.equal(bits(fa), bits(fb))


def test_dx_of_an_image_does_not_depend_on_the_rest_of_the_batch(ops):
    c = bb.conv_case(bb.MULTI_CHUNK)
    d = bb.build_conv_rounded(c)
    _, whole = rounded_call(ops, c, d)
    for i in range(c.b):
        _, alone = rounded_call(ops, c, d, rows=slice(i, i + 1))
        assert torch.equal(bits(alone), bits(whole[i:i + 1])), f"image {i}"


def test_stride_1_through_the_new_keyword_is_the_existing_call(ops):
    c = bb.conv_case("3x3_s2")
    d = bb.build_conv_rounded(c)
    x, w = dev(d["x"]), dev(d["w"])
    dy = torch.randn(c.b, c.h, c.w, c.cout, device=DEV)
    a = ops.conv_bn_act_backward(dy, x, w, None, None, c.pad)
    b = ops.conv_bn_act_backward(dy, x, w, None, None, c.pad, stride=1)
    for name in ("dx", "dw", "dshift"):
        assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), name


# ------------------------------------------------------------------------------------------------------------------ arguments
def test_bad_arguments_are_refused_with_the_house_message_before_any_launch(ops, layers):
    op = ops.conv_bn_act_backward
    x, w3, w1 = torch.zeros(1, 8, 8, 8, device=DEV), torch.zeros(6, 3, 3, 8, device=DEV), torch.zeros(6, 1, 1, 8, device=DEV)
    g = torch.zeros(1, 4, 4, 6, device=DEV)
    prof = ops.CONV_PROFILE
    ops.CONV_PROFILE = []                  # every launch of a binding is booked here: it must stay empty
    try:
        with pytest.raises(RuntimeError, match="conv_bn_act_backward: stride must be 1 or 2, got 3"):
            op(g, x, w1, None, stride=3)
        with pytest.raises(RuntimeError, match=r"conv_bn_act_backward: w must be float32 \[Cout,1,1,8\] without padding for a data gradient "
                                               r"at stride 2 \(needs\[0\]\), got float32 \[6, 3, 3, 8\]"):
            op(g, x, w3, None, pad=(1, 1, 1, 1), stride=2)
        with pytest.raises(RuntimeError, match="conv_bn_act_backward: row_counts must be None at stride 2"):
            op(g, x, w1, None, row_counts=torch.zeros(4, dtype=torch.int32, device=DEV), rows_per_group=4, stride=2)
        with pytest.raises(RuntimeError, match="conv_bn_act_backward: scatter must be False at stride 2"):
            op(g, x, torch.zeros(24, 1, 1, 8, device=DEV), None, scatter=True, stride=2)
        with pytest.raises(RuntimeError, match=r"conv_bn_act_backward: grad_out must be float32 \[1,4,4,6\], got float32 \[1, 8, 8, 6\]"):
            op(torch.zeros(1, 8, 8, 6, device=DEV), x, w1, None, stride=2)
        a = torch.zeros(1, 4, 4, 8, device=DEV)
        with pytest.raises(RuntimeError, match=r"dilate2_sum: \(height, width\) must be two ints with ceil\(height / 2\) = 4 and "
                                               r"ceil\(width / 2\) = 4, got \(9, 8\)"):
            ops.dilate2_sum(a, None, 9, 8)
        with pytest.raises(RuntimeError, match=r"dilate2_sum: b must be float32 \[1,4,4,8\] or None, got float32 \[1, 4, 4, 4\]"):
            ops.dilate2_sum(a, a[..., :4], 8, 8)
        with pytest.raises(RuntimeError, match=r"dilate2_sum: a must be float32 \[B,OH,OW,C\] with C a multiple of 4"):
            ops.dilate2_sum(torch.zeros(1, 4, 4, 6, device=DEV), None, 8, 8)
        with pytest.raises(RuntimeError, match=r"dilate2_sum: out tensor out must be float32 \[1,8,8,8\] contiguous"):
            ops.dilate2_sum(a, None, 8, 8, out=torch.zeros(1, 8, 8, 4, device=DEV))
        with pytest.raises(RuntimeError, match=r"maxpool_backward: grad_out must be float32 \[1,4,4,8\], got float32 \[1, 4, 4, 6\]"):
            ops.maxpool_backward(g, x, 3, 2, (0, 0, 1, 1))
        with pytest.raises(RuntimeError, match=r"maxpool_backward: x must be float32 \[B,H,W,C\] with C a multiple of 4"):
            ops.maxpool_backward(g, x[..., :6].contiguous(), 3, 2, (0, 0, 1, 1))
        with pytest.raises(RuntimeError, match=r"maxpool_backward: kernel must be an int in 1 .. 3, got 4"):
            ops.maxpool_backward(g, x, 4, 2)
        assert ops.CONV_PROFILE == [], "a refused call launched something"
    finally:
        ops.CONV_PROFILE = prof
    # a 3x3 stride-2 layer in front of a tensor that needs a gradient: refused in the backward, by the op
    xg = x.clone().requires_grad_(True)
    y = layers.conv_bn_act(xg, w3, pad=(1, 1, 1, 1), stride=2)
    with pytest.raises(RuntimeError, match="without padding for a data gradient at stride 2"):
        y.sum().backward()


# ---------------------------------------------------------------------------------------------------------- schedule fuzzing
# The child's time limit: four times the wall time measured on the fuzzed library, rounded up to 30 s: 5.0 s (29 tests; 3 s of it
# inside pytest, the rest start-up), so 19.9 s -> 30 s.
FUZZ_TIMEOUT = 30


@pytest.mark.skipif(os.environ.get("MRCNN_SYNC_FUZZ_CHILD") == "1", reason="this IS the fuzzed child run")
def test_this_file_passes_under_schedule_fuzzing():
    """conv_wgrad_f32 hands a k tile's operands and the pixel table of the next one — whose (iy0, ix0) now carry the stride — from
    wave to wave through LDS with one barrier per k tile; on that build every wave sleeps a random time behind each barrier, and a
    hand-off that the barrier does not order fails its bit comparison there."""
    assert os.path.exists(FUZZ_LIB), f"{FUZZ_LIB} is missing: run __graft_entry__.build()"
    env = dict(os.environ, MRCNN_LIB=FUZZ_LIB, MRCNN_SYNC_FUZZ_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_backbone_backward.py", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=FUZZ_TIMEOUT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
