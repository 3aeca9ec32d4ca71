"""Host-side checks (no GPU) of the backbone backward: the conditions under which its exact-data cases equal float64 bit for bit,
the numpy restatements of the two new rules against float64 autograd, the strided chunking (through the library's own query), the
C ABI as the header declares it, the build flags, and the refusals that need no launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import backbone_backward_cases as bb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maskrcnn_hip.h")
ENTRY_POINTS = ("mrcnn_conv_backward_weights_f32", "mrcnn_conv_backward_data_f32", "mrcnn_conv_backward_workspace_bytes",
                "mrcnn_conv_backward_weights_chunk", "mrcnn_dilate2_sum_f32", "mrcnn_maxpool_backward_f32")


# ------------------------------------------------------------------------------------------------------ exactness conditions
@pytest.mark.parametrize("name", [c.id for c in bb.CONVS])
def test_bit_equality_with_float64_is_a_theorem_for_the_conv_case(name):
    c = bb.conv_case(name)
    d = bb.build_conv(c)
    bb.check_conv(c, d)
    assert c.stride == 2 and d.z.shape == (c.b, *c.out_hw, c.cout4) and not bool(d.z[..., c.cout:].any())
    assert d.dx.shape == (c.b, c.h, c.w, c.cin)


@pytest.mark.parametrize("name", [k.id for k in bb.BLOCKS])
def test_bit_equality_with_float64_is_a_theorem_for_the_block_case(name):
    k = bb.block_case(name)
    d = bb.build_block(k)
    bb.check_block(k, d)
    assert d.y.shape == (k.b, *k.out_hw, 4 * k.planes) and len(d.tape) == (4 if k.down else 3)


def test_bit_equality_with_float64_is_a_theorem_for_the_chain():
    d = bb.build_chain()
    bb.check_chain(d)
    assert len(d.tape) == 8 and d.y.shape == (2, 2, 2, bb.CHAIN_COUT) and d.mids[2].shape == (2, 3, 3, 16)


def test_the_cases_are_the_shapes_the_mechanisms_need():
    shapes = {c.id: (c.h % 2, c.w % 2) for c in bb.CONVS if c.pointwise}
    assert (1, 1) in shapes.values() and (0, 0) in shapes.values()                 # H and W each odd in one case, even in another
    assert any(c.cout % 4 for c in bb.CONVS) and any(c.k == (7, 7) and c.cin == 4 for c in bb.CONVS)
    assert {(h % 2, w % 2) for _, h, w, _ in bb.DILATE_SHAPES} >= {(1, 1), (0, 0), (0, 1)}
    assert bb.pool_case("3x3_s2_odd").pad == (1, 1, 1, 1) and bb.pool_case("3x3_s2_even").pad == (0, 0, 1, 1)
    assert [k.stride for k in bb.BLOCKS] == [1, 1, 2] and [k.down for k in bb.BLOCKS] == [False, True, True]


# ------------------------------------------------------------------------------------------------------ numpy restatements
@pytest.mark.parametrize("shape", bb.DILATE_SHAPES)
def test_dilate2_sum_restated_in_numpy_equals_float64_autograd(shape):
    _, h, w, _ = shape
    a, b = bb.dilate_operands(shape)
    for second in (None, b):
        want = bb.dilate2_sum64(a, second, h, w)
        got = bb.dilate2_sum_np(a.numpy(), None if second is None else second.numpy(), h, w)
        assert np.array_equal(got, want.numpy())
        assert not got[:, 1::2].any() and not got[:, :, 1::2].any() and got.any()
    # the same through F.conv2d: the data gradient of a 1x1 stride-2 conv is its compact gradient at the even positions
    c = bb.conv_case("1x1_s2_odd")
    d = bb.build_conv(c)
    compact, _ = bb.conv_grads64(d.x[:, ::2, ::2], d.w, d.z[..., :c.cout], c.pad, 1)
    assert np.array_equal(bb.dilate2_sum_np(compact.numpy(), None, c.h, c.w), d.dx.numpy())


@pytest.mark.parametrize("name", [p.id for p in bb.POOLS])
def test_the_max_pool_rule_restated_in_numpy_equals_float64_autograd(name):
    p = bb.pool_case(name)
    x, dy = bb.pool_operands(p)
    want = bb.pool_grad64(p, x, dy)
    got, dropped = bb.maxpool_backward_np(x.numpy(), dy.numpy(), p.kernel, p.stride, p.pad, np.float64)
    assert np.array_equal(got, want.numpy())
    got32, _ = bb.maxpool_backward_np(x.numpy(), dy.numpy(), p.kernel, p.stride, p.pad)
    assert got32.dtype == np.float32 and np.array_equal(got32.astype(np.float64), want.numpy())      # integer gradients: exact in fp32
    if p.kernel == 1:
        assert dropped == 0 and np.array_equal(got, bb.dilate2_sum_np(dy.numpy(), None, p.h, p.w))     # P6 is a dilation
        return
    # the data hold what the rule is about: ties, zero windows, windows whose padding tap wins, overlapping windows that add
    y = bb.pool64(x, p.kernel, p.stride, p.pad)
    pt, pl, _, _ = p.pad
    assert dropped > 0 and float(want.abs().sum()) < float(dy.abs().sum())
    zero, neg = want[..., 1], want[..., 2]
    assert not bool(y[..., 1].any()) and bool(zero.any())                          # all-zero windows: the first tap, real or padding
    if pt and pl:       # padding in front of the real taps takes every border window's gradient; the interior windows keep theirs
        assert not bool(zero[:, 0].any()) and not bool(zero[:, :, 0].any()) and float(zero.abs().sum()) < float(dy[..., 1].abs().sum())
    else:               # padding behind the real taps alone: the first real zero is taken, nothing is dropped
        assert float(zero.sum()) == float(dy[..., 1].sum()) and bool(zero[:, -2].any())
    assert bool((x[..., 2] < 0).all()) and bool(neg.any())                         # interior windows of the negative plane: a real tap
    assert not bool(y[:, -1, :, 2].any()) and not bool(neg[:, -1].any())           # ... and its border windows: the padding zero
    taken = int((want != 0).sum())
    assert taken < int((dy != 0).sum()), "no input element is taken by two windows"


def test_nan_and_ties_follow_torchs_walk():
    x = torch.tensor([0.0, 1.0, float("nan"), 1.0, 2.0, float("nan"), 2.0, 2.0, -1.0], dtype=torch.float64).reshape(1, 3, 3, 1)
    x = x.expand(1, 3, 3, 4).contiguous()
    dy = torch.full((1, 1, 1, 4), 5.0, dtype=torch.float64)
    got, dropped = bb.maxpool_backward_np(x.numpy(), dy.numpy(), 3, 1, (0, 0, 0, 0), np.float64)
    xg = x.clone().requires_grad_(True)
    bb.pool64(xg, 3, 1).backward(dy)
    assert dropped == 0 and np.array_equal(got, xg.grad.numpy()) and got[0, 1, 2, 0] == 5.0      # the LAST NaN of the walk
    ties = torch.tensor([1.0, 3.0, 3.0, 0.0, 3.0, 2.0, 3.0, 1.0, 3.0], dtype=torch.float64).reshape(1, 3, 3, 1).expand(1, 3, 3, 4).contiguous()
    got, _ = bb.maxpool_backward_np(ties.numpy(), dy.numpy(), 3, 1, (0, 0, 0, 0), np.float64)
    assert got[0, 0, 1, 0] == 5.0 and got.sum() == 20.0                                           # the first of the equal maxima


# ------------------------------------------------------------------------------------------------------------------- chunking
def test_the_chunk_function_with_a_stride_through_the_librarys_query():
    from maskrcnn_amd import ops
    for c in bb.CONVS:
        L = bb.chunk_of(c)
        assert L >= 128 and L % 32 == 0, (c.id, L)
    c = bb.conv_case(bb.MULTI_CHUNK)
    assert c.m == 512 and bb.chunk_of(c) == 128 and -(-c.m // bb.chunk_of(c)) == 4
    # the stride enters through M = B*OH*OW alone: stride 1 is the default (8 tiles of 128 x 128: 64 chunks of the 8192 pixels),
    # and a stride-2 1x1 layer has the chunk of the stride-1 layer on its output map
    args = (2, 64, 64, 256, 512, 1, 1)
    assert ops.conv_backward_chunk(*args, stride=1) == ops.conv_backward_chunk(*args) == 128
    assert ops.conv_backward_chunk(*args, stride=2) == ops.conv_backward_chunk(2, 32, 32, 256, 512, 1, 1)
    assert ops.conv_backward_chunk(2, 63, 63, 256, 512, 1, 1, stride=2) == ops.conv_backward_chunk(2, 32, 32, 256, 512, 1, 1)
    assert ops.conv_backward_chunk(2, 1024, 1024, 4, 64, 7, 7, (3, 3, 3, 3), stride=2) % 32 == 0       # the stem
    with pytest.raises(RuntimeError, match="conv_backward_chunk: stride must be 1 or 2, got 3"):
        ops.conv_backward_chunk(*args, stride=3)
    with pytest.raises(RuntimeError, match="conv_backward_chunk: the conv backward refuses these arguments .*pad larger than the kernel size - 1"):
        ops.conv_backward_chunk(1, 8, 8, 8, 8, 3, 3, (3, 1, 1, 1), stride=2)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_and_the_library_exports_the_entry_points():
    from maskrcnn_amd import _lib
    text = open(HEADER).read()
    declared, protos = _lib.declared_symbols(), _lib.header_prototypes()
    for name in ENTRY_POINTS:
        assert name in declared and name in protos and hasattr(_lib.lib, name), name
        assert getattr(_lib.lib, name).argtypes == protos[name][1]
    # one set of entry points, the stride an argument of the four above: no conv name that carries the stride is declared, spoken of
    # or exported (the library's symbol table and its message strings)
    with_stride = re.compile(r"conv_\w*strided")
    assert not with_stride.search(text) and not [n for n in declared if with_stride.search(n)]
    assert not re.search(with_stride.pattern.encode(), open(_lib.LIB_PATH, "rb").read())
    assert _lib.header_abi_version() >= 35 and int(_lib.lib.mrcnn_abi_version()) == _lib.header_abi_version()
    for phrase in ("the first of equal maxima wins", "a padding tap loses the gradient", "the LAST NaN of a window",
                   "Every byte of dx is\n *           written exactly once", "a + b2 as ONE fp32\n *           add",
                   "in ascending (oy, ox) order", "it depends on the stride through M = B*OH*OW"):
        assert phrase in text, phrase
    i32, vp, sz = _lib.c_i32, _lib.c_vp, ctypes.c_size_t
    # the stride comes directly after kw, where the forward has it; the weight gradient alone takes row counts
    assert protos["mrcnn_conv_backward_weights_chunk"] == (i32, [i32] * 12)
    assert protos["mrcnn_conv_backward_workspace_bytes"] == (sz, [i32] * 12)
    assert protos["mrcnn_conv_backward_weights_f32"] == (ctypes.c_int, [vp] + [i32] * 4 + [vp] + [i32] * 8 + [vp, i32, vp, vp, sz, vp])
    assert protos["mrcnn_conv_backward_data_f32"] == (ctypes.c_int, [vp] + [i32] * 4 + [vp] + [i32] * 8 + [vp, vp, sz, vp])
    assert protos["mrcnn_dilate2_sum_f32"] == (ctypes.c_int, [vp, vp, i32, i32, i32, i32, vp, vp])
    assert protos["mrcnn_maxpool_backward_f32"] == (ctypes.c_int, [vp, vp] + [i32] * 10 + [vp, vp])
    # queries: at stride 1 the workspace holds the ceil(M / L) chunk sums of Cout * KH*KW*Cin floats; a refused stride answers 0
    from maskrcnn_amd import ops
    lib = _lib.lib
    chunks = -(-2 * 16 * 16 // ops.conv_backward_chunk(2, 16, 16, 64, 64, 3, 3, (1, 1, 1, 1)))
    assert chunks == 4
    assert int(lib.mrcnn_conv_backward_workspace_bytes(2, 16, 16, 64, 64, 3, 3, 1, 1, 1, 1, 1)) == chunks * 64 * 9 * 64 * 4
    assert int(lib.mrcnn_conv_backward_workspace_bytes(2, 16, 16, 64, 64, 3, 3, 3, 1, 1, 1, 1)) == 0
    assert int(lib.mrcnn_conv_backward_weights_chunk(2, 16, 16, 64, 64, 3, 3, 0, 1, 1, 1, 1)) == 0
    assert b"stride must be 1 or 2" in lib.mrcnn_last_error()


def test_the_library_refuses_bad_arguments_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail with another message (or crash on the null pointers)."""
    from maskrcnn_amd._lib import lib
    err = lambda: lib.mrcnn_last_error().decode()
    assert lib.mrcnn_conv_backward_data_f32(None, 1, 8, 8, 8, None, 8, 3, 3, 2, 1, 1, 1, 1, None, None, 0, None) != 0
    assert "the stride-2 data gradient covers the 1 x 1 kernel without padding, got 3 x 3 with pads (1, 1, 1, 1)" in err()
    assert lib.mrcnn_conv_backward_data_f32(None, 1, 8, 8, 8, None, 8, 1, 1, 4, 0, 0, 0, 0, None, None, 0, None) != 0
    assert "stride must be 1 or 2, got 4" in err()
    assert lib.mrcnn_conv_backward_weights_f32(None, 1, 8, 8, 6, None, 8, 1, 1, 2, 0, 0, 0, 0, None, 0, None, None, 0, None) != 0
    assert "Cin % 4 == 0 required" in err()
    assert lib.mrcnn_conv_backward_weights_f32(None, 1, 8, 8, 8, None, 8, 1, 1, 2, 0, 0, 0, 0, None, 0, None, None, 0, None) != 0
    assert "null pointer" in err()
    # row counts at stride 2 (a dummy non-null pointer: never dereferenced on the host, and no launch is reached)
    assert lib.mrcnn_conv_backward_weights_f32(None, 1, 8, 8, 8, None, 8, 1, 1, 2, 0, 0, 0, 0, 16, 4, None, None, 0, None) != 0
    assert "row counts need stride 1" in err()
    assert lib.mrcnn_dilate2_sum_f32(None, None, 1, 5, 5, 6, None, None) != 0 and "C % 4 == 0 required" in err()
    assert lib.mrcnn_dilate2_sum_f32(None, None, 1, 5, 5, 8, None, None) != 0 and "null pointer" in err()
    assert lib.mrcnn_dilate2_sum_f32(None, None, 1 << 14, 1 << 10, 1 << 10, 8, None, None) != 0 and "tensor too large" in err()
    assert lib.mrcnn_maxpool_backward_f32(None, None, 1, 8, 8, 8, 4, 2, 0, 0, 0, 0, None, None) != 0
    assert "kernel must be in 1 .. 3 and stride in 1 .. 2, got 4 and 2" in err()
    assert lib.mrcnn_maxpool_backward_f32(None, None, 1, 8, 8, 8, 3, 3, 0, 0, 0, 0, None, None) != 0 and "stride in 1 .. 2" in err()
    assert lib.mrcnn_maxpool_backward_f32(None, None, 1, 8, 8, 8, 3, 2, 3, 0, 0, 0, None, None) != 0
    assert "every pad must be in 0 .. kernel - 1" in err()
    assert lib.mrcnn_maxpool_backward_f32(None, None, 1, 8, 8, 6, 3, 2, 0, 0, 1, 1, None, None) != 0 and "C % 4 == 0 required" in err()
    assert lib.mrcnn_maxpool_backward_f32(None, None, 1, 8, 8, 8, 3, 2, 0, 0, 1, 1, None, None) != 0 and "null pointer" in err()


def test_the_kernel_files_are_built_without_contraction_and_have_no_atomic_or_memset():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_b", os.path.join(ROOT, "maskrcnn_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "-ffp-contract=off" in b.SOURCES["pool_backward.hip"] and "-ffp-contract=off" in b.SOURCES["conv_backward.hip"]
    code = re.sub(r"//.*", "", open(os.path.join(b.CSRC, "pool_backward.hip")).read())
    for word in ("atomic", "hipMemset", "hipMalloc", "Synchronize", "__syncthreads", "__shared__"):
        assert word not in code, word
    assert not re.search(r"\basm\b", code)
    for kernel in ("dilate2_sum", "maxpool_backward"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\(", code), kernel
    assert code.count("reinterpret_cast<float4*>(p.dx)[e] =") == 2, "one 16-byte store per thread is all that writes dx"


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_are_refused_before_any_launch():
    from maskrcnn_amd import layers, ops
    for name in ("dilate2_sum", "maxpool_backward"):
        assert name not in ops.__all__ and not hasattr(torch.ops.maskrcnn, name) and callable(getattr(ops, name))
    assert layers.__all__ == ["conv_bn_act", "deconv2x2", "maxpool", "bottleneck"]
    x, w, g = torch.zeros(1, 8, 8, 8), torch.zeros(6, 3, 3, 8), torch.zeros(1, 4, 4, 6)
    op = ops.conv_bn_act_backward
    with pytest.raises(RuntimeError, match="conv_bn_act_backward: stride must be 1 or 2, got 3"):
        op(g, x, w, None, pad=(1, 1, 1, 1), stride=3)
    with pytest.raises(RuntimeError, match="conv_bn_act_backward: stride must be 1 or 2, got 2.0"):
        op(g, x, w, None, pad=(1, 1, 1, 1), stride=2.0)
    with pytest.raises(RuntimeError, match="dilate2_sum: a must be float32 .B>=1,OH>=1,OW>=1,C>=4., got None"):
        ops.dilate2_sum(None, None, 4, 4)
    with pytest.raises(RuntimeError, match=r"maxpool_backward: kernel must be an int in 1 .. 3, got 4"):
        ops.maxpool_backward(g, x, 4, 2)
    with pytest.raises(RuntimeError, match=r"maxpool_backward: stride must be 1 or 2, got 3"):
        ops.maxpool_backward(g, x, 3, 3)
    with pytest.raises(RuntimeError, match=r"maxpool_backward: pad must be \(top, left, bottom, right\) in 0 .. kernel - 1 = 2, got \(3, 0, 0, 0\)"):
        ops.maxpool_backward(g, x, 3, 2, (3, 0, 0, 0))
    with pytest.raises(RuntimeError, match="conv_bn_act: stride must be 1 or 2, got 4"):
        layers.conv_bn_act(x, w, stride=4)
    with pytest.raises(RuntimeError, match="maxpool: kernel must be an int in 1 .. 3, got 5"):
        layers.maxpool(x, 5, 2)
    with pytest.raises(RuntimeError, match=r"maxpool: x must be float32 \[B,H,W,C\] with C a multiple of 4"):
        layers.maxpool(x[..., :6], 3, 2)
    w1, w2, w3 = torch.zeros(4, 1, 1, 8), torch.zeros(4, 3, 3, 4), torch.zeros(16, 1, 1, 4)
    s, t, s4, t4 = torch.ones(4), torch.zeros(4), torch.ones(16), torch.zeros(16)
    with pytest.raises(RuntimeError, match="bottleneck: stride must be 1 or 2, got 3"):
        layers.bottleneck(x, w1, s, t, w2, s, t, w3, s4, t4, stride=3)
    with pytest.raises(RuntimeError, match=r"bottleneck: wd must be a downsample weight \[16,1,1,8\] where the stride is 2 or Cin != 4 \* planes"):
        layers.bottleneck(x, w1, s, t, w2, s, t, w3, s4, t4)
    # CPU tensors: the refusal every op without a staged CPU form gives
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.dilate2_sum(torch.zeros(1, 2, 2, 4), None, 4, 4)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.maxpool_backward(torch.zeros(1, 4, 4, 8), x, 3, 2, (0, 0, 1, 1))
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        layers.maxpool(x.requires_grad_(True), 3, 2, (0, 0, 1, 1))
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        layers.bottleneck(x, w1, s, t, w2, s, t, w3, s4, t4, torch.zeros(16, 1, 1, 8), s4, t4, stride=2)
