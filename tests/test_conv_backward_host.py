"""Host-side checks (no GPU) of the conv backward: the conditions under which its exact-data cases equal float64 bit for bit, the
chunking the cases rely on (through the library's own query), the C ABI as the header declares it, the build flags, and the
refusals that need no launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import conv_backward_cases as cb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maskrcnn_hip.h")
ENTRY_POINTS = ("mrcnn_conv_act_backward_f32", "mrcnn_conv_backward_data_f32", "mrcnn_conv_backward_weights_f32",
                "mrcnn_conv_backward_workspace_bytes", "mrcnn_conv_backward_weights_chunk")


@pytest.mark.parametrize("name", [c.id for c in cb.cases()])
def test_bit_equality_with_float64_is_a_theorem_for_the_case(name):
    c = cb.case(name)
    d = cb.build(c)
    cb.check_invariants(c, d)
    assert d.z.shape[-1] == c.cout4 and not bool(d.z[..., c.cout:].any())
    if c.counts:
        off = ~d.valid.reshape(-1)
        assert bool(off.any()) and not bool(d.z.reshape(c.m, -1)[off].any()) and not bool(d.dx.reshape(c.m, -1)[off].any())
    if c.res_div == 1:
        assert not torch.equal(d.g, d.z[..., :c.cout]) and torch.equal(d.dresidual, d.g)
    if c.res_div == 2:
        assert d.dresidual.shape == (c.b, c.out_hw[0] // 2, c.out_hw[1] // 2, c.cout)


def test_chunking_of_the_cases_through_the_librarys_query():
    names = [c.id for c in cb.cases()]
    assert len(set(names)) == len(names)
    c = cb.case("multi_chunk")
    L, chunks = cb.chunk_of(c), cb.chunks_of(c)
    oh, ow = c.out_hw
    assert c.b == 5 and oh % 2 == 1 and oh == ow and chunks >= 3 and c.m % L, (L, chunks, c.m)
    assert not {i * L for i in range(1, chunks)} & {i * oh * ow for i in range(1, c.b)}, "a chunk boundary on an image boundary"
    smaller = cb.Case("smaller", 5, c.h - 2, c.w - 2, 8, 8, (3, 3), (1, 1, 1, 1))
    assert cb.chunks_of(smaller) < 3 or smaller.m % cb.chunk_of(smaller) == 0, "multi_chunk is not the smallest such map"
    singles = [k for k in cb.cases() if k.single]
    assert len(singles) >= 3 and all("single" in k.id for k in singles)
    for k in cb.cases():
        assert k.single == ("single" in k.id)
        if k.single:
            assert cb.chunks_of(k) == 1, k.id
    assert cb.chunks_of(cb.case("3x3_ragged")) >= 2 and cb.chunks_of(cb.case("rows")) >= 2
    # a function of the shape only: the layers of the microbenchmark, on any machine
    from maskrcnn_amd import ops
    assert ops.conv_backward_chunk(800, 14, 14, 256, 256, 3, 3, (1, 1, 1, 1)) % 32 == 0
    assert ops.conv_backward_chunk(800, 1, 1, 12544, 1024, 1, 1) == 800      # 784 tiles: one chunk
    with pytest.raises(RuntimeError, match="conv_backward_chunk: the conv backward refuses these arguments .*pad larger than the kernel size - 1"):
        ops.conv_backward_chunk(1, 8, 8, 8, 8, 3, 3, (3, 1, 1, 1))
    with pytest.raises(RuntimeError, match=r"Cin %% 4 == 0 required|Cin % 4 == 0 required"):
        ops.conv_backward_chunk(1, 8, 8, 6, 8, 3, 3, (1, 1, 1, 1))


def test_header_declares_and_the_library_exports_the_entry_points():
    from maskrcnn_amd import _lib
    text = open(HEADER).read()
    declared, protos = _lib.declared_symbols(), _lib.header_prototypes()
    for name in ENTRY_POINTS:
        assert name in declared and name in protos and hasattr(_lib.lib, name), name
        assert getattr(_lib.lib, name).argtypes == protos[name][1]
    assert _lib.header_abi_version() >= 30 and int(_lib.lib.mrcnn_abi_version()) == _lib.header_abi_version()
    for phrase in ("No gradient of `scale` is produced", "fmaf chain over the chunk's pixels in ascending order",
                   "are never read into the arithmetic", "(g00 + g01) + (g10 + g11)"):
        assert phrase in text, phrase
    i32, vp = _lib.c_i32, _lib.c_vp
    assert protos["mrcnn_conv_backward_weights_chunk"] == (i32, [i32] * 12)
    assert protos["mrcnn_conv_backward_workspace_bytes"] == (ctypes.c_size_t, [i32] * 12)
    assert protos["mrcnn_conv_backward_weights_f32"] == (ctypes.c_int, [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32,
                                                                      vp, i32, vp, vp, ctypes.c_size_t, vp])
    # the workspace holds the chunk sums: ceil(M / L) * Cout * KH*KW*Cin floats where that is the largest of the three uses
    c = cb.case("3x3_pow2")
    assert int(_lib.lib.mrcnn_conv_backward_workspace_bytes(*c.shape_args)) == 4 * cb.chunks_of(c) * c.cout * 9 * c.cin
    assert int(_lib.lib.mrcnn_conv_backward_workspace_bytes(0, 1, 1, 4, 4, 1, 1, 1, 0, 0, 0, 0)) == 0


def test_the_kernel_file_is_built_without_contraction_and_has_no_atomic_or_assembly():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_b", os.path.join(ROOT, "maskrcnn_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "-ffp-contract=off" in b.SOURCES["conv_backward.hip"]
    text = open(os.path.join(b.CSRC, "conv_backward.hip")).read()
    code = re.sub(r"//.*", "", text)
    assert "atomic" not in code and not re.search(r"\basm\b", code) and "hipMalloc" not in code and "Synchronize" not in code
    assert code.index('#include "conv_common.hpp"') < code.index("__syncthreads()")
    for kernel in ("conv_act_backward", "conv_weight_flip", "conv_wgrad_f32", "conv_wgrad_reduce"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\(", code), kernel
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in code


def test_bad_arguments_are_refused_before_any_launch():
    import maskrcnn_amd
    from maskrcnn_amd import layers, ops
    assert maskrcnn_amd.layers is layers
    assert "conv_bn_act_backward" not in ops.__all__ and not hasattr(torch.ops.maskrcnn, "conv_bn_act_backward")
    x, w, g = torch.zeros(1, 4, 4, 8), torch.zeros(6, 3, 3, 8), torch.zeros(1, 4, 4, 6)
    op = ops.conv_bn_act_backward
    with pytest.raises(RuntimeError, match=r"conv_bn_act_backward: act must be 0 \(none\), 1 \(ReLU\) or 2 \(sigmoid\), got 3"):
        op(g, x, w, g, pad=(1, 1, 1, 1), act=3)
    with pytest.raises(RuntimeError, match=r"conv_bn_act_backward: res_div must be 0 \(no residual\), 1 or 2, got 4"):
        op(g, x, w, g, pad=(1, 1, 1, 1), res_div=4)
    with pytest.raises(RuntimeError, match="conv_bn_act_backward: act must be 0 or 1 with a residual or the scatter"):
        op(g, x, w, g, pad=(1, 1, 1, 1), act=2, res_div=1)
    with pytest.raises(RuntimeError, match="conv_bn_act_backward: needs must hold 4 flags"):
        op(g, x, w, g, pad=(1, 1, 1, 1), needs=(True, True))
    with pytest.raises(RuntimeError, match="conv_bn_act_backward: needs must be without dresidual where res_div is 0"):
        op(g, x, w, g, pad=(1, 1, 1, 1), needs=(True, True, True, True))
    with pytest.raises(RuntimeError, match=r"conv_bn_act_backward: x must be float32 \[B>=1,H>=1,W>=1,Cin>=4\], got None"):
        op(g, None, w, g, pad=(1, 1, 1, 1))
    # CPU tensors: the refusal every op without a staged CPU form gives
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        op(g, x, w, g, pad=(1, 1, 1, 1))
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        layers.conv_bn_act(x.requires_grad_(True), w, pad=(1, 1, 1, 1))
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        layers.deconv2x2(x, torch.zeros(8, 1, 1, 8), torch.zeros(8))


def test_the_scatter_relabelling_and_the_reference_agree_with_conv_transpose2d():
    """The reference works on GEMM columns; scatter_nhwc must be the transposed conv's pixel order, or the scatter case tests a
    relabelling of its own."""
    rng = np.random.default_rng(1)
    b, h, w, cin, c = 2, 3, 4, 8, 5
    x = torch.from_numpy(rng.integers(-4, 5, (b, h, w, cin)).astype(np.float64))
    w4 = torch.from_numpy(rng.integers(-3, 4, (4 * c, 1, 1, cin)).astype(np.float64))
    wt = w4.reshape(2, 2, c, cin).permute(3, 2, 0, 1)                         # [Cin][C][dy][dx]
    want = torch.nn.functional.conv_transpose2d(x.permute(0, 3, 1, 2), wt, stride=2).permute(0, 2, 3, 1)
    got = cb.scatter_nhwc(cb.conv64(x, w4, (0, 0, 0, 0)))
    assert torch.equal(got, want) and torch.equal(cb.gather_nhwc(got), cb.conv64(x, w4, (0, 0, 0, 0)))
