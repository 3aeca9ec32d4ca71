"""CPU tests of the boundary: the C-ABI library loads and exports every symbol include/*.h declares
(no compute without a GPU), the drop-in `maskrcnn` package has the reference's surface, and the
product never touches oracle/."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from maskrcnn_amd import _lib
    names = _lib.declared_symbols()
    assert len(names) >= 10
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/maskrcnn_hip.h but not exported"
    assert set(_lib._SIGS) == set(names), "ctypes table and header disagree"
    assert _lib.lib.mrcnn_abi_version() == _lib.header_abi_version() >= 2
    assert _lib.lib.mrcnn_arch() == b"gfx950"


def test_ctypes_table_matches_header_prototypes():
    """_SIGS is a hand-kept copy of the header: argument counts and types are cross-checked against the prototypes
    (a mismatch would pass wrong-width arguments to a kernel launch)."""
    from maskrcnn_amd import _lib
    protos = _lib.header_prototypes()
    assert set(protos) == set(_lib._SIGS)
    for name, (res, args) in _lib._SIGS.items():
        hres, hargs = protos[name]
        assert res == hres, f"{name}: return type {res} vs header {hres}"
        assert len(args) == len(hargs), f"{name}: {len(args)} arguments vs {len(hargs)} in the header"
        for i, (a, h) in enumerate(zip(args, hargs)):
            assert a == h, f"{name}: argument {i} is {a} in _SIGS, {h} in the header"


def test_stale_library_is_rejected(tmp_path, monkeypatch):
    """An .so built from another revision of the header must not load (same names, other argument lists)."""
    from maskrcnn_amd import _lib
    fake = tmp_path / "maskrcnn_hip.h"
    fake.write_text(open(_lib.HEADER).read().replace(f"#define MRCNN_ABI_VERSION {_lib.header_abi_version()}",
                                                     "#define MRCNN_ABI_VERSION 9999"))
    monkeypatch.setattr(_lib, "HEADER", str(fake))
    monkeypatch.setattr(_lib, "header_abi_version", lambda header=str(fake): 9999)
    with pytest.raises(ImportError, match="ABI version"):
        _lib._load()


def test_inference_config_validates_kernel_limits():
    from maskrcnn_amd.config import InferenceConfig
    InferenceConfig(pre_nms_limit=4096, proposal_count=1000)
    for kw in (dict(pre_nms_limit=6000), dict(proposal_count=5000, pre_nms_limit=4096), dict(detection_max_instances=0),
               dict(backbone="resnet18"), dict(image_height=1000)):
        with pytest.raises(ValueError):
            InferenceConfig(**kw)


def test_dropin_surface_matches_reference():
    import maskrcnn
    assert callable(maskrcnn.nms) and callable(maskrcnn.CropFunction(7, 7, 0))
    for name in ("nms", "crop_forward", "crop_backward"):  # csrc/vision.cpp:11-15
        assert callable(getattr(maskrcnn._C, name))
    for name in ("nms", "crop_forward", "crop_backward", "crop"):
        assert hasattr(torch.ops.maskrcnn, name)
    f = maskrcnn.CropFunction(14, 14)
    assert (f.crop_height, f.crop_width, f.extrapolation_value) == (14, 14, 0)


def test_cpu_tensors_without_a_gpu_fail_loudly():
    """CPU tensors are staged through the GPU (tests/test_gpu_ops.py::test_cpu_tensors_through_the_dropin); there is no CPU
    arithmetic in the product, so without a visible GPU the call must raise — never fall back to anything."""
    import maskrcnn
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: the staged path runs (covered under -m gpu)")
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        maskrcnn.nms(torch.rand(4, 5), 0.5)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        maskrcnn.CropFunction(2, 2)(torch.zeros(1, 1, 4, 4), torch.zeros(1, 4),
                                    torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        torch.ops.maskrcnn.conv_bn_act(torch.zeros(1, 4, 4, 32), torch.zeros(32, 1, 1, 32), None, None, 1, [0, 0, 0, 0], False,
                                       None, 1)


def test_product_never_imports_oracle():
    pat = re.compile(r"^\s*(from|import)\s+oracle\b|oracle[./]|liboracle", re.M)
    for pkg in ("maskrcnn_amd", "maskrcnn"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, pkg)):
            for f in files:
                if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                    text = open(os.path.join(dirpath, f)).read()
                    assert not pat.search(text), f"{pkg}/{f} references oracle/"


def test_entry_points_refuse_tensors_beyond_32bit_offsets():
    """Argument validation runs before any HIP call (no GPU needed, the pointers are never touched): the fp32 stem + pool entry
    point writes 16 B per input pixel through 32-bit buffer byte offsets — 256 images of 1024 x 1024 (2^28 pixels, a 4 GiB
    output) must be refused, not wrapped (round-5 advice)."""
    from maskrcnn_amd import _lib
    lib = _lib.lib
    dummy = ctypes.c_void_p(16)
    rc = lib.mrcnn_stem_conv7x7_s2_pool_f32(dummy, 256, 1024, 1024, dummy, None, None, dummy, None)
    assert rc != 0 and b"too large" in lib.mrcnn_last_error()
    rc = lib.mrcnn_conv3x3_winograd4_f32(dummy, 1, 64, 64, 12, dummy, 64, None, None, 1, dummy, None, None)
    assert rc != 0 and b"Cin" in lib.mrcnn_last_error()


def test_native_cxx_module_loads_and_registers():
    """maskrcnn/_C_native.so (maskrcnn/csrc/vision_hip.cpp): the reference's pybind module — the three names and doc strings of
    c++ext/maskrcnn/csrc/vision.cpp:11-15 — built on the C ABI, plus the TORCH_LIBRARY registration maskrcnn_native::* a C++ /
    TorchScript caller uses. No GPU here: it must import, expose the functions and the dispatcher schemas, and refuse CPU tensors
    the way the reference built without CPU support would (nms.h:24)."""
    from maskrcnn import build_native
    build_native.build()
    m = build_native.load()
    assert m.nms.__doc__.strip().endswith("non-maximum suppression")
    assert m.crop_forward.__doc__.strip().endswith("crop forward") and m.crop_backward.__doc__.strip().endswith("crop backward")
    s = torch.ops.maskrcnn_native.nms.default._schema
    assert str(s) == "maskrcnn_native::nms(Tensor dets, float threshold) -> Tensor"
    assert "Tensor(a!) crops" in str(torch.ops.maskrcnn_native.crop_forward.default._schema)
    assert "Tensor(a!) grads_image" in str(torch.ops.maskrcnn_native.crop_backward.default._schema)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        m.nms(torch.zeros(3, 5), 0.5)


OOB = 0xFFFFFFF0  # csrc/conv_common.hpp: the byte offset dropped loads and stores use; no descriptor's num_records may pass it


def _largest_accepted(accepts, lo: int, hi: int) -> int:
    """Largest v in [lo, hi) with accepts(v), for a predicate that holds on a prefix of the range (lo accepted, hi refused)."""
    assert accepts(lo) and not accepts(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if accepts(mid) else (lo, mid)
    return lo


def test_size_predicates_keep_every_buffer_within_the_oob_sentinel():
    """The *_supported predicates and max_batch_per_launch are host arithmetic (no HIP call). At the largest shape each one
    accepts, every buffer it sizes stays at or below OOB (0xFFFFFFF0 bytes), so a store sent to OOB is dropped; the next shape
    up is refused. Before the shared MAX_BUFFER_BYTES an fp32 tensor of 2^30 - 3 ... 2^30 - 1 elements was accepted."""
    from maskrcnn_amd import _lib
    from maskrcnn_amd.config import InferenceConfig
    from maskrcnn_amd.pipeline import MAX_BUFFER_BYTES, max_batch_per_launch
    lib = _lib.lib
    assert MAX_BUFFER_BYTES == OOB
    # F(4x4): x and y fp32 [B*H*W][C]; the width is the free size (multiples of 4)
    for cin, cout in ((8, 64), (1024, 960), (24, 192)):
        ok = lambda q: bool(lib.mrcnn_conv3x3_winograd4_supported(1, 4, 4 * q, cin, cout))
        q = _largest_accepted(ok, 1, 1 << 28)
        assert 4 * 16 * q * max(cin, cout) <= OOB < 4 * 16 * (q + 1) * max(cin, cout), (cin, cout, q)
    # the C2 fp16 bottleneck: x and y fp16 [px][256]
    for ds, cin in ((0, 256), (1, 64)):
        ok = lambda px: bool(lib.mrcnn_bottleneck_c2_f16_supported(1, 1, px, cin, 64, ds))
        px = _largest_accepted(ok, 1, 1 << 30)
        assert 512 * px <= OOB and 512 * (px + 1) >= 1 << 31, (ds, px)
    # the fp16 mask tail: x fp16 [m][256], fp32 output [m][4][classes]
    for classes in (1, 81, 96):
        ok = lambda r: bool(lib.mrcnn_mask_tail_f16_supported(r, 14, 14, 256, 256, classes))
        r = _largest_accepted(ok, 1, 1 << 24)
        for rr, accepted in ((r, True), (r + 1, False)):
            m = rr * 196
            assert (512 * m < 1 << 31 and 16 * m * classes <= OOB - 65536) == accepted, (classes, rr)
            assert not accepted or max(512 * m, 16 * m * classes) <= OOB, (classes, rr)
    # the pipelined fp16 conv: fp16 x, fp16 weights, fp32 y (the largest)
    for k, pad, cout in ((1, (0, 0, 0, 0), 64), (3, (1, 1, 1, 1), 256), (3, (0, 0, 1, 1), 128)):
        ok = lambda wd: bool(lib.mrcnn_conv_f16_pipelined_supported(1, 64, wd, 64, cout, k, k, 1, *pad))
        wd = _largest_accepted(ok, 8, 1 << 24)
        for ww, accepted in ((wd, True), (wd + 1, False)):
            oh, ow = 64 + pad[0] + pad[2] - k + 1, ww + pad[1] + pad[3] - k + 1
            ybytes, xbytes = 4 * oh * ow * cout, 2 * 64 * ww * 64
            assert (max(ybytes, xbytes) < 1 << 31) == accepted and (not accepted or max(ybytes, xbytes) <= OOB), (k, cout, ww)
    # max_batch_per_launch: every batch-scaled fp32 tensor of the step
    for h, w, p, d in ((1024, 1024, 500, 50), (832, 1344, 1000, 50), (256, 256, 1000, 50), (128, 128, 4096, 4096),
                       (64, 64, 1000, 100), (64, 64, 1, 1)):
        cfg = InferenceConfig(image_height=h, image_width=w, pre_nms_limit=p, proposal_count=p, detection_max_instances=d)
        m = max_batch_per_launch(cfg)
        nc, up, pool2 = cfg.num_classes, (2 * cfg.mask_pool_size) ** 2, cfg.pool_size ** 2
        nbytes = lambda b: 4 * max(b * (h // 4) * (w // 4) * 512, b * p * pool2 * 256, b * p * 1024, b * p * nc * 5,
                                   b * d * up * 256, b * d * up * nc, b * d * (up // 4) * 256)
        assert nbytes(m) <= OOB < nbytes(m + 1), (h, w, p, d, m)


def test_direct_conv_refuses_the_oob_sentinel_window():
    """Argument validation runs before any HIP call (the pointers are never touched). A 1x1 conv of 466 x 1103 pixels, Cin 32 ->
    Cout 2089 has M * Cout = 2^30 - 2 elements, an fp32 output of 0xFFFFFFF8 bytes: the offset OOB of the dropped stores of
    its ragged tiles would lie inside it (element 2^30 - 4 = y[M-1, 2087]). It is refused; the same call with Cout 1905 on
    4 x 113 x 1247 pixels (exactly OOB bytes) is the largest of its kind accepted (tests/test_gpu_large_tensors.py runs it)."""
    from maskrcnn_amd import _lib
    lib = _lib.lib
    dummy = ctypes.c_void_p(16)
    for b, h, w, cin, cout in ((1, 466, 1103, 32, 2089), (1, 1, (2 ** 30 - 1) // 3, 4, 3), (4, 113, 1247, 32, 1906),
                               (1, 2048, 2048, 256, 64)):
        rc = lib.mrcnn_conv_bn_act_f32(dummy, b, h, w, cin, dummy, cout, 1, 1, 1, 0, 0, 0, 0, None, None, None, 1, 0, 0, dummy,
                                       0, None)
        assert rc != 0 and b"too large" in lib.mrcnn_last_error(), (b, h, w, cin, cout)
