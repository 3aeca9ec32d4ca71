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
    # the bindings come from header_prototypes(): declared_symbols() is an independent regex, so equal name sets mean the
    # parser dropped no prototype, and every one of them carries its ctypes signature on the loaded library
    protos = _lib.header_prototypes()
    assert set(protos) == set(names), "the prototype parser and the header's declared names disagree"
    for n, (res, args) in protos.items():
        fn = getattr(_lib.lib, n)
        assert fn.restype == res and list(fn.argtypes) == args, f"{n} is not bound with the header's signature"
    assert _lib.lib.mrcnn_abi_version() == _lib.header_abi_version() >= 2
    assert _lib.lib.mrcnn_arch() == b"gfx950"


def test_header_parser_yields_the_hand_written_signatures():
    """The ctypes signatures are parsed from the header (a wrong one would pass wrong-width arguments to a kernel launch). These
    are written out by hand, one entry point or more for every category the parser distinguishes: a const char* / size_t /
    int64_t return, a (void) argument list, int64_t / float / size_t scalars, mrcnn_stream_t, plain pointers, host arrays of
    pointers (const float* const fm[4]) and host arrays of int32_t, float and double."""
    from maskrcnn_amd import _lib
    c_int, c_i32, c_i64, c_f32, c_vp, c_size = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p,
                                                ctypes.c_size_t)
    P = ctypes.POINTER
    want = {
        "mrcnn_last_error": (ctypes.c_char_p, []),
        "mrcnn_nms_max_boxes": (c_i64, []),
        "mrcnn_nms_workspace_bytes": (c_size, [c_i32, c_i64]),
        "mrcnn_nms_plan": (c_int, [c_i64, c_i32, P(c_i32)]),
        "mrcnn_nms_batched_f32": (c_int, [c_vp, c_i32, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp,
                                          c_f32, c_vp, c_vp, c_vp, c_size, c_vp]),
        "mrcnn_roi_align_pyramid_counted_f32": (c_int, [P(c_vp), P(c_i32), P(c_i32),
                                                        c_i32, c_i32, c_vp, c_vp, c_i32, c_i32, c_vp, c_i32, c_f32, c_vp,
                                                        c_i32, c_vp, c_vp]),
        "mrcnn_proposal_decode_f32": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32,
                                              P(c_f32), c_f32, c_f32, c_vp, c_vp]),
        "mrcnn_mold_images_u8": (c_int, [c_vp, c_i32, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32,
                                         P(ctypes.c_double), c_vp, c_vp, c_size, c_vp]),
        "mrcnn_bottleneck_forward_f32": (c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, P(c_vp), c_i32,
                                                 c_i32, c_vp, c_size, c_vp, c_vp]),
    }
    protos = _lib.header_prototypes()
    for name, (res, args) in want.items():
        hres, hargs = protos[name]
        assert res == hres, f"{name}: return type {res} vs header {hres}"
        assert len(args) == len(hargs), f"{name}: {len(args)} arguments vs {len(hargs)} in the header"
        for i, (a, h) in enumerate(zip(args, hargs)):
            assert a == h, f"{name}: argument {i} is {a} by hand, {h} from the header"


def test_unknown_type_in_the_header_is_an_import_error(tmp_path, monkeypatch):
    """A prototype whose type the parser has no ctypes type for must stop the import and name the prototype (it was a bare
    KeyError): binding it with a guessed width is how a kernel launch gets wrong arguments."""
    from maskrcnn_amd import _lib
    fake = tmp_path / "maskrcnn_hip.h"
    fake.write_text(open(_lib.HEADER).read() + "\nint mrcnn_made_up_entry(const float* x, uint8_t flag, mrcnn_stream_t stream);\n")
    monkeypatch.setattr(_lib, "HEADER", str(fake))
    with pytest.raises(ImportError, match=r"uint8_t.*mrcnn_made_up_entry\(const float\* x, uint8_t flag"):
        _lib._load()
    with pytest.raises(ImportError, match="mrcnn_made_up_entry"):
        _lib.header_prototypes(str(fake))


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


def _f16_checks(cfg, b):
    """Every fp16 size check the "f16" step consults at batch b (modules.py: ConvWeight.takes_pipelined, FusedBottleneck, FusedMask),
    by layer: the FPN laterals (1x1 C2..C5 -> 256) and smoothing convs (3x3 256 -> 256), the RPN's shared 3x3 256 -> 512 at every
    pyramid level, the one-launch C2 blocks, the classifier's 7x7 and 1x1 GEMMs, the mask head's 3x3 convs and its fused tail."""
    from maskrcnn_amd import ops
    p = min(cfg.proposal_count, cfg.pre_nms_limit)
    d = min(cfg.detection_max_instances, p)
    same3 = (1, 1, 1, 1)
    out = {}
    for lvl, (h, w) in enumerate(cfg.backbone_shapes):
        if lvl < 4:
            out[f"lateral P{lvl + 2}"] = ops.conv_f16_pipelined_supported(b, h, w, 256 << lvl, 256, 1, 1)
            out[f"smooth P{lvl + 2}"] = ops.conv_f16_pipelined_supported(b, h, w, 256, 256, 3, 3, same3)
        out[f"rpn P{lvl + 2}"] = ops.conv_f16_pipelined_supported(b, h, w, 256, 512, 3, 3, same3)
    h2, w2 = cfg.backbone_shapes[0]
    out["c2 block"] = ops.bottleneck_c2_f16_supported(b, h2, w2, 256, 64, False)
    out["c2 first block"] = ops.bottleneck_c2_f16_supported(b, h2, w2, 64, 64, True)
    # the classifier runs its 7x7 'valid' conv as a 1x1 conv on the flattened crops (modules.FusedClassifier)
    out["fc1"] = ops.conv_f16_pipelined_supported(b * p, 1, 1, cfg.pool_size * cfg.pool_size * 256, 1024, 1, 1)
    out["fc2"] = ops.conv_f16_pipelined_supported(b * p, 1, 1, 1024, 1024, 1, 1)
    mp = cfg.mask_pool_size
    out["mask conv"] = ops.conv_f16_pipelined_supported(b * d, mp, mp, 256, 256, 3, 3, same3)
    out["mask tail"] = ops.mask_tail_f16_supported(b * d, mp, mp, 256, 256, cfg.num_classes)
    return out


def test_max_batch_per_launch_f16_keeps_every_fp16_check_at_its_batch_1_answer():
    """max_batch_per_launch(cfg, "f16"): up to that batch the fp16 size checks of the "f16" step's batch-scaled layers (_f16_checks:
    the FPN, the RPN at every level, the C2 blocks, the classifier, the mask head and its tail) answer as they do for one image,
    so none of those layers changes kernel with the batch (image i of a batch == image i alone). The fp16 family keeps each
    tensor below 2^31 bytes and the pipelined conv counts its fp32 result even where it only writes fp16 or the RPN head sums:
    the RPN's 512-channel shared conv on P2 allows 15 images at 1024^2 and at 832 x 1344, not the fp32 step's 31 and 30. Beyond
    the bound some check changes its answer, or the fp32 bound (which the mode also obeys) is passed."""
    from maskrcnn_amd.config import InferenceConfig
    from maskrcnn_amd.pipeline import max_batch_per_launch
    for h, w, p, d in ((1024, 1024, 500, 50), (832, 1344, 1000, 50), (256, 256, 1000, 50), (128, 128, 4096, 4096),
                       (64, 64, 1000, 100), (64, 64, 1, 1)):
        cfg = InferenceConfig(image_height=h, image_width=w, pre_nms_limit=p, proposal_count=p, detection_max_instances=d)
        m = max_batch_per_launch(cfg, "f16")
        assert 1 <= m <= max_batch_per_launch(cfg), (h, w, p, d, m)
        one, at_m = _f16_checks(cfg, 1), _f16_checks(cfg, m)
        assert at_m == one, (h, w, p, d, m, {k: (one[k], at_m[k]) for k in one if one[k] != at_m[k]})
        assert _f16_checks(cfg, m + 1) != one or m == max_batch_per_launch(cfg), (h, w, p, d, m)
    big = InferenceConfig(image_height=1024, image_width=1024)
    r101 = InferenceConfig(image_height=832, image_width=1344, pre_nms_limit=1000, proposal_count=1000)
    assert (max_batch_per_launch(big, "f16"), max_batch_per_launch(r101, "f16")) == (15, 15)
    assert (max_batch_per_launch(big), max_batch_per_launch(r101)) == (31, 30)
    for cfg in (big, r101):   # the binding check: P2's RPN conv (its heads form) goes off the pipelined kernel at 16 images
        assert _f16_checks(cfg, 1)["rpn P2"] and not _f16_checks(cfg, 16)["rpn P2"]
    # the other precisions run no fp16-family kernel: the fp32 bound
    for precision in ("f32", "f16x3", "f32+f16x3"):
        assert max_batch_per_launch(big, precision) == 31


def test_entry_points_refuse_the_first_shape_past_their_limit():
    """Argument validation runs before any HIP call (dummy pointers, never touched): for each kernel family with 32-bit buffer
    byte offsets, the first shape past its size check is refused as "too large", and the shape just below it is inside the
    check's arithmetic (tests/test_gpu_large_tensors.py runs several of them on the GPU). OOB = 0xFFFFFFF0."""
    from maskrcnn_amd import _lib
    lib = _lib.lib
    dp = ctypes.c_void_p(16)
    dq = ctypes.c_void_p(4096)   # a second pointer where the entry point refuses aliasing
    big = ctypes.c_size_t(1 << 40)

    def refused(rc, what):
        assert rc != 0 and b"too large" in lib.mrcnn_last_error(), (what, lib.mrcnn_last_error())

    # F(2x2): 4 B H W max(Cin, Cout) <= OOB. B4 x 512 x 510, 1024 -> 1000 is accepted: 4 * 4 * 512 * 510 * 1024 <= OOB
    assert 4 * 4 * 512 * 510 * 1024 <= OOB < 4 * 4 * 512 * 512 * 1024
    refused(lib.mrcnn_conv3x3_winograd_f32(dp, 1, 4, 512, 512, 1024, dp, 1000, None, None, 0, dp, None, None, 0, None), "wino k-blocked")
    refused(lib.mrcnn_conv3x3_winograd_f32(dp, 0, 4, 512, 512, 1024, dp, 1000, None, None, 0, dp, dq, dp, big, None), "wino nhwc")
    refused(lib.mrcnn_conv3x3_winograd_f32(dp, 1, 4, 512, 512, 8, dp, 1024, None, None, 0, dp, None, None, 0, None), "wino Cout")
    refused(lib.mrcnn_conv3x3_winograd_nhwc_f32(dp, 4, 512, 512, 1024, dp, 1000, None, None, 0, dp, dq, big, None), "wino nhwc form")
    # F(2x2) heads (the RPN's shared conv + heads): 4 B H W Cin <= OOB; B16 x 512 x 510 x 256 accepted
    assert 4 * 16 * 512 * 510 * 256 <= OOB < 4 * 16 * 512 * 512 * 256
    refused(lib.mrcnn_conv3x3_winograd_heads_f32(dp, 16, 512, 512, 256, dp, 512, None, None, 1, dp, 2, dq, None), "wino heads")
    # the fused fp32 bottleneck: 4 px 256 <= OOB; B4 x 1024 x 1008 accepted
    assert 4 * 4 * 1024 * 1008 * 256 <= OOB < 4 * 4 * 1024 * 1024 * 256
    refused(lib.mrcnn_bottleneck_fused_f32(dp, 4, 1024, 1024, 256, dp, None, None, dp, None, None, dp, None, None, 64, dq, None),
            "bottleneck fused")
    # the stem: y fp32 [B][H/2][W/2][64] <= OOB; B16 x 2048 x 2040 accepted (3.98 GiB)
    assert 256 * 16 * 1024 * 1020 <= OOB < 256 * 16 * 1024 * 1024
    for f in (lib.mrcnn_stem_conv7x7_s2_nhwc_f32, lib.mrcnn_stem_conv7x7_s2_nchw_f32, lib.mrcnn_stem_conv7x7_s2_nchw_f16out):
        refused(f(dp, 16, 2048, 2048, dp, None, None, 1, dq, None), f.__name__)
    # the stem + pool: fp32 y below 2^31 bytes (B32 x 2048 x 2040 accepted), fp32 x <= OOB for the fp16 form (B85 x 2048^2)
    assert 16 * 32 * 2048 * 2040 < 1 << 31 <= 16 * 32 * 2048 * 2048
    refused(lib.mrcnn_stem_conv7x7_s2_pool_f32(dp, 32, 2048, 2048, dp, None, None, dq, None), "stem pool f32")
    assert 12 * 85 * 2048 * 2048 <= OOB < 12 * 86 * 2048 * 2048
    refused(lib.mrcnn_stem_conv7x7_s2_pool_f16(dp, 86, 2048, 2048, dp, None, None, dq, None), "stem pool f16")
    # the fp16 tile kernel (fill_common counts every tensor at 4 bytes per element): the 1x1 conv of
    # test_direct_conv_refuses_the_oob_sentinel_window, M Cout = 2^30 - 2
    for products in (1, 3):
        refused(lib.mrcnn_conv_bn_act_nhwc_f16mfma(dp, 1, 466, 1103, 32, dp, dp, 2089, 1, 1, 1, 0, 0, 0, 0, None, None, None, 1, 0,
                                                   products, dq, None), f"f16mfma products {products}")
    for xf, yf in ((1, 1), (1, 0), (0, 1)):
        refused(lib.mrcnn_conv_bn_act_nhwc_f16io(dp, xf, 1, 466, 1103, 32, dp, 2090, 1, 1, 1, 0, 0, 0, 0, None, None, None, 1, 0,
                                                 dq, yf, None), f"f16io {xf}{yf}")
    # the 2x2 deconvs: GEMM N = 4 Cout; 512 x 512 pixels x 4 x 1022 accepted, 4 x 1024 refused
    assert 16 * 512 * 512 * 1022 <= OOB < 16 * 512 * 512 * 1024
    refused(lib.mrcnn_deconv2x2_bias_act_nhwc_f16io(dp, 1, 512, 512, 32, dp, 1024, dp, 1, dq, None), "deconv f16io")
    refused(lib.mrcnn_deconv2x2_bias_act_nhwc_f16mfma(dp, 1, 512, 512, 32, dp, dp, 1024, dp, 1, 3, dq, None), "deconv f16mfma")
    # the fp16 family's own predicates, at the suggested top-of-range shapes and the first shape past them
    assert lib.mrcnn_conv_f16_pipelined_supported(8, 512, 508, 256, 256, 3, 3, 1, 1, 1, 1, 1)
    assert not lib.mrcnn_conv_f16_pipelined_supported(8, 512, 512, 256, 256, 3, 3, 1, 1, 1, 1, 1)
    assert lib.mrcnn_bottleneck_c2_f16_supported(16, 512, 508, 256, 64, 0)
    assert not lib.mrcnn_bottleneck_c2_f16_supported(16, 512, 512, 256, 64, 0)
    assert lib.mrcnn_mask_tail_f16_supported(16907, 14, 14, 256, 256, 81)
    assert not lib.mrcnn_mask_tail_f16_supported(16908, 14, 14, 256, 256, 81)


def test_conv_entry_points_with_a_shared_fill_keep_every_refusal():
    """The conv entry points whose parameter blocks are filled by one shared function (F(4x4) plain / heads / conv3, F(2x2)
    plain / NHWC / heads, the pipelined fp16 conv and its heads form, the stem and the two stem + pool forms): one row per check of
    each entry point — return code and exact message —, and where one bad tuple trips two checks, the one that came first
    still wins. Validation runs before any HIP call (dummy pointers, never touched); every row is a refusal, so nothing is
    launched on a machine that has a GPU."""
    from maskrcnn_amd import _lib
    lib = _lib.lib
    dp, dq, N = ctypes.c_void_p(16), ctypes.c_void_p(4096), None
    INVALID, UNSUPPORTED = -1, -2
    big = ctypes.c_size_t(1 << 40)

    def row(rc, code, text):
        assert (rc, lib.mrcnn_last_error()) == (code, text.encode()), (text, rc, lib.mrcnn_last_error())

    # ---- F(4x4) plain: (x, B, H, W, Cin, u, Cout, scale, shift, act, y, yk, stream)
    w4 = lib.mrcnn_conv3x3_winograd4_f32
    shape4 = "%s: B=%d H=%d W=%d (%% 4 == 0) Cin=%d (%% 8 == 0) Cout=%d (%% 64 == 0), 4*B*H*W*C <= 0xFFFFFFF0 bytes required"
    who = "conv3x3_winograd4"
    row(w4(N, 1, 8, 8, 8, dp, 64, N, N, 1, dq, N, N), INVALID, who + ": null pointer")
    row(w4(dp, 1, 8, 8, 8, N, 64, N, N, 1, dq, N, N), INVALID, who + ": null pointer")
    row(w4(dp, 1, 8, 8, 8, dp, 64, N, N, 1, N, N, N), INVALID, who + ": null pointer")
    for b, h, w, cin, cout in ((0, 8, 8, 8, 64), (1, 6, 8, 8, 64), (1, 8, 10, 8, 64), (1, 0, 8, 8, 64), (1, 8, 8, 12, 64),
                               (1, 8, 8, 0, 64), (1, 8, 8, 8, 96), (1, 8, 8, 8, 32),
                               (4, 512, 512, 1024, 64), (4, 512, 512, 8, 1024), (1, 8, 8, 8192, 4096)):   # the three byte limits
        row(w4(dp, b, h, w, cin, dp, cout, N, N, 1, dq, N, N), INVALID, shape4 % (who, b, h, w, cin, cout))
    row(w4(dp, 1, 8, 8, 8, dp, 64, N, N, 2, dq, N, N), INVALID, who + ": activation must be 0 or 1")
    row(w4(dp, 1, 8, 8, 8, dp, 64, N, N, -1, N, dq, N), INVALID, who + ": activation must be 0 or 1")
    row(w4(N, 1, 6, 8, 8, dp, 64, N, N, 2, dq, N, N), INVALID, who + ": null pointer")                    # first check wins
    row(w4(dp, 1, 6, 8, 8, dp, 64, N, N, 2, dq, N, N), INVALID, shape4 % (who, 1, 6, 8, 8, 64))
    # ---- F(4x4) heads: (x, B, H, W, Cin, u, Cout, scale, shift, act, w_head, head_part, stream)
    w4h = lib.mrcnn_conv3x3_winograd4_heads_f32
    who = "conv3x3_winograd4_heads"
    row(w4h(dp, 1, 8, 8, 8, dp, 64, N, N, 1, N, dq, N), INVALID, who + ": null pointer")
    row(w4h(dp, 1, 8, 8, 8, dp, 64, N, N, 1, dp, N, N), INVALID, who + ": null pointer")
    for b, h, w, cin, cout in ((1, 6, 8, 8, 64), (1, 8, 8, 12, 64), (1, 8, 8, 8, 96), (4, 512, 512, 1024, 64)):
        row(w4h(dp, b, h, w, cin, dp, cout, N, N, 1, dp, dq, N), INVALID, shape4 % (who, b, h, w, cin, cout))
    row(w4h(dp, 1, 8, 8, 8, dp, 64, N, N, 2, dp, dq, N), INVALID, who + ": activation must be 0 or 1")
    # the head sums: 512 rows x 32 fp32 per M tile, a tile per 4 x 4 image here: 65 536 tiles are 2^32 bytes
    assert lib.mrcnn_conv3x3_winograd4_supported(65536, 4, 4, 8, 64) and 4 * 65536 * 512 * 32 > OOB >= 4 * 65535 * 512 * 32
    row(w4h(dp, 65536, 4, 4, 8, dp, 64, N, N, 1, dp, dq, N), INVALID, who + ": tensor too large (32-bit buffer byte offsets)")
    row(w4h(dp, 65536, 4, 4, 8, dp, 64, N, N, 2, dp, dq, N), INVALID, who + ": activation must be 0 or 1")   # first check wins
    row(w4h(dp, 65536, 4, 4, 12, dp, 64, N, N, 2, dp, dq, N), INVALID, shape4 % (who, 65536, 4, 4, 12, 64))
    # ---- F(4x4) conv2 + conv3: (x, B, H, W, Cin, u, scale, shift, w3, c3, scale3, shift3, residual, y, stream)
    w43 = lib.mrcnn_conv3x3_winograd4_conv3_f32
    who = "conv3x3_winograd4_conv3"
    shape43 = who + ": B=%d H=%d W=%d (%% 4 == 0) Cin=%d (%% 8 == 0), 4*B*H*W*C <= 0xFFFFFFF0 bytes required"
    row(w43(dp, 1, 8, 8, 64, dp, N, N, N, 256, N, N, dp, dq, N), INVALID, who + ": null pointer")
    row(w43(dp, 1, 8, 8, 64, dp, N, N, dp, 256, N, N, N, dq, N), INVALID, who + ": null pointer")
    row(w43(dp, 1, 8, 8, 64, dp, N, N, dp, 256, N, N, dp, N, N), INVALID, who + ": null pointer")
    for b, h, w, cin in ((1, 6, 8, 64), (1, 8, 8, 12), (0, 8, 8, 64), (16, 1024, 1024, 64)):
        row(w43(dp, b, h, w, cin, dp, N, N, dp, 256, N, N, dp, dq, N), INVALID, shape43 % (b, h, w, cin))
    for c3 in (0, 48, 288):
        row(w43(dp, 1, 8, 8, 64, dp, N, N, dp, c3, N, N, dp, dq, N), INVALID,
            who + ": c3=%d must be a multiple of 32, at most 256" % c3)
    row(w43(dp, 1, 8, 8, 64, dp, N, N, dp, 256, N, N, dq, dq, N), INVALID, who + ": in-place operation is not supported")
    assert lib.mrcnn_conv3x3_winograd4_supported(32, 512, 512, 64, 64) and 4 * 32 * 512 * 512 * 256 > OOB
    row(w43(dp, 32, 512, 512, 64, dp, N, N, dp, 256, N, N, dp, dq, N), INVALID, who + ": tensor too large (32-bit buffer byte offsets)")
    row(w43(dp, 1, 6, 8, 64, dp, N, N, dp, 48, N, N, dq, dq, N), INVALID, shape43 % (1, 6, 8, 64))              # first check wins
    row(w43(dp, 1, 8, 8, 64, dp, N, N, dp, 48, N, N, dq, dq, N), INVALID, who + ": c3=48 must be a multiple of 32, at most 256")
    row(w43(dp, 32, 512, 512, 64, dp, N, N, dp, 256, N, N, dq, dq, N), INVALID, who + ": in-place operation is not supported")

    # ---- F(2x2) plain: (x, x_layout, B, H, W, Cin, u, Cout, scale, shift, act, y, yk, workspace, workspace_bytes, stream)
    w2 = lib.mrcnn_conv3x3_winograd_f32
    who = "conv3x3_winograd"
    need_ws = who + ": an NHWC input needs a workspace of mrcnn_conv3x3_winograd_workspace_bytes()"
    row(w2(N, 1, 1, 8, 8, 8, dp, 64, N, N, 1, dq, N, N, 0, N), INVALID, who + ": null pointer")
    row(w2(dp, 1, 1, 8, 8, 8, N, 64, N, N, 1, dq, N, N, 0, N), INVALID, who + ": null pointer")
    row(w2(dp, 1, 1, 8, 8, 8, dp, 64, N, N, 1, N, N, N, 0, N), INVALID, who + ": null pointer")
    row(w2(dp, 2, 1, 8, 8, 8, dp, 64, N, N, 1, dq, N, N, 0, N), INVALID, who + ": bad x_layout")
    row(w2(dp, 0, 1, 8, 8, 8, dp, 64, N, N, 1, dq, N, N, big, N), INVALID, need_ws)
    row(w2(dp, 0, 1, 8, 8, 8, dp, 64, N, N, 1, dq, N, dq, 4 * 8 * 8 * 8 - 1, N), INVALID, need_ws)
    for b, h, w in ((0, 8, 8), (1, 7, 8), (1, 8, 9), (1, 0, 8)):
        row(w2(dp, 1, b, h, w, 8, dp, 64, N, N, 1, dq, N, N, 0, N), INVALID,
            who + ": B=%d H=%d W=%d (even sizes required)" % (b, h, w))
    for cin, cout in ((12, 64), (0, 64), (8, 0)):
        row(w2(dp, 1, 1, 8, 8, cin, dp, cout, N, N, 1, dq, N, N, 0, N), INVALID,
            who + ": Cin=%d (%% 8 == 0 required) Cout=%d" % (cin, cout))
    row(w2(dp, 1, 1, 8, 8, 8, dp, 12, N, N, 1, N, dq, N, 0, N), INVALID, who + ": a k-blocked output needs Cout % 8 == 0")
    row(w2(dp, 1, 1, 8, 8, 8, dp, 12, N, N, 2, dq, N, N, 0, N), INVALID, who + ": activation must be 0 or 1")
    for cin, cout in ((1024, 1000), (8, 1024)):   # 4 B H W Cin, 4 B H W Cout; 64 Cin Cout below
        row(w2(dp, 1, 4, 512, 512, cin, dp, cout, N, N, 0, dq, N, N, 0, N), INVALID, who + ": tensor too large (32-bit buffer byte offsets)")
    row(w2(dp, 1, 1, 8, 8, 8192, dp, 8192, N, N, 0, dq, N, N, 0, N), INVALID, who + ": tensor too large (32-bit buffer byte offsets)")
    row(w2(N, 2, 1, 7, 8, 8, dp, 64, N, N, 1, dq, N, N, 0, N), INVALID, who + ": null pointer")                # first check wins
    row(w2(dp, 2, 1, 7, 8, 8, dp, 64, N, N, 1, dq, N, N, 0, N), INVALID, who + ": bad x_layout")
    row(w2(dp, 0, 1, 7, 8, 8, dp, 64, N, N, 1, dq, N, N, 0, N), INVALID, need_ws)
    row(w2(dp, 1, 1, 7, 8, 12, dp, 64, N, N, 1, dq, N, N, 0, N), INVALID, who + ": B=1 H=7 W=8 (even sizes required)")
    row(w2(dp, 1, 1, 8, 8, 12, dp, 12, N, N, 1, dq, dq, N, 0, N), INVALID, who + ": Cin=12 (% 8 == 0 required) Cout=12")
    row(w2(dp, 1, 1, 8, 8, 8, dp, 12, N, N, 2, dq, dq, N, 0, N), INVALID, who + ": a k-blocked output needs Cout % 8 == 0")
    row(w2(dp, 1, 4, 512, 512, 1024, dp, 1000, N, N, 2, dq, N, N, 0, N), INVALID, who + ": activation must be 0 or 1")
    # ---- F(2x2), the NHWC form: (x, B, H, W, Cin, u, Cout, scale, shift, act, y, workspace, workspace_bytes, stream): the same checks
    w2n = lib.mrcnn_conv3x3_winograd_nhwc_f32
    row(w2n(dp, 1, 8, 8, 8, dp, 64, N, N, 1, N, dq, big, N), INVALID, who + ": null pointer")
    row(w2n(dp, 1, 8, 8, 8, dp, 64, N, N, 1, dq, N, big, N), INVALID, need_ws)
    row(w2n(dp, 1, 8, 8, 8, dp, 64, N, N, 1, dq, dq, 4 * 8 * 8 * 8 - 1, N), INVALID, need_ws)
    row(w2n(dp, 1, 7, 8, 8, dp, 64, N, N, 1, dq, dq, big, N), INVALID, who + ": B=1 H=7 W=8 (even sizes required)")
    row(w2n(dp, 1, 8, 8, 12, dp, 64, N, N, 1, dq, dq, big, N), INVALID, who + ": Cin=12 (% 8 == 0 required) Cout=64")
    row(w2n(dp, 1, 8, 8, 8, dp, 64, N, N, 2, dq, dq, big, N), INVALID, who + ": activation must be 0 or 1")
    row(w2n(dp, 4, 512, 512, 1024, dp, 1000, N, N, 0, dq, dq, big, N), INVALID, who + ": tensor too large (32-bit buffer byte offsets)")
    row(w2n(dp, 1, 7, 8, 8, dp, 64, N, N, 2, dq, N, big, N), INVALID, need_ws)                                   # first check wins
    # ---- F(2x2) heads: (x, B, H, W, Cin, u, Cout, scale, shift, act, w_head, tile_mode, head_part, stream)
    w2h = lib.mrcnn_conv3x3_winograd_heads_f32
    who = "conv3x3_winograd_heads"
    bad_mode = who + ": tile_mode must be 2 (8 x 8 position blocks), on maps of at least 8 x 8 tile positions"
    row(w2h(dp, 1, 16, 16, 8, dp, 64, N, N, 1, N, 2, dq, N), INVALID, who + ": null pointer")
    row(w2h(dp, 1, 16, 16, 8, dp, 64, N, N, 1, dp, 2, N, N), INVALID, who + ": null pointer")
    row(w2h(dp, 1, 15, 16, 8, dp, 64, N, N, 1, dp, 2, dq, N), INVALID, who + ": B=1 H=15 W=16 (even sizes required)")
    for cin, cout in ((12, 64), (8, 96), (8, 32)):
        row(w2h(dp, 1, 16, 16, cin, dp, cout, N, N, 1, dp, 2, dq, N), INVALID,
            who + ": Cin=%d (%% 8 == 0) Cout=%d (%% 64 == 0) required" % (cin, cout))
    row(w2h(dp, 1, 16, 16, 8, dp, 64, N, N, 2, dp, 2, dq, N), INVALID, who + ": activation must be 0 or 1")
    row(w2h(dp, 1, 16, 16, 8, dp, 64, N, N, 1, dp, 3, dq, N), INVALID, bad_mode)
    row(w2h(dp, 1, 16, 14, 8, dp, 64, N, N, 1, dp, 2, dq, N), INVALID, bad_mode)    # 8 x 7 tile positions
    row(w2h(dp, 16, 512, 512, 256, dp, 512, N, N, 1, dp, 2, dq, N), INVALID, who + ": tensor too large (32-bit buffer byte offsets)")
    row(w2h(dp, 1, 15, 16, 12, dp, 64, N, N, 1, dp, 2, dq, N), INVALID, who + ": B=1 H=15 W=16 (even sizes required)")   # first wins
    row(w2h(dp, 1, 16, 16, 12, dp, 64, N, N, 2, dp, 2, dq, N), INVALID, who + ": Cin=12 (% 8 == 0) Cout=64 (% 64 == 0) required")
    row(w2h(dp, 1, 16, 16, 8, dp, 64, N, N, 2, dp, 3, dq, N), INVALID, who + ": activation must be 0 or 1")
    row(w2h(dp, 16, 512, 512, 256, dp, 512, N, N, 1, dp, 3, dq, N), INVALID, bad_mode)

    # ---- the pipelined fp16 conv: (x, B, H, W, Cin, w, Cout, kh, kw, stride, pads t l b r, scale, shift, residual, res_div, act,
    #      y16, y32, tile_rows, tile_cols, stream). A call that names both tile sizes needs no device query.
    p8 = lib.mrcnn_conv_f16_pipelined
    who = "conv_f16_pipelined"
    unsup = (who + ": needs Cin %% 64 == 0, Cout %% 64 == 0, <= 25 taps, 0 <= pads < kernel, 32-bit byte offsets "
             "(got %dx%dx%dx%d -> %d, %dx%d stride %d)")
    row(p8(N, 1, 8, 8, 64, dp, 64, 3, 3, 1, 1, 1, 1, 1, N, N, N, 1, 1, dq, N, 128, 64, N), INVALID, who + ": null pointer")
    row(p8(dp, 1, 8, 8, 64, N, 64, 3, 3, 1, 1, 1, 1, 1, N, N, N, 1, 1, dq, N, 128, 64, N), INVALID, who + ": null pointer")
    row(p8(dp, 1, 8, 8, 64, dp, 64, 3, 3, 1, 1, 1, 1, 1, N, N, N, 1, 1, N, N, 128, 64, N), INVALID, who + ": null pointer")
    row(p8(dp, 1, 8, 8, 64, dp, 64, 3, 3, 1, 1, 1, 1, 1, N, N, N, 1, 2, dq, N, 128, 64, N), INVALID,
        who + ": activation must be 0 (none) or 1 (ReLU)")
    for b, h, w, cin, cout, k, s, pad in ((1, 8, 8, 32, 64, 3, 1, 1), (1, 8, 8, 64, 96, 3, 1, 1), (1, 8, 8, 64, 64, 6, 1, 1),
                                          (1, 8, 8, 64, 64, 3, 9, 1), (1, 8, 8, 64, 64, 3, 1, 3), (0, 8, 8, 64, 64, 3, 1, 1),
                                          (8, 512, 512, 256, 256, 3, 1, 1)):
        row(p8(dp, b, h, w, cin, dp, cout, k, k, s, pad, pad, pad, pad, N, N, N, 1, 1, dq, N, 128, 64, N), UNSUPPORTED,
            unsup % (b, h, w, cin, cout, k, k, s))
    row(p8(dp, 1, 8, 8, 64, dp, 64, 3, 3, 1, 1, 1, 1, 1, N, N, dp, 3, 1, dq, N, 128, 64, N), INVALID,
        who + ": res_div must be 1, or 2 with even output sizes (got 3, 8x8)")
    row(p8(dp, 1, 7, 8, 64, dp, 64, 1, 1, 1, 0, 0, 0, 0, N, N, dp, 2, 1, dq, N, 128, 64, N), INVALID,
        who + ": res_div must be 1, or 2 with even output sizes (got 2, 7x8)")
    for rows, cols, cout in ((100, 256, 256), (128, 256, 128), (128, 100, 256), (128, 128, 192),
                             (16, 256, 256), (31, 256, 256), (-5, 256, 256), (-31, 128, 128), (128, 32, 64), (128, -5, 64)):   # x / 32, x / 64 == 0
        row(p8(dp, 1, 8, 8, 64, dp, cout, 3, 3, 1, 1, 1, 1, 1, N, N, N, 1, 1, dq, N, rows, cols, N), INVALID,
            who + ": tile %d x %d does not fit Cout %d" % (rows, cols, cout))
    for rows, cols, cout in ((160, 128, 128), (192, 64, 64), (96, 256, 256), (128, 192, 192), (128, 512, 512)):
        row(p8(dp, 1, 8, 8, 64, dp, cout, 3, 3, 1, 1, 1, 1, 1, N, N, N, 1, 1, dq, N, rows, cols, N), INVALID,
            who + ": tile must be 0 (auto), rows 128 / 160 / 192 / 256 x 256 columns, or rows 128 / 256 x 128 / 64 columns "
            "(got %d x %d)" % (rows, cols))
    row(p8(N, 1, 8, 8, 32, dp, 64, 3, 3, 1, 1, 1, 1, 1, N, N, N, 1, 2, dq, N, 100, 256, N), INVALID, who + ": null pointer")   # first wins
    row(p8(dp, 1, 8, 8, 32, dp, 64, 3, 3, 1, 1, 1, 1, 1, N, N, dp, 3, 2, dq, N, 100, 256, N), INVALID,
        who + ": activation must be 0 (none) or 1 (ReLU)")
    row(p8(dp, 1, 8, 8, 32, dp, 64, 3, 3, 1, 1, 1, 1, 1, N, N, dp, 3, 1, dq, N, 100, 256, N), UNSUPPORTED, unsup % (1, 8, 8, 32, 64, 3, 3, 1))
    row(p8(dp, 1, 8, 8, 64, dp, 64, 3, 3, 1, 1, 1, 1, 1, N, N, dp, 3, 1, dq, N, 100, 256, N), INVALID,
        who + ": res_div must be 1, or 2 with even output sizes (got 3, 8x8)")
    # ---- its heads form: (x, B, H, W, Cin, w, Cout, kh, kw, pads t l b r, scale, shift, act, w_head, head_part, tile_rows, stream)
    p8h = lib.mrcnn_conv_f16_pipelined_heads
    who = "conv_f16_pipelined_heads"
    unsup = (who + ": needs Cin %% 64 == 0, Cout %% 256 == 0, <= 25 taps, 0 <= pads < kernel, 32-bit byte offsets "
             "(got %dx%dx%dx%d -> %d, %dx%d)")
    row(p8h(dp, 1, 8, 8, 64, dp, 256, 3, 3, 1, 1, 1, 1, N, N, 1, N, dq, 128, N), INVALID, who + ": null pointer")
    row(p8h(dp, 1, 8, 8, 64, dp, 256, 3, 3, 1, 1, 1, 1, N, N, 1, dp, N, 128, N), INVALID, who + ": null pointer")
    row(p8h(dp, 1, 8, 8, 64, dp, 256, 3, 3, 1, 1, 1, 1, N, N, 2, dp, dq, 128, N), INVALID, who + ": activation must be 0 (none) or 1 (ReLU)")
    for cin, cout, k in ((64, 128, 3), (32, 256, 3), (64, 256, 6)):
        row(p8h(dp, 1, 8, 8, cin, dp, cout, k, k, 1, 1, 1, 1, N, N, 1, dp, dq, 128, N), UNSUPPORTED, unsup % (1, 8, 8, cin, cout, k, k))
    for rows in (96, 100, 224, 288, 16, 31, -5):
        row(p8h(dp, 1, 8, 8, 64, dp, 256, 3, 3, 1, 1, 1, 1, N, N, 1, dp, dq, rows, N), INVALID,
            who + ": tile_rows must be 0 (auto), 128, 160, 192 or 256")
    row(p8h(dp, 1, 8, 8, 64, dp, 128, 3, 3, 1, 1, 1, 1, N, N, 2, dp, dq, 96, N), INVALID, who + ": activation must be 0 (none) or 1 (ReLU)")
    row(p8h(dp, 1, 8, 8, 64, dp, 128, 3, 3, 1, 1, 1, 1, N, N, 1, dp, dq, 96, N), UNSUPPORTED, unsup % (1, 8, 8, 64, 128, 3, 3))

    # ---- the stem: (x, B, H, W, w, scale, shift, act, y, stream), three forms with the same checks
    for f in (lib.mrcnn_stem_conv7x7_s2_nhwc_f32, lib.mrcnn_stem_conv7x7_s2_nchw_f32, lib.mrcnn_stem_conv7x7_s2_nchw_f16out):
        row(f(N, 1, 8, 8, dp, N, N, 1, dq, N), INVALID, "stem: null pointer")
        row(f(dp, 1, 8, 8, N, N, N, 1, dq, N), INVALID, "stem: null pointer")
        row(f(dp, 1, 8, 8, dp, N, N, 1, N, N), INVALID, "stem: null pointer")
        for b, h, w in ((0, 8, 8), (1, 7, 8), (1, 8, 9), (1, 0, 8)):
            row(f(dp, b, h, w, dp, N, N, 1, dq, N), INVALID, "stem: B=%d H=%d W=%d (even sizes required)" % (b, h, w))
        row(f(dp, 1, 8, 8, dp, N, N, 2, dq, N), INVALID, "stem: activation must be 0 or 1")
        row(f(dp, 16, 2048, 2048, dp, N, N, 1, dq, N), INVALID, "stem: tensor too large (32-bit buffer byte offsets)")
        row(f(N, 1, 7, 8, dp, N, N, 2, dq, N), INVALID, "stem: null pointer")                                     # first check wins
        row(f(dp, 1, 7, 8, dp, N, N, 2, dq, N), INVALID, "stem: B=1 H=7 W=8 (even sizes required)")
        row(f(dp, 16, 2048, 2048, dp, N, N, 2, dq, N), INVALID, "stem: activation must be 0 or 1")
    # ---- the stem + pool: (x, B, H, W, w, scale, shift, y, stream); each form with its own size limit
    for f, who, b_over, note in ((lib.mrcnn_stem_conv7x7_s2_pool_f16, "stem_pool", 86, ""),
                                 (lib.mrcnn_stem_conv7x7_s2_pool_f32, "stem_pool_f32", 32, ": B*H*W < 2^27 pixels")):
        row(f(N, 1, 8, 8, dp, N, N, dq, N), INVALID, who + ": null pointer")
        row(f(dp, 1, 8, 8, N, N, N, dq, N), INVALID, who + ": null pointer")
        row(f(dp, 1, 8, 8, dp, N, N, N, N), INVALID, who + ": null pointer")
        for b, h, w in ((0, 8, 8), (1, 6, 8), (1, 8, 10), (1, 0, 8)):
            row(f(dp, b, h, w, dp, N, N, dq, N), INVALID, who + ": B=%d H=%d W=%d (multiples of 4 required)" % (b, h, w))
        too_large = who + ": tensor too large (32-bit buffer byte offsets%s)" % note
        row(f(dp, b_over, 2048, 2048, dp, N, N, dq, N), INVALID, too_large)
        row(f(N, 1, 6, 8, dp, N, N, dq, N), INVALID, who + ": null pointer")                                      # first check wins
        row(f(dp, b_over, 2046, 2048, dp, N, N, dq, N), INVALID, who + ": B=%d H=2046 W=2048 (multiples of 4 required)" % b_over)


def test_refine_stage_entry_points_refuse_bad_arguments():
    """Argument validation of the selection / glue / RoIAlign entry points runs before any HIP call (dummy pointers, never
    touched): each refusal with its message."""
    from maskrcnn_amd import _lib
    lib = _lib.lib
    dp = ctypes.c_void_p(4096)
    i5 = lambda *v: (ctypes.c_int32 * 5)(*v)
    i4 = lambda *v: (ctypes.c_int32 * 4)(*v)

    def refused(rc, text):
        assert rc != 0 and text in lib.mrcnn_last_error(), (text, lib.mrcnn_last_error())

    # top-k: k <= 4096, k <= n, n < 2^32 - 1 (indices are stored complemented in 32 bits, 0 is the padding key), workspace
    need = lib.mrcnn_topk_workspace_bytes(2)
    assert need > 0 and lib.mrcnn_topk_workspace_bytes(0) == 0
    refused(lib.mrcnn_topk_desc_f32(dp, 2, 100000, 4097, dp, dp, dp, need, None), b"topk: k=4097 must be in [1, min(n, 4096)]")
    refused(lib.mrcnn_topk_desc_f32(dp, 2, 10, 11, dp, dp, dp, need, None), b"topk: k=11 must be in [1, min(n, 4096)]")
    refused(lib.mrcnn_topk_desc_f32(dp, 1, 2 ** 32 - 1, 1000, dp, dp, dp, need, None), b"topk: batch=1 n=4294967295")
    refused(lib.mrcnn_topk_desc_f32(dp, 2, 100000, 1000, dp, dp, dp, need - 1, None),
            b"topk: workspace too small (%d < %d)" % (need - 1, need))
    refused(lib.mrcnn_topk_desc_f32(dp, 2, 100000, 1000, dp, dp, dp, lib.mrcnn_topk_workspace_bytes(1), None),
            b"topk: workspace too small")
    # proposal_select: keep[:proposal_count] of k boxes
    refused(lib.mrcnn_proposal_select_f32(dp, dp, dp, 2, 1000, 1001, 1024.0, 1024.0, dp, dp, None),
            b"proposal_select: batch=2 k=1000 proposal_count=1001 (1 <= proposal_count <= k)")
    # rpn_scores_deltas: the head-sum forms need whole tiles and the bias they have not added yet
    heads = (ctypes.c_void_p * 5)(*[4096] * 5)
    bias = ctypes.c_void_p(8192)
    for lvl, h, w, mode, b in ((0, 7, 8, 1, bias), (1, 8, 7, 2, bias), (2, 7, 8, 2, bias), (3, 6, 8, 3, bias), (4, 8, 6, 3, bias),
                               (0, 8, 8, 1, None), (1, 8, 8, 2, None), (2, 8, 8, 3, None), (3, 8, 8, 4, None), (4, 8, 8, 5, bias)):
        hs, ws, modes = [8] * 5, [8] * 5, [0] * 5
        hs[lvl], ws[lvl], modes[lvl] = h, w, mode
        refused(lib.mrcnn_rpn_scores_deltas_v2_f32(heads, i5(*hs), i5(*ws), i5(*modes), b, 1, dp, dp, None),
                b"rpn_scores_deltas: level %d: mode must be 0 (NHWC heads), 1 or 2" % lvl)
    # the pyramid RoIAlign: roi_counts excludes roi_batch; four channels per lane; pool
    fm = (ctypes.c_void_p * 4)(*[4096] * 4)
    call = lambda depth, roi_batch, counts, pool: lib.mrcnn_roi_align_pyramid_counted_f32(
        fm, i4(32, 16, 8, 4), i4(32, 16, 8, 4), 2, depth, dp, roi_batch, 16, 8, counts, pool, 16384.0, dp, 0, None, None)
    refused(call(256, dp, dp, 7), b"roi_align_pyramid: roi_counts needs rois_per_image (no roi_batch)")
    refused(call(258, None, None, 7), b"roi_align_pyramid: depth=258 must be a multiple of 4")
    refused(call(2, None, None, 7), b"roi_align_pyramid: depth=2 must be a multiple of 4")
    refused(call(256, None, None, 0), b"roi_align_pyramid: pool=0")
    refused(call(256, None, None, 1025), b"roi_align_pyramid: pool=1025")


def test_detection_decode_argmax_sentinel_restated():
    """The arg-max loop of detection_decode restated on the host (`v > best` from -inf with the index sentinel 0x7fffffff): a
    row without an ordered maximum — all NaN, all -inf — leaves the sentinel in place, which the kernel used to multiply by 4
    as a bbox offset and write out as a class id; a NaN or +inf logit beside ordinary ones leaves a valid index but a NaN
    sum of exponentials. The rule the kernel now applies (index outside [0, C) or NaN sum: the empty-slot record) catches
    exactly the rows whose softmax is NaN in torch (tests/test_gpu_refine_edges.py runs the kernel)."""
    import numpy as np
    nan, inf = float("nan"), float("inf")
    rows = {"benign": [0.5, 2.0, -1.0], "some -inf": [-inf, 1.0, -inf], "one NaN": [0.5, nan, 1.0], "one +inf": [0.5, inf, 1.0],
            "all NaN": [nan] * 3, "all -inf": [-inf] * 3}
    for name, row in rows.items():
        best, besti = np.float32(-inf), 0x7FFFFFFF
        for c, v in enumerate(np.float32(row)):
            if v > best:
                best, besti = v, c
        with np.errstate(invalid="ignore"):
            total = np.float32(sum(np.exp(v - best) for v in np.float32(row)))
        assert (besti == 0x7FFFFFFF) == (name in ("all NaN", "all -inf")), name
        dropped = not 0 <= besti < len(row) or bool(np.isnan(total))
        softmax_is_nan = bool(torch.isnan(torch.softmax(torch.tensor(row), 0)).all())
        assert dropped == softmax_is_nan == (name not in ("benign", "some -inf")), name
        if softmax_is_nan:
            assert int(torch.max(torch.softmax(torch.tensor(row), 0), 0)[1]) == 0      # the reference: background
