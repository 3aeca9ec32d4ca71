"""Host-side checks (no GPU) of the backward of the pyramid RoIAlign: the tests' reference against the fixture made from the
reference's own code, the C ABI as the header declares it, and the refusals that need no launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import roi_align_backward_cases as rc
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maskrcnn_hip.h")
NAME = "mrcnn_roi_align_pyramid_backward_f32"


def test_expected_reproduces_the_reference_fixture_bit_for_bit(oracle):
    """rc.expected (oracle.crop_backward per level, boxes in index order) with the fixture's stored levels against what the
    reference's crop_backward gave for model.roi_align's level split: this ties the GPU tests' reference to the reference."""
    z = load_golden("roi_align_backward")
    rois, levels = z["rois"], z["levels"]
    sizes = [tuple(int(v) for v in s) for s in z["map_sizes"]]
    assert sorted(set(levels.tolist())) == [2, 3, 4, 5] and len(rois) >= 30
    area = float(z["image_shape"][0] * z["image_shape"][1])
    k = rc.unrounded_level(rois, area)
    assert bool((np.abs(k[np.isfinite(k), None] - np.array([2.5, 3.5, 4.5])[None]).min(1) >= 1e-3).all())
    for pool in (7, 14, 1):
        grad = z[f"grad_out_p{pool}"]
        assert grad.shape == (len(rois), pool, pool, 4 if pool == 14 else 8)
        got = rc.expected(oracle, grad, rois, levels, 1, sizes, rois_per_image=len(rois))
        for l in range(4):
            want = z[f"g{l}_p{pool}"]
            assert want.shape == (1, *sizes[l], grad.shape[3]) and np.count_nonzero(want)
            assert np.array_equal(got[l].numpy().view(np.int32), want.view(np.int32)), (pool, l)


def test_expected_drops_skipped_slots_and_images_out_of_range(oracle):
    rng = np.random.default_rng(3)
    area, sizes = 128.0 * 128.0, [(32, 32), (16, 16), (8, 8), (4, 4)]
    rois = rc.boxes_on(rng, 6, 2, area)
    levels = rc.levels_of(rois, area)
    grad = rng.standard_normal((6, 2, 2, 4)).astype(np.float32)
    assert rc.roi_images(6, 2, rois_per_image=3, roi_counts=[2, 0]).tolist() == [0, 0, -1, -1, -1, -1]
    assert rc.roi_images(4, 2, roi_batch=[1, -1, 2, 0]).tolist() == [1, -1, -1, 0]
    full = rc.expected(oracle, grad[:2], rois[:2], levels[:2], 1, sizes, rois_per_image=2)
    nan = grad.copy()
    nan[2:] = np.nan
    counted = rc.expected(oracle, nan, rois, levels, 2, sizes, rois_per_image=3, roi_counts=[2, 0])
    for a, b in zip(full, counted):
        assert torch.equal(a[0], b[0]) and not bool(b[1].any())


def test_header_declares_the_function_and_the_binding_derives_its_signature():
    from maskrcnn_amd import _lib
    text = open(HEADER).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", text) and "ascending RoI index" in text
    assert NAME in _lib.declared_symbols() and "mrcnn_roi_align_pyramid_backward_workspace_bytes" in _lib.declared_symbols()
    res, args = _lib.header_prototypes()[NAME]
    p = ctypes.POINTER
    assert res is ctypes.c_int
    assert args == [_lib.c_vp, p(_lib.c_i32), p(_lib.c_i32), _lib.c_i32, _lib.c_i32, _lib.c_vp, _lib.c_vp, _lib.c_i32, _lib.c_i32,
                    _lib.c_vp, _lib.c_i32, _lib.c_f32, p(_lib.c_vp), _lib.c_vp, ctypes.c_size_t, _lib.c_vp]
    fn = getattr(_lib.lib, NAME)
    assert fn.argtypes == args and fn.restype is res
    assert _lib.lib.mrcnn_roi_align_pyramid_backward_workspace_bytes(0) == 0
    assert _lib.lib.mrcnn_roi_align_pyramid_backward_workspace_bytes(1000) == 32000


def test_abi_version_is_29_or_later_and_matches_the_library():
    from maskrcnn_amd import _lib
    assert _lib.header_abi_version() >= 29
    assert int(_lib.lib.mrcnn_abi_version()) == _lib.header_abi_version()


def test_the_kernel_file_is_built_without_contraction_and_shares_the_level_function():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_b", os.path.join(ROOT, "maskrcnn_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "-ffp-contract=off" in b.SOURCES["roi_align_backward.hip"]
    csrc = os.path.join(ROOT, "maskrcnn_amd", "csrc")
    math = open(os.path.join(csrc, "crop_math.hpp")).read()
    assert "int roi_level(" in math
    for f in ("crop.hip", "roi_align_backward.hip"):   # one definition: forward and backward cannot disagree about a box
        text = open(os.path.join(csrc, f)).read()
        assert "int roi_level(" not in text and "mrcnn_crop::roi_level" in text, f
    assert "atomic" not in re.sub(r"//.*", "", open(os.path.join(csrc, "roi_align_backward.hip")).read())


def test_bad_arguments_are_refused_before_any_launch():
    from maskrcnn_amd import ops
    assert "roi_align_pyramid_backward" not in ops.__all__ and not hasattr(torch.ops.maskrcnn, "roi_align_pyramid_backward")
    g, rois, sizes = torch.zeros(2, 7, 7, 8), torch.zeros(2, 4), [(8, 8), (4, 4), (2, 2), (1, 1)]
    with pytest.raises(RuntimeError, match=r"roi_align_pyramid_backward: map_sizes must be the \(H, W\) of the 4 levels P2..P5, each >= 1, got"):
        ops.roi_align_pyramid_backward(g, rois, 7, 1.0, 1, sizes[:3], rois_per_image=2)
    with pytest.raises(RuntimeError, match=r"roi_align_pyramid_backward: map_sizes must be"):
        ops.roi_align_pyramid_backward(g, rois, 7, 1.0, 1, [(8, 8), (4, 4), (2, 2), (0, 1)], rois_per_image=2)
    with pytest.raises(RuntimeError, match=r"roi_align_pyramid_backward: pool must be in 1 .. 1024, got 0"):
        ops.roi_align_pyramid_backward(g, rois, 0, 1.0, 1, sizes, rois_per_image=2)
    with pytest.raises(RuntimeError, match=r"roi_align_pyramid_backward: batch must be >= 1, got 0"):
        ops.roi_align_pyramid_backward(g, rois, 7, 1.0, 0, sizes, rois_per_image=2)
    with pytest.raises(RuntimeError, match=r"roi_align_pyramid_backward: grad_out must be float32 \[R,7,7,C\], got None"):
        ops.roi_align_pyramid_backward(None, rois, 7, 1.0, 1, sizes, rois_per_image=2)
    # CPU tensors: the refusal every op without a staged CPU form gives
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.roi_align_pyramid_backward(g, rois, 7, 1.0, 1, sizes, rois_per_image=2)
    maps = [torch.zeros(1, h, w, 8, requires_grad=True) for h, w in sizes]
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.roi_align_pyramid(maps, rois, 7, 1.0, rois_per_image=2)
