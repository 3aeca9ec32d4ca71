"""Rendering detections (data.blend_image without the labels) without a GPU: tests/golden/blend.npz (made with the reference's own
blend_image / blend_mask / random_colors under Pillow: tests/golden/make_golden_blend.py) against the numpy host route of
image.blend_image, which the GPU tests use as the yardstick where Pillow cannot go; and the boundary of the new entry point:
header, exported symbol, public names, loud CPU refusal, predict.py --render."""
import ctypes
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def blend_cases():
    """The golden cases, read once and shared: dicts of name, n, h, w, seed, image [h,w,3], masks uint8 0 / 1 [n,h,w], boxes
    float64 [n,4], colors uint8 [n,3], want uint8 [h,w,3]. The arrays are read-only."""
    z = load_golden("blend")
    out = []
    for k, name in enumerate(z["names"].tolist()):
        n, h, w = (int(v) for v in z["shapes"][k])
        rows = slice(int(z["box_off"][k]), int(z["box_off"][k + 1]))
        px = slice(int(z["img_off"][k]), int(z["img_off"][k + 1]))
        bits = np.unpackbits(z["masks"][int(z["mask_off"][k]):int(z["mask_off"][k + 1])])[:n * h * w]
        c = dict(name=name, n=n, h=h, w=w, seed=int(z["seeds"][k]), image=z["images"][px].reshape(h, w, 3),
                 masks=bits.reshape(n, h, w), boxes=z["boxes"][rows], colors=z["colors"][rows],
                 want=z["outputs"][px].reshape(h, w, 3))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(c)
    return tuple(out)


def case(name):
    return next(c for c in blend_cases() if c["name"] == name)


def host(c, **kw):
    from maskrcnn_amd import image
    args = dict(image=np.array(c["image"]), boxes=None if c["boxes"] is None else np.array(c["boxes"]), masks=torch.from_numpy(c["masks"].copy()), colors=c["colors"], threshold=0,
                device="cpu")
    args.update(kw)
    return image.blend_image(**args).numpy()


def test_golden_fixture_covers_the_cases():
    cases = {c["name"]: c for c in blend_cases()}
    for size in ("1x1", "2x5", "5x2", "3x3", "17x23"):
        for kind in ("full_", "empty_", "random_"):
            assert kind + size in cases
    assert cases["n0_5x7"]["n"] == 0 and cases["n50_24x40"]["n"] == 50 and cases["full_3x3"]["n"] == 1
    assert cases["blobs_9x37"]["w"] % 16 != 0
    seams = cases["seams_40x530"]
    assert seams["h"] > 2 * 16 and seams["w"] > 2 * 256                       # more than two tiles of 256 x 16 each way
    for y, x in ((15, 255), (16, 256), (31, 511), (32, 512), (8, 15), (8, 16)):   # on both sides of the tile and run seams
        assert seams["masks"][:, y, x].any()
    g = cases["gradient_8x256"]
    assert g["seed"] == -1 and sorted(set(map(tuple, g["colors"].tolist()))) == [(0, 127, 255), (255, 0, 128)]
    assert set(g["image"][0, :, 0].tolist()) == set(range(256))
    for c in cases.values():
        assert c["image"].min() == 0 and c["image"].max() == 255, c["name"]
    pal = np.concatenate([c["colors"] for c in cases.values()])
    assert pal.min() == 0 and pal.max() == 255
    for kind in ("inside", "cross_top", "cross_left", "cross_bottom", "cross_right", "outside", "flat", "thin", "point", "frame",
                 "fractional", "negative_fractional"):
        assert f"box_{kind}_17x23" in cases
    assert cases["box_frame_17x23"]["boxes"].tolist() == [[0, 0, 16, 22]]
    assert not np.array_equal(cases["box_outside_17x23"]["want"], cases["box_inside_17x23"]["want"])
    assert np.array_equal(cases["box_outside_17x23"]["want"], cases["box_outside_17x23"]["image"])
    # Pillow's quirk: a box with y1 == y2 also colours the row below at its two end columns
    flat = cases["box_flat_17x23"]
    changed = np.argwhere((flat["want"] != flat["image"]).any(2)).tolist()
    assert [7, 3] in changed and [7, 14] in changed and [7, 8] not in changed and [6, 8] in changed
    assert str(load_golden("blend")["pillow"])


def test_host_route_equals_every_golden_case():
    for c in blend_cases():
        got = host(c)
        assert got.dtype == np.uint8 and got.shape == c["want"].shape, c["name"]
        bad = np.argwhere((got != c["want"]).any(2))
        assert bad.size == 0, (c["name"], len(bad), bad[:5].tolist())


def test_host_blend_equals_the_stored_table():
    """All 65 536 (pixel value, colour value) pairs of Image.blend at 0.2 through the host route: a 256 x 1 image of every pixel
    value under one all-on mask, three colour values per call (one per channel)."""
    from maskrcnn_amd import image
    table = load_golden("blend")["blend_table"]
    assert table.shape == (256, 256) and table.dtype == np.uint8
    got = np.empty((256, 256), np.uint8)
    col = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None], (256, 1, 3))
    for c0 in range(0, 256, 3):
        cs = [min(c0 + k, 255) for k in range(3)]
        out = image._blend_host(col, np.ones((1, 256, 1), bool), np.array([cs], np.uint8), None)
        for k, c in enumerate(cs):
            got[:, c] = out[:, 0, k]
    assert np.array_equal(got, table)
    # what the rule is NOT: the same expression with the float32 constant widened to double differs on thousands of pairs
    p, c = np.meshgrid(np.arange(256.0), np.arange(256.0), indexing="ij")
    assert np.array_equal(np.trunc(p + 0.2 * (c - p)).astype(np.uint8), table)
    assert np.count_nonzero(np.trunc(p + float(np.float32(0.2)) * (c - p)).astype(np.uint8) != table) > 1000


def test_random_colors_equals_the_stored_palettes():
    from maskrcnn_amd import image
    seen = 0
    for c in blend_cases():
        if c["seed"] < 0 or c["n"] == 0:
            continue
        random.seed(c["seed"])
        got = image.random_colors(c["n"])
        assert isinstance(got, list) and all(isinstance(t, tuple) and len(t) == 3 for t in got)
        assert np.array_equal(np.array(got, np.uint8), c["colors"]), c["name"]
        seen += 1
    assert seen > 40
    assert image.random_colors(3, shuffle=False) == [(255, 0, 0), (0, 255, 0), (0, 0, 255)]
    assert image.random_colors(2, bright=False, shuffle=False) == [(178, 0, 0), (0, 178, 178)]


def test_no_instances_returns_the_image():
    c = case("n0_5x7")
    assert np.array_equal(host(c), c["image"]) and np.array_equal(c["want"], c["image"])
    assert np.array_equal(host(c, boxes=None), c["image"])


def test_small_images_have_no_outline():
    """H < 3 or W < 3: every pixel is on the frame. A single on pixel changes that pixel alone."""
    rng = np.random.default_rng(3)
    for h, w in ((1, 1), (1, 7), (7, 1), (2, 5), (5, 2), (2, 2)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        m = np.zeros((1, h, w), np.uint8)
        m[0, h // 2, w // 2] = 1
        got = host(dict(image=img, boxes=None, masks=m, colors=np.array([[255, 0, 128]], np.uint8)))
        changed = (got != img).any(2)
        changed[h // 2, w // 2] = False
        assert not changed.any(), (h, w)


def test_extreme_boxes_change_nothing_and_raise_nothing():
    c = case("empty_17x23")
    for b in ([INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX], [INT32_MAX, 3, INT32_MAX, 9], [INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX],
              [INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN], [3, INT32_MAX, 9, INT32_MAX]):
        got = host(c, boxes=torch.tensor([b], dtype=torch.int32))
        assert np.array_equal(got, c["image"]), b
    # float boxes beyond int32 saturate instead of wrapping
    got = host(c, boxes=torch.tensor([[-1e12, -1e12, 1e12, 1e12]], dtype=torch.float64))
    assert np.array_equal(got, c["image"])


def test_inverted_box_raises_on_the_host_route():
    c = case("empty_17x23")
    for b in ([9, 3, 4, 12], [3, 12, 9, 4]):
        with pytest.raises(ValueError, match="blend_image: box"):
            host(c, boxes=np.array([b], np.float64))


def test_threshold_rule_and_bool_masks_on_the_host_route():
    c = case("overlap3_17x23")
    rng = np.random.default_rng(5)
    grey = np.where(c["masks"] > 0, rng.integers(128, 256, c["masks"].shape), rng.integers(0, 128, c["masks"].shape)).astype(np.uint8)
    assert np.array_equal(host(c, masks=torch.from_numpy(grey), threshold=None), c["want"])       # uint8: 127
    assert np.array_equal(host(c, masks=torch.from_numpy(grey), threshold=127), c["want"])
    assert np.array_equal(host(c, masks=torch.from_numpy(c["masks"] > 0), threshold=None), c["want"])   # bool: 0
    assert np.array_equal(host(c, masks=None), host(c, masks=torch.zeros(3, 17, 23, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="threshold"):
        host(c, threshold=255)


def test_header_declares_and_library_exports_the_entry_point():
    from maskrcnn_amd import _lib
    protos = _lib.header_prototypes()
    assert "mrcnn_blend_instances_u8" in _lib.declared_symbols() and hasattr(_lib.lib, "mrcnn_blend_instances_u8")
    res, args = protos["mrcnn_blend_instances_u8"]
    c_i32, c_i64, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert res == ctypes.c_int
    assert args == [c_vp, c_i64, c_vp, c_i64, c_i64, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_i64, c_vp]
    assert _lib.header_abi_version() >= 23 and _lib.lib.mrcnn_abi_version() == _lib.header_abi_version()


def test_entry_point_refuses_bad_arguments():
    """Argument validation runs before any HIP call (dummy pointers, never touched)."""
    from maskrcnn_amd import _lib
    lib = _lib.lib
    dp = ctypes.c_void_p(4096)

    def refused(text, image_rs=69, mask_is=391, mask_rs=23, n=1, h=17, w=23, t=0, out_rs=69):
        rc = lib.mrcnn_blend_instances_u8(dp, image_rs, dp, mask_is, mask_rs, dp, None, n, h, w, t, dp, out_rs, None)
        assert rc != 0 and text in lib.mrcnn_last_error(), (text, lib.mrcnn_last_error())

    refused(b"blend_instances: image 0x23", h=0)
    refused(b"blend_instances: image 17x16385", w=16385, image_rs=3 * 16385, out_rs=3 * 16385, mask_rs=16385)
    refused(b"blend_instances: n=-1", n=-1)
    refused(b"blend_instances: n=65536", n=65536)
    refused(b"blend_instances: threshold=255", t=255)
    refused(b"blend_instances: threshold=-1", t=-1)
    refused(b"is shorter than a row of 23 RGB pixels", image_rs=68)
    refused(b"is shorter than a row of 23 RGB pixels", out_rs=68)
    refused(b"mask row stride 22", mask_rs=22)
    refused(b"mask image stride -1", mask_is=-1)


def test_public_interface_and_cpu_refusal():
    from maskrcnn_amd import image, ops
    assert "blend_instances" in ops.__all__ and hasattr(torch.ops.maskrcnn, "blend_instances")
    for name in ("random_colors", "blend_image"):
        assert callable(getattr(image, name))
    img, m, col = torch.zeros(4, 5, 3, dtype=torch.uint8), torch.zeros(1, 4, 5, dtype=torch.uint8), torch.zeros(1, 3, dtype=torch.uint8)
    refused = pytest.raises(RuntimeError, match="Not compiled with CPU support")
    with refused:
        ops.blend_instances(img, m, col)
    with refused:
        ops.blend_instances(img, m, col, torch.zeros(1, 4, dtype=torch.int32), 0, img)
    with refused:
        torch.ops.maskrcnn.blend_instances(img, m, col, None, 0)
    with refused:
        torch.ops.maskrcnn.blend_instances(img, m, col, torch.zeros(1, 4, dtype=torch.int32), 127)


def test_host_route_never_touches_the_library(monkeypatch):
    from maskrcnn_amd import ops
    monkeypatch.setattr(ops, "blend_instances", lambda *a, **k: pytest.fail("the host route called into the library"))
    c = case("overlap3_17x23")
    assert np.array_equal(host(c), c["want"])


def test_predict_lists_render():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "predict.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--render" in r.stdout and "--seed" in r.stdout
