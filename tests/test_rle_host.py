"""COCO RLE without a GPU: the pure-numpy reader of maskrcnn_amd.image (rle_counts / rle_decode) against the golden vectors made
with the reference's own codec (tests/golden/make_golden_rle.py: rleEncode / rleToString / rleArea / rleToBbox of
cocoapi/common/maskApi.c), and the boundary of the encoder: header, exported symbols, signatures, loud CPU refusal."""
import inspect

import numpy as np
import pytest
import torch

from conftest import load_golden


def golden_cases():
    z = load_golden("rle")
    for k, name in enumerate(z["names"].tolist()):
        h, w = (int(v) for v in z["shapes"][k])
        mask = np.unpackbits(z["bits"][z["bit_off"][k]:z["bit_off"][k + 1]])[:h * w].reshape(h, w).astype(bool)
        yield dict(name=name, mask=mask, counts=z["counts"][z["cnt_off"][k]:z["cnt_off"][k + 1]],
                   string=z["strings"][z["str_off"][k]:z["str_off"][k + 1]].tobytes(), area=int(z["areas"][k]),
                   bbox=z["bboxes"][k].tolist())


def test_golden_fixture_covers_the_cases():
    cases = list(golden_cases())
    names = " ".join(c["name"] for c in cases)
    assert len(cases) >= 40
    for kind in ("random", "empty", "full", "1x1", "row_1x", "col_", "checker", "first_pixel", "wrap", "width3_", "ellipse", "blob"):
        assert kind in names, kind
    for c in cases:   # the fixture is consistent with itself: the counts cover the mask, the area is the on-pixel count
        assert int(c["counts"].astype(np.int64).sum()) == c["mask"].size and c["area"] == int(c["mask"].sum()), c["name"]


def test_rle_decode_of_golden_strings_and_count_lists():
    from maskrcnn_amd import image
    for c in golden_cases():
        size = list(c["mask"].shape)
        assert np.array_equal(image.rle_decode({"size": size, "counts": c["string"]}), c["mask"]), c["name"]
        assert np.array_equal(image.rle_decode({"size": size, "counts": c["string"].decode("ascii")}), c["mask"]), c["name"]
        assert np.array_equal(image.rle_decode({"size": size, "counts": c["counts"].tolist()}), c["mask"]), c["name"]
        assert np.array_equal(image.rle_decode(c["counts"].tolist(), size=size), c["mask"]), c["name"]
        got = image.rle_decode({"size": size, "counts": c["string"]})
        assert got.dtype == np.bool_ and got.shape == c["mask"].shape


def test_rle_counts_of_golden_strings():
    from maskrcnn_amd import image
    for c in golden_cases():
        got = image.rle_counts(c["string"])
        assert got.dtype == np.uint32 and np.array_equal(got, c["counts"]), c["name"]
        assert np.array_equal(image.rle_counts({"size": list(c["mask"].shape), "counts": c["string"]}), c["counts"])
        assert np.array_equal(image.rle_counts(c["counts"].tolist()), c["counts"])
    with pytest.raises(ValueError):
        image.rle_decode([3, 2], size=(2, 2))           # five pixels of runs for a four-pixel mask
    with pytest.raises(ValueError):
        image.rle_decode([4])                           # raw counts need a size


def test_header_declares_and_library_exports_the_rle_entry_points():
    from maskrcnn_amd import _lib
    declared = _lib.declared_symbols()
    protos = _lib.header_prototypes()
    for name in ("mrcnn_rle_workspace_bytes", "mrcnn_rle_encode_u8"):
        assert name in declared and name in protos
        assert hasattr(_lib.lib, name)
    assert len(protos["mrcnn_rle_encode_u8"][1]) == 17 and len(protos["mrcnn_rle_workspace_bytes"][1]) == 3
    # sizing needs no GPU: nothing for an empty call or a refused size, something otherwise
    ws = _lib.lib.mrcnn_rle_workspace_bytes
    assert ws(0, 64, 64) == 0 and ws(1, 16385, 4) == 0 and ws(1, 4, 0) == 0
    assert ws(2, 64, 64) > 0 and ws(50, 1200, 1920) >= 50 * 1920 * 8


def test_public_interface():
    from maskrcnn_amd import image, ops
    from maskrcnn_amd.pipeline import MaskRCNNInference
    p = inspect.signature(MaskRCNNInference.detect).parameters
    assert p["mask_format"].default == "dense" and list(p)[:3] == ["self", "images", "timings"]
    assert "rle_encode" in ops.__all__
    assert ops.rle_default_capacity(1200, 1920) == 4 * 1920 + 2 and ops.rle_default_capacity(64, 64) == 1024
    assert ops.rle_default_capacity(3, 3) == 10
    assert hasattr(torch.ops.maskrcnn, "rle_encode")
    for name in ("RleMasks", "rle_decode", "rle_counts"):
        assert hasattr(image, name)


def test_rle_encode_refuses_cpu_tensors():
    from maskrcnn_amd import ops
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.rle_encode(torch.zeros(2, 8, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        torch.ops.maskrcnn.rle_encode(torch.zeros(2, 8, 8, dtype=torch.uint8), 0, None)
