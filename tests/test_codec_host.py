"""The COCO RLE codec on tables without a GPU: tests/golden/codec.npz (made with the reference's own rleToString / rleFrString /
rleArea / rleToBbox / rleDecode: tests/golden/make_golden_codec.py) against the numpy readers that are already trusted
(image.rle_counts, image.rle_decode, cocoeval._rle_area_bbox), and the boundary of the new entry points: header, exported
symbols, loud CPU refusal, the host token counter, and the host routes that must never touch the library."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden


def codec_cases():
    z = load_golden("codec")
    out = []
    for k, name in enumerate(z["names"].tolist()):
        h, w = (int(v) for v in z["shapes"][k])
        c = dict(name=name, h=h, w=w, counts=z["counts"][z["cnt_off"][k]:z["cnt_off"][k + 1]],
                 string=z["strings"][z["str_off"][k]:z["str_off"][k + 1]].tobytes(), area=int(z["areas"][k]),
                 bbox=z["bboxes"][k].tolist(), mask=None)
        if z["has_bits"][k]:
            c["mask"] = np.unpackbits(z["bits"][z["bit_off"][k]:z["bit_off"][k + 1]])[:h * w].reshape(h, w).astype(bool)
        out.append(c)
    return out


def token_lengths(s: bytes):
    ends = np.flatnonzero(((np.frombuffer(s, np.uint8).astype(np.int16) - 48) & 0x20) == 0)
    return np.diff(np.concatenate([[-1], ends]))


def test_golden_fixture_covers_the_cases():
    cases = {c["name"]: c for c in codec_cases()}
    for k in range(6):
        assert cases[f"tokens{k}"]["counts"].size == k
    for d in (15, 16, -16, -17):
        assert int(cases[f"diff{d}"]["counts"][3]) - int(cases[f"diff{d}"]["counts"][1]) == d
    assert len(cases["diff15"]["string"]) + 1 == len(cases["diff16"]["string"])       # the sign boundary costs a character
    assert len(cases["diff-16"]["string"]) + 1 == len(cases["diff-17"]["string"])
    for k in range(1, 7):
        assert token_lengths(cases[f"toklen{k}"]["string"]).tolist() == [1, 1, k, 1, k]
    for n in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        s = cases[f"chars{n}"]["string"]
        assert len(s) == n
        ends = np.cumsum(token_lengths(s))                 # no token boundary at a multiple of 64: a token straddles every one
        assert not [e for e in ends.tolist() if e % 64 == 0 and e != n]
    for n in (63, 64, 65, 1023, 1024, 1025):
        assert cases[f"runs{n}_37"]["counts"].size == n
    assert cases["one_run_16384sq"]["counts"].tolist() == [0, 1 << 28] and cases["one_run_16384sq"]["area"] == 1 << 28
    assert cases["cross_column_24x10"]["bbox"] == [3, 0, 2, 24]                        # ys = 0, ye = h - 1
    for size in ("1x1", "1x9", "9x1", "5x7", "37x53", "64x61", "65x64", "33x130"):
        for kind in ("decode_", "decode_leading_zero_odd_", "decode_empty_", "decode_full_"):
            assert cases[kind + size]["mask"] is not None
    assert cases["decode_leading_zero_odd_37x53"]["counts"][0] == 0 and cases["decode_leading_zero_odd_37x53"]["counts"].size % 2 == 1
    for c in cases.values():
        s = np.frombuffer(c["string"], np.uint8)
        assert ((s >= 48) & (s <= 111)).all() and (token_lengths(c["string"]) <= 6).all(), c["name"]
    assert load_golden("codec")["fr_equal"].all()


def test_golden_is_consistent_with_the_numpy_readers():
    from maskrcnn_amd import cocoeval, image
    for c in codec_cases():
        got = image.rle_counts(c["string"])
        assert got.dtype == np.uint32 and np.array_equal(got, c["counts"]), c["name"]
        area, bbox = cocoeval._rle_area_bbox(c["counts"], c["h"], c["w"])
        assert np.uint32(area) == np.uint32(c["area"]) and [int(v) for v in bbox] == c["bbox"], c["name"]
        if c["mask"] is not None:
            assert np.array_equal(image.rle_decode(c["counts"].tolist(), size=(c["h"], c["w"])), c["mask"]), c["name"]


def test_host_token_counter_equals_the_reader_on_every_golden_string():
    from maskrcnn_amd import image, ops
    cases = codec_cases()
    data = np.frombuffer(b"".join(c["string"] for c in cases), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(c["string"]) for c in cases])])
    tokens = ops.rle_string_tokens(data, off)
    assert tokens.dtype == np.int64 and tokens.tolist() == [len(image.rle_counts(c["string"])) for c in cases]
    assert ops.rle_string_tokens(np.zeros(0, np.uint8), [0, 0, 0]).tolist() == [0, 0]


def test_header_declares_and_library_exports_the_codec_entry_points():
    from maskrcnn_amd import _lib
    declared, protos = _lib.declared_symbols(), _lib.header_prototypes()
    want = {"mrcnn_rle_from_string": 11, "mrcnn_rle_area_bbox": 9, "mrcnn_rle_to_string": 12, "mrcnn_rle_to_string_workspace_bytes": 1,
            "mrcnn_rle_decode_u8": 12, "mrcnn_rle_decode_workspace_bytes": 2}
    for name, nargs in want.items():
        assert name in declared and hasattr(_lib.lib, name) and len(protos[name][1]) == nargs, name
    assert _lib.header_abi_version() >= 22 and _lib.lib.mrcnn_abi_version() == _lib.header_abi_version()
    lib = _lib.lib
    assert lib.mrcnn_rle_to_string_workspace_bytes(0) == 0 and lib.mrcnn_rle_to_string_workspace_bytes(100) >= 800
    assert lib.mrcnn_rle_decode_workspace_bytes(0, 8) == 0 and lib.mrcnn_rle_decode_workspace_bytes(3, 100) >= 1200


def test_public_interface():
    from maskrcnn_amd import cocoeval, image, ops
    import inspect
    for name in ("rle_from_string", "rle_area_bbox", "rle_to_string", "rle_decode"):
        assert name in ops.__all__ and hasattr(torch.ops.maskrcnn, name), name
    assert hasattr(ops, "rle_to_string_rows")
    for name in ("rle_masks_from_table", "rle_decode_masks"):
        assert hasattr(image, name)
    assert hasattr(image.RleMasks, "decode")
    assert inspect.signature(cocoeval.load_results).parameters["device"].default is None
    assert inspect.signature(cocoeval.ann_to_rle).parameters["compress"].default is False


def test_the_ops_refuse_cpu_tensors():
    from maskrcnn_amd import ops
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    nr, counts = i32(2), torch.tensor([[3, 5]], dtype=torch.int32)
    refused = pytest.raises(RuntimeError, match="Not compiled with CPU support")
    with refused:
        ops.rle_from_string(torch.zeros(3, dtype=torch.uint8), torch.tensor([0, 3]), i32(2), i32(4), capacity=4)
    with refused:
        ops.rle_area_bbox(nr, counts, i32(2), i32(4))
    with refused:
        ops.rle_to_string(nr, counts)
    with refused:
        ops.rle_decode(nr, counts, 2, 4)
    with refused:
        torch.ops.maskrcnn.rle_from_string(torch.zeros(3, dtype=torch.uint8), torch.tensor([0, 3]), i32(2), i32(4), 4)
    with refused:
        torch.ops.maskrcnn.rle_area_bbox(nr, counts, i32(2), i32(4))
    with refused:
        torch.ops.maskrcnn.rle_to_string(nr, counts, None)
    with refused:
        torch.ops.maskrcnn.rle_decode(nr, counts, 2, 4)


def test_host_routes_never_touch_the_library(monkeypatch):
    """load_results(device=None) and rle_table(device="cpu") are the code they were: every ops entry point raises here."""
    from maskrcnn_amd import cocoeval, image, ops

    def boom(*a, **k):
        raise AssertionError("the host route called into the library")

    for name in ("rle_from_string", "rle_area_bbox", "rle_to_string", "rle_decode", "rle_encode", "rle_iou", "rle_merge", "rle_from_poly"):
        monkeypatch.setattr(ops, name, boom)
    z = load_golden("cocoeval")
    results = json.loads(str(z["results_json"]))
    segm_only = [{k: v for k, v in r.items() if k != "bbox"} for r in results]
    for device in (None, "cpu"):
        anns = cocoeval.load_results(segm_only, "segm") if device is None else cocoeval.load_results(segm_only, "segm", device)
        assert type(anns) is list and len(anns) == len(results)
        for a, r in zip(anns, results):
            cnts = image.rle_counts(r["segmentation"])
            area, bbox = cocoeval._rle_area_bbox(cnts, *r["segmentation"]["size"])
            assert type(a["area"]) is np.uint32 and a["area"] == area
            assert isinstance(a["bbox"], np.ndarray) and a["bbox"].dtype == np.float64 and a["bbox"].tolist() == bbox
    same = [r["segmentation"] for r in results if r["segmentation"]["size"] == [120, 160]]
    assert len(same) > 3
    mixed = same[:2] + [image.rle_counts(same[2]).tolist()] + [same[3]["counts"]]
    num_runs, counts = image.rle_table(mixed, (120, 160), device="cpu")
    assert num_runs.device.type == "cpu" and num_runs.dtype == torch.int32 and counts.dtype == torch.int32
    for i, obj in enumerate(mixed):
        want = image.rle_counts(obj)
        assert int(num_runs[i]) == want.size and np.array_equal(counts[i, :want.size].numpy().view(np.uint32), want)
