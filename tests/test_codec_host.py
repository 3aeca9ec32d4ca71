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


def test_merge_tables_places_rows_by_index_and_zero_fills():
    """image._merge_tables on CPU tensors: parts of different widths out of index order, a row no part covers, stale values
    behind num_runs in the input, and a capacity wider than every part."""
    from maskrcnn_amd import image
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    wide = ([3, 0], i32([2, 1]), i32([[7, 8, 99, 98], [5, 97, 96, 95]]))            # rows 3 and 0: 4 wide, stale tails
    narrow = (np.array([2]), i32([4]), i32([[1, 2, 3, 4]]))
    short = ([2], i32([2]), i32([[6, 9, 94]]))                                      # 3 wide
    for parts, capacity, width in (([wide, narrow], None, 4), ([short, wide], None, 4), ([wide, narrow], 7, 7), ([short], None, 3)):
        num_runs, counts = image._merge_tables(5, parts, "cpu", capacity)
        assert num_runs.dtype == torch.int32 and counts.dtype == torch.int32 and tuple(counts.shape) == (5, width)
        want = np.zeros((5, width), np.int64)
        for idx, nr, c in parts:
            for i, n, row in zip(list(idx), nr.tolist(), c.tolist()):
                want[i, :n] = row[:n]
        assert counts.tolist() == want.tolist()
        assert num_runs.tolist() == [int(np.count_nonzero(r)) for r in want]         # every live run here is non-zero
    assert image._merge_tables(5, [wide, narrow], "cpu")[0].tolist() == [1, 0, 4, 2, 0]
    empty = image._merge_tables(3, [], "cpu")
    assert empty[0].tolist() == [0, 0, 0] and tuple(empty[1].shape) == (3, 1) and not empty[1].any()


def test_build_table_on_the_host_with_one_size_per_entry(monkeypatch):
    """image._build_table with the host string decoder: dicts, bare strings, count lists and a skipped row of two sizes equal
    _pack_table of rle_counts of each entry; of two bad entries the lower index is named. The library is not touched."""
    from maskrcnn_amd import image, ops
    from test_rle_host import golden_cases
    for name in ("rle_from_string", "rle_area_bbox", "rle_encode"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("the host route called into the library"))
    by_size = {}
    for c in golden_cases():
        by_size.setdefault(c["mask"].shape, []).append(c)
    small, (big, big2) = by_size[29, 13][0], by_size[60, 90][:2]
    objs = [{"size": [60, 90], "counts": big["string"]}, small["string"], big2["counts"].tolist(), [[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]],
            {"size": [29, 13], "counts": small["counts"].tolist()}, big2["string"].decode("ascii")]
    sizes = [(60, 90), (29, 13), (60, 90), (0, 0), (29, 13), (60, 90)]
    skip = [False, False, False, True, False, False]
    rows = [np.zeros(0, np.uint32) if s else image.rle_counts(o) for o, s in zip(objs, skip)]
    assert [r.size for r in rows] == [big["counts"].size, small["counts"].size, big2["counts"].size, 0, small["counts"].size, big2["counts"].size]
    for device, host_strings in (("cpu", False), ("cpu", True)):
        num_runs, counts = image._build_table(objs, sizes, device, skip=skip, host_strings=host_strings)
        want = image._pack_table(rows, "cpu")
        assert torch.equal(num_runs, want[0]) and torch.equal(counts, want[1]) and counts.dtype == torch.int32
    wide = image._build_table(objs, sizes, "cpu", counts.size(1) + 3, skip=skip)
    assert torch.equal(wide[1], image._pack_table(rows, "cpu", counts.size(1) + 3)[1])
    with pytest.raises(ValueError, match="rle_table: capacity 5 is less than the longest mask's"):
        image._build_table(objs, sizes, "cpu", 5, skip=skip)
    with pytest.raises(ValueError, match=r"rle_table: mask 4 is \[29, 13\], the table is \[60, 90\]"):
        image._build_table(objs, [(60, 90)] * 6, "cpu", skip=[False, True, False, True, False, False])
    with pytest.raises(ValueError, match="rle_table: the runs of mask 0 cover 30 pixels, the mask has 60 x 90"):
        image._build_table([[10, 20], [5000, 0, 400], big["string"]], [(60, 90)] * 3, "cpu")
    with pytest.raises(ValueError, match="ground truth: mask 1 has an empty run after the first one"):
        image._build_table([big["string"], [5000, 0, 400], [10, 20]], [(60, 90)] * 3, "cpu", prefix="ground truth")
    with pytest.raises(ValueError, match="rle_table: mask 0 has an empty run after the first one"):
        image.rle_table([[5000, 0, 400], [10, 20]], (60, 90), "cpu")
