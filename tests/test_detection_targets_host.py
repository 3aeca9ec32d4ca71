"""Detection training targets without a GPU: the numpy route of maskrcnn_amd.targets.detection_targets equals what the reference's
model.mrn_samples produced (tests/golden/detection_targets.npz, made by tests/golden/make_golden_detection_targets.py) — every
integer output, rois_out, dy, dx and every mask target bit for bit, dh / dw within 2 fp32 ulps (detection_targets_cases.compare) —
plus the neg_limit table, the list / packed forms, the ValueErrors, the header's version and the library's exports."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from detection_targets_cases import EXPECTED, case, case_masks, cases, compare, images, usable

ENTRY_POINTS = ("mrcnn_detection_targets", "mrcnn_mask_targets_u8", "mrcnn_mask_targets_f32")


def numpy_route(c, **kw):
    from maskrcnn_amd import targets
    args = dict(count=c["count"], positive_ratio=c["ratio"], mask_shape=c["mask_shape"], keys=c["keys"], device="cpu")
    args.update(kw)
    return targets.detection_targets(c["rois"], c["boxes"], c["ids"], case_masks(c), gt_off=c["off"], **args)


def as_dict(t):
    """DetectionTargets → the names of detection_targets_cases.EXPECTED."""
    v = {k: getattr(t, k).cpu().numpy() for k in t._fields}
    v["rois_out"], v["class_ids"], v["deltas"] = v.pop("rois"), v.pop("target_class_ids"), v.pop("target_deltas")
    assert set(EXPECTED) <= set(v)
    return v


def test_fixture_covers_the_cases():
    from maskrcnn_amd import targets
    names = {c["name"] for c in cases()}
    for want in ("basic_b3", "basic_b3_count8", "basic_b3_count8_equal_keys", "basic_b3_count8_mod4_keys", "n1", "n63", "n65",
                 "n4096_rows50", "rows1024_n64", "both_limits_ratio0.33", "both_limits_ratio0.25", "both_limits_ratio0.5", "no_positives",
                 "only_positives", "thresholds", "row_ties", "crowds", "all_crowd_between", "zero_padded", "masks_outside",
                 "masks_outside_14x28", "midpoints_u8", "midpoints_f32", "basic_b3_mask1x1", "basic_b3_mask8x8", "basic_b3_ramp", "mask1024"):
        assert want in names, want
    b = case("basic_b3")
    assert np.diff(b["off"]).tolist() == [4, 3, 1] and b["rois"].shape == (3, 64, 4) and b["count"] == 100
    assert (b["num_pos"] < 33).all() and (b["num_pos"] > 0).all()                       # fewer positives than the limit,
    assert [int(1.0 / 0.33 * p - p) for p in b["num_pos"]] == b["num_neg"].tolist()      # negatives cut by neg_limit
    for name in ("basic_b3_count8", "basic_b3_count8_equal_keys", "basic_b3_count8_mod4_keys"):
        assert case(name)["num_pos"].tolist() == [2, 2, 2] and case(name)["num_neg"].tolist() == [4, 4, 4]
    assert (case("basic_b3_count8_equal_keys")["keys"] == 7).all() and case("basic_b3_count8_mod4_keys")["keys"].max() == 3
    assert case("n4096_rows50")["rois"].shape == (1, 4096, 4) and len(case("n4096_rows50")["ids"]) == 50
    assert len(case("rows1024_n64")["ids"]) == 1024 and case("rows1024_n64")["gt_index"].max() > 255
    for name, (p, q) in (("both_limits_ratio0.33", (33, 67)), ("both_limits_ratio0.25", (25, 75)), ("both_limits_ratio0.5", (50, 50)),
                         ("n4096_rows50", (33, 67))):
        assert (case(name)["num_pos"].tolist(), case(name)["num_neg"].tolist()) == ([p], [q]), name
    n = case("no_positives")
    cls = targets.roi_match_numpy(n["rois"][0], n["boxes"], n["ids"])[0]
    assert (cls == 1).all() and n["num_pos"].tolist() == n["num_neg"].tolist() == [0]    # negatives exist, none is kept
    o = case("only_positives")
    assert o["num_pos"].tolist() == [16] and o["num_neg"].tolist() == [0]
    t = case("thresholds")
    cls, _, iou, _ = targets.roi_match_numpy(t["rois"][0], t["boxes"], t["ids"])
    assert cls.tolist() == [0, 1] and iou[0] == np.float32(0.5) and iou[1] == np.nextafter(np.float32(0.5), np.float32(0))
    assert t["roi_index"][0, :2].tolist() == [0, 1] and t["class_ids"][0, :2].tolist() == [7, 0]
    r = case("row_ties")
    assert set(r["gt_index"][0, :r["num_pos"][0]].tolist()) == {0, 2} and set(r["class_ids"][0, :r["num_pos"][0]].tolist()) == {11, 13}
    cr = case("crowds")
    cls0 = targets.roi_match_numpy(cr["rois"][0], *images(cr)[0])[0]
    assert (cls0[40:43] == 2).all()                                                      # RoIs inside the crowd: neither class
    assert 1 not in cr["gt_index"][0, :cr["num_pos"][0]].tolist()                        # the id-0 row beside a crowd is dropped
    p1 = cr["num_pos"][1]
    assert 0 in cr["class_ids"][1, :p1].tolist() and 0 in cr["gt_index"][1, :p1].tolist()   # without a crowd it is kept: class 0
    assert case("all_crowd_between")["status"].tolist() == [0, 1, 0]
    z = case("zero_padded")
    assert not z["rois"][0, 27:].any() and (z["roi_index"][0, z["num_pos"][0]:30] >= 27).any()   # a zero row is a sampled negative
    assert (case("masks_outside")["rois"] < 0).any() and (case("masks_outside")["rois"] > 1).any()
    assert case("masks_outside_14x28")["mask_shape"] == (14, 28) and case("basic_b3_mask1x1")["mask_shape"] == (1, 1)
    m = case("midpoints_u8")
    assert m["mask_shape"] == (2, 3) and m["target_mask"][0, 0].tolist() == [[0, 0, 0], [1, 1, 1]]      # 0.5 -> 0
    m = case("midpoints_f32")
    assert m["target_mask"][0, 0].tolist() == [[2, 2, 2], [2, 3, 3]]                     # 1.5 -> 2
    assert m["target_mask"][1, 0].tolist() == [[2, 3, 3], [3, 4, 4]]                     # 2.5 -> 2, 3.5 -> 4
    assert case("basic_b3_mask8x8")["mask_hw"] == (8, 8) and case("mask1024")["mask_hw"] == (1024, 1024)
    assert case_masks(case("basic_b3_ramp")).dtype == np.float32 and 0 < case_masks(case("basic_b3_ramp")).max() <= 1


def test_numpy_route_equals_the_fixture():
    differing = worst = total = 0
    for c in cases():
        if not usable(c):
            continue
        got = numpy_route(c)
        assert all(v.dtype == (torch.float32 if k in ("rois", "target_deltas", "target_mask") else torch.int32) for k, v in zip(got._fields, got))
        d, w = compare(c, as_dict(got))
        differing, worst, total = differing + d, max(worst, w), total + 2 * int(c["num_pos"].sum())
    print(f"dh / dw against the reference's fp32 log, all cases: {differing} of {total} values differ, largest distance {worst} ulp")


def test_numpy_functions_equal_the_fixture_image_by_image_with_an_unusable_image():
    """all_crowd_between cannot go through the front end (it raises); its three images go through the exported functions."""
    from maskrcnn_amd import targets
    c = case("all_crowd_between")
    masks = case_masks(c)
    for i, (boxes, ids) in enumerate(images(c)):
        cls, arg, _, status = targets.roi_match_numpy(c["rois"][i], boxes, ids)
        idx, p, q = targets.roi_sample_numpy(cls, c["keys"][i], c["count"], c["ratio"])
        assert (status, p, q) == (c["status"][i], c["num_pos"][i], c["num_neg"][i])
        assert np.array_equal(idx, c["roi_index"][i]) and np.array_equal(arg[idx[:p]], c["gt_index"][i, :p])
        deltas = targets.roi_deltas_numpy(c["rois"][i][idx[:p]], boxes[arg[idx[:p]]])
        assert np.array_equal(deltas[:, :2], c["deltas"][i, :p, :2])
        got = targets.mask_targets_numpy(masks[c["off"][i]:c["off"][i + 1]], arg[idx[:p]], c["rois"][i][idx[:p]], c["mask_shape"])
        assert np.array_equal(got, c["target_mask"][i, :p])


@pytest.mark.parametrize("ratio", [0.33, 0.25, 0.5, 1.0])
def test_neg_limit_is_the_references_expression(ratio):
    from maskrcnn_amd import targets
    count = 1000
    pos_limit = int(count * ratio)
    keys = np.arange(2 * count, dtype=np.int32)
    for p in range(pos_limit + 1):
        cls = np.ones(2 * count, np.int32)                         # p positives and more negatives than any limit
        cls[:p] = 0
        idx, num_pos, num_neg = targets.roi_sample_numpy(cls, keys, count, ratio)
        assert num_pos == p and num_neg == int(1.0 / ratio * p - p), (ratio, p)
        assert idx[:p].tolist() == list(range(p)) and (idx[p + num_neg:] == -1).all()
    cls = np.zeros(2 * count, np.int32)
    assert targets.roi_sample_numpy(cls, keys, count, ratio)[1] == pos_limit
    if ratio == 0.33:
        assert [targets.roi_sample_numpy(np.r_[np.zeros(p, int), np.ones(300, int)], np.arange(p + 300), 100, 0.33)[2]
                for p in (0, 1, 2, 31, 32, 33, 60)] == [0, 2, 4, 62, 64, 67, 67]


def test_list_and_packed_forms_agree():
    from maskrcnn_amd import targets
    for name in ("basic_b3_count8_mod4_keys", "crowds"):
        c = case(name)
        masks = case_masks(c)
        bs, cs = zip(*images(c))
        ms = [masks[s:e] for s, e in zip(c["off"][:-1], c["off"][1:])]
        packed = numpy_route(c)
        lists = targets.detection_targets(list(c["rois"]), list(bs), list(cs), ms, c["count"], c["ratio"], mask_shape=c["mask_shape"],
                                          keys=c["keys"], device="cpu")
        tensors = targets.detection_targets(torch.from_numpy(c["rois"].copy()), [torch.from_numpy(b.copy()) for b in bs],
                                            [torch.from_numpy(i.copy()) for i in cs], [torch.from_numpy(m.copy()) for m in ms], c["count"],
                                            c["ratio"], mask_shape=c["mask_shape"], keys=torch.from_numpy(c["keys"].copy()), device="cpu")
        for a, b, d in zip(packed, lists, tensors):
            assert torch.equal(a, b) and torch.equal(a, d) and a.dtype == b.dtype == d.dtype
        # unpad: the reference's shapes
        for i in range(c["batch"]):
            n = int(c["num_pos"][i] + c["num_neg"][i])
            r, k, d, m = packed.unpad(i)
            assert tuple(r.shape) == (n, 4) and tuple(k.shape) == (n,) and tuple(d.shape) == (n, 4) and tuple(m.shape) == (n, *c["mask_shape"])
            assert np.array_equal(r.numpy(), c["rois_out"][i, :n]) and np.array_equal(k.numpy(), c["class_ids"][i, :n])
    empty = numpy_route(case("no_positives")).unpad(0)
    assert [tuple(t.shape) for t in empty] == [(0,)] * 4 and empty[1].dtype == torch.int32


def test_drawn_keys_on_the_cpu_route_give_valid_counts():
    from maskrcnn_amd import targets
    c = case("both_limits_ratio0.33")
    run = lambda seed: numpy_route(c, keys=None, generator=torch.Generator().manual_seed(seed))
    a, b, d = run(3), run(3), run(4)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a.roi_index, d.roi_index)
    cls = targets.roi_match_numpy(c["rois"][0], c["boxes"], c["ids"])[0]
    idx = a.roi_index[0].numpy()
    assert a.num_pos.tolist() == [33] and a.num_neg.tolist() == [67]
    assert (cls[idx[:33]] == 0).all() and (cls[idx[33:]] == 1).all() and len(set(idx.tolist())) == 100


def test_value_errors_name_the_image():
    from maskrcnn_amd import targets
    c = case("all_crowd_between")
    masks = case_masks(c)
    bs, cs = (list(v) for v in zip(*images(c)))
    ms = [masks[s:e] for s, e in zip(c["off"][:-1], c["off"][1:])]
    run = lambda rois=c["rois"], b=bs, i=cs, m=ms, **kw: targets.detection_targets(rois, b, i, m, device="cpu", **kw)
    with pytest.raises(ValueError, match="detection_targets: image 1 has no usable ground truth"):
        run()
    with pytest.raises(ValueError, match="detection_targets: image 1 has no usable ground truth"):
        targets.detection_targets(c["rois"], c["boxes"], c["ids"], masks, gt_off=c["off"], device="cpu")
    good = dict(rois=c["rois"][[0, 2]], b=[bs[0], bs[2]], i=[cs[0], cs[2]], m=[ms[0], ms[2]])
    assert run(**good).status.tolist() == [0, 0]
    flipped = bs[2].copy()
    flipped[1, [0, 2]] = flipped[1, [2, 0]]
    with pytest.raises(ValueError, match="image 1: boxes must be finite with y2 >= y1"):
        run(**{**good, "b": [bs[0], flipped]})
    bad_rois = good["rois"].copy()
    bad_rois[0, 5, 3] = np.nan
    with pytest.raises(ValueError, match="image 0: rois must be finite"):
        run(**{**good, "rois": bad_rois})
    many = np.tile(bs[0][:1], (1025, 1))
    with pytest.raises(ValueError, match="image 0 has 1025 rows; at most 1024"):
        run(**{**good, "b": [many, bs[2]], "i": [np.ones(1025, np.int32), cs[2]], "m": [np.zeros((1025, 4, 4), np.uint8), np.zeros((3, 4, 4), np.uint8)]})
    with pytest.raises(ValueError, match="N=4097 rois per image; at most 4096"):
        run(**{**good, "rois": np.zeros((2, 4097, 4), np.float32)})
    with pytest.raises(ValueError, match=r"image 1: gt_masks must be \[G,H,W\] with one mask per box \(3\)"):
        run(**{**good, "m": [ms[0], ms[2][:2]]})
    b3 = case("basic_b3")
    with pytest.raises(ValueError, match=r"gt_masks must be \[M,H,W\] with one row per row of gt_boxes \(8\)"):
        targets.detection_targets(b3["rois"], b3["boxes"], b3["ids"], case_masks(b3)[:7], gt_off=b3["off"], device="cpu")
    with pytest.raises(ValueError, match="uint8, bool or float32"):
        run(**{**good, "m": [ms[0].astype(np.int32), ms[2].astype(np.int32)]})
    for kw, msg in ((dict(count=0), "count=0"), (dict(count=1025), "count=1025"), (dict(positive_ratio=0.0), "positive_ratio"),
                    (dict(positive_ratio=1.5), "positive_ratio"), (dict(mask_shape=(65, 28)), "mask_shape")):
        with pytest.raises(ValueError, match=msg):
            run(**good, **kw)


def test_header_version_and_exports():
    from maskrcnn_amd import _lib, ops, targets
    assert _lib.header_abi_version() >= 25 and int(_lib.lib.mrcnn_abi_version()) == _lib.header_abi_version()
    declared, protos = _lib.declared_symbols(), _lib.header_prototypes()
    for name in ENTRY_POINTS:
        assert name in declared and name in protos
        fn = getattr(_lib.lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == protos[name][1]
    args = protos["mrcnn_detection_targets"][1]
    assert len(args) == 22 and args[9] is ctypes.c_double and args[12] == ctypes.POINTER(ctypes.c_float) and args[-1] is ctypes.c_void_p
    assert len(protos["mrcnn_mask_targets_u8"][1]) == len(protos["mrcnn_mask_targets_f32"][1]) == 14
    for name in ("detection_targets", "mask_targets"):
        assert name in ops.__all__ and callable(getattr(ops, name)) and hasattr(torch.ops.maskrcnn, name)
    for name in ("detection_targets", "DetectionTargets", "roi_match_numpy", "roi_sample_numpy", "roi_deltas_numpy", "mask_targets_numpy"):
        assert name in targets.__all__ and hasattr(targets, name)
    header = open(_lib.HEADER).read()
    block = header[header.index("Detection training targets"):]
    for phrase in ("model.py:396-576", "FIRST kept row", "pos_limit", "neg_limit", "BugFixed", "ties to even", "1024 rows per image"):
        assert phrase in block, phrase
    build = open(f"{ROOT}/maskrcnn_amd/build.py").read()
    assert re.search(r'"detection_targets\.hip": \["-ffp-contract=off"\]', build)
    src = open(f"{ROOT}/maskrcnn_amd/csrc/detection_targets.hip").read()
    assert "#pragma clang fp contract(off)" in src and '#include "crop_math.hpp"' in src


def test_the_ops_refuse_cpu_tensors():
    from maskrcnn_amd import ops
    c = case("basic_b3")
    t = [torch.from_numpy(np.array(v)) for v in (c["rois"], c["boxes"], c["ids"], c["off"], c["keys"])]
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.detection_targets(*t)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        torch.ops.maskrcnn.detection_targets(*t)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.mask_targets(torch.zeros(8, 4, 4, dtype=torch.uint8), t[3], torch.zeros(3, 5, 4), torch.zeros(3, 5, dtype=torch.int32),
                         torch.zeros(3, dtype=torch.int32))


def test_the_library_validates_its_arguments():
    """Host-side checks of the C entry points, reachable without a GPU: they fail before any launch."""
    from maskrcnn_amd import _lib
    lib = _lib.lib
    std = (ctypes.c_float * 4)(0.1, 0.1, 0.2, 0.2)
    p = ctypes.c_void_p(16)           # never dereferenced: every call below is refused first

    def targets_rc(batch=1, n=8, m=2, count=8, ratio=0.33):
        return lib.mrcnn_detection_targets(p, p, p, p, p, batch, n, m, count, ratio, 0.5, 0.001, std, p, p, p, p, p, p, p, p, None)

    def masks_rc(fn=lib.mrcnn_mask_targets_u8, m=2, h=8, w=8, batch=1, count=8, mh=28, mw=28):
        return fn(p, m, h, w, p, batch, count, p, p, p, mh, mw, p, None)

    for kw, msg in ((dict(n=0), "num_rois=0"), (dict(n=4097), "num_rois=4097"), (dict(count=0), "count=0"), (dict(count=1025), "count=1025"),
                    (dict(batch=0), "batch=0"), (dict(batch=65536), "batch=65536"), (dict(m=1025), "at most 1024 rows per image"),
                    (dict(ratio=0.0), "positive_ratio"), (dict(ratio=1.25), "positive_ratio"), (dict(ratio=float("nan")), "positive_ratio")):
        assert targets_rc(**kw) != 0 and msg in lib.mrcnn_last_error().decode(), kw
    for fn in (lib.mrcnn_mask_targets_u8, lib.mrcnn_mask_targets_f32):
        for kw, msg in ((dict(h=0), "height and width"), (dict(w=16385), "height and width"), (dict(mh=0), "mask_height"),
                        (dict(mw=65), "mask_height"), (dict(count=1025), "count=1025"), (dict(batch=0), "batch=0"),
                        (dict(m=1025), "at most 1024 rows per image")):
            assert masks_rc(fn, **kw) != 0 and msg in lib.mrcnn_last_error().decode(), kw
    assert lib.mrcnn_detection_targets(None, p, p, p, p, 1, 8, 2, 8, 0.33, 0.5, 0.001, std, p, p, p, p, p, p, p, p, None) != 0
    assert "null pointer" in lib.mrcnn_last_error().decode()
