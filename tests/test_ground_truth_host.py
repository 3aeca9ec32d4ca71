"""Host tests (no GPU) of ground_truth.load_batch: the device="cpu" route — numpy and Pillow — against
tests/golden/ground_truth.npz, which tests/golden/make_golden_ground_truth.py writes from the reference's own
CocoMaskRCNNDataset.load, encode_image, encode_masks and encode_boxes. Boxes are compared bit for bit, masks on the reference's
extent with the rest of the canvas zero. tests/test_gpu_ground_truth.py runs the same comparison on the device route."""
import copy
import json
from typing import NamedTuple

import numpy as np
import pytest
import torch

from conftest import load_golden


class Case(NamedTuple):
    gt: dict
    labels: dict
    min_dim: int
    max_dim: int
    image_ids: list
    flips: list
    counts: list          # rows per image
    ids: np.ndarray       # int32 [M]: load()'s label_ids
    boxes: np.ndarray     # uint32 [M,4]
    scales: list
    windows: np.ndarray   # int64 [B,4]
    shapes: np.ndarray    # int64 [B,2]: the reference's mask extent per image
    masks: list           # per image uint8 [count, H, W]


def fixture_cases():
    g = load_golden("ground_truth")
    gt = json.loads(str(g["gt_json"]))
    labels = {c: int(v) for c, v in enumerate(g["from_class"].tolist()) if v >= 0}
    row_off = np.concatenate([[0], np.cumsum(g["exp_count"])])
    cases = []
    for c in range(len(g["case_min_dim"])):
        t0, t1 = int(g["case_off"][c]), int(g["case_off"][c + 1])
        masks = []
        for t in range(t0, t1):
            n, (h, w) = int(g["exp_count"][t]), g["exp_mask_shape"][t]
            bits = np.unpackbits(g["exp_masks"][int(g["exp_mask_off"][t]):int(g["exp_mask_off"][t + 1])])
            masks.append(bits[:n * h * w].reshape(n, h, w))
        cases.append(Case(gt, labels, int(g["case_min_dim"][c]), int(g["case_max_dim"][c]), g["case_image_ids"][t0:t1].tolist(),
                          [bool(v) for v in g["case_flips"][t0:t1]], g["exp_count"][t0:t1].tolist(),
                          g["exp_labels"][row_off[t0]:row_off[t1]], g["exp_boxes"][row_off[t0]:row_off[t1]],
                          g["exp_scale"][t0:t1].tolist(), g["exp_window"][t0:t1], g["exp_mask_shape"][t0:t1], masks))
    return cases


def same_as_fixture(got, case: Case):
    """got: a GroundTruth made with crowds="reference"."""
    off = np.concatenate([[0], np.cumsum(case.counts)])
    assert got.gt_off.dtype == torch.int32 and got.gt_off.cpu().numpy().tolist() == off.tolist()
    assert got.gt_class_ids.dtype == torch.int32 and np.array_equal(got.gt_class_ids.cpu().numpy(), case.ids)
    assert got.gt_boxes.dtype == torch.float32 and got.gt_boxes.shape == (off[-1], 4)
    assert np.array_equal(got.gt_boxes.cpu().numpy().view(np.uint32), case.boxes)
    assert got.scales == case.scales and got.flips == case.flips
    assert got.windows.dtype == torch.int64 and np.array_equal(got.windows.cpu().numpy(), case.windows)
    masks = got.gt_masks.cpu().numpy()
    assert masks.dtype == np.uint8 and masks.shape == (off[-1], case.max_dim, case.max_dim)
    for i, want in enumerate(case.masks):
        mine = masks[off[i]:off[i + 1]]
        h, w = want.shape[1:]
        assert h <= case.max_dim and w <= case.max_dim
        assert np.array_equal(mine[:, :h, :w], want), (case.image_ids[i], case.flips[i])
        assert not mine[:, h:].any() and not mine[:, :, w:].any()


@pytest.fixture(scope="module")
def cases():
    return fixture_cases()


@pytest.fixture(scope="module")
def gtlib():
    from maskrcnn_amd import ground_truth
    return ground_truth


def test_the_fixture_holds_the_cases_the_rule_needs(cases):
    gt = cases[0].gt
    kinds = {("poly" if isinstance(a["segmentation"], list) else "string" if isinstance(a["segmentation"]["counts"], str) else "counts",
              int(a["iscrowd"])) for a in gt["annotations"]}
    assert {("poly", 0), ("string", 0), ("counts", 0), ("string", 1)} <= kinds
    assert any(a["category_id"] == 0 for a in gt["annotations"])
    sizes = {img["id"]: [img["height"], img["width"]] for img in gt["images"]}
    assert any(a["iscrowd"] and isinstance(a["segmentation"], dict) and a["segmentation"]["size"] != sizes[a["image_id"]]
               for a in gt["annotations"])
    scales = [s for c in cases for s in c.scales]
    assert any(s > 1 for s in scales) and any(0.6 < s < 0.7 for s in scales) and any(s <= 0.25 for s in scales) and 1 in scales
    assert any(c.counts[i] == 1 and c.ids[sum(c.counts[:i])] == 0 for c in cases for i in range(len(c.counts)))      # the fake row
    assert {True, False} == {f for c in cases for f in c.flips}
    pads = [(c.max_dim - (w[2] - w[0]), c.max_dim - (w[3] - w[1])) for c in cases for w, s in zip(c.windows, c.scales) if s != 1]
    assert any(p[0] % 2 for p in pads) and any(p[1] % 2 for p in pads) and any(not p[0] % 2 and not p[1] % 2 for p in pads)
    assert any(1 in sizes[i] for c in cases for i in c.image_ids)


def test_load_batch_on_the_host_equals_the_reference(cases, gtlib):
    for case in cases:
        got = gtlib.load_batch(case.gt, case.image_ids, case.min_dim, case.max_dim, hflip=case.flips, crowds="reference",
                               labels=case.labels, device="cpu")
        assert all(t.device.type == "cpu" for t in got[:5])
        same_as_fixture(got, case)


def test_load_batch_reads_a_file_and_one_image_at_a_time(cases, gtlib, tmp_path):
    case = cases[-1]
    path = tmp_path / "gt.json"
    path.write_text(json.dumps(case.gt))
    whole = gtlib.load_batch(str(path), case.image_ids, case.min_dim, case.max_dim, hflip=case.flips, crowds="reference", device="cpu")
    same_as_fixture(whole, case)
    off = whole.gt_off.tolist()
    for i, image_id in enumerate(case.image_ids):
        one = gtlib.load_batch(case.gt, [image_id], case.min_dim, case.max_dim, hflip=[case.flips[i]], crowds="reference", device="cpu")
        assert torch.equal(one.gt_masks, whole.gt_masks[off[i]:off[i + 1]]) and torch.equal(one.gt_boxes, whole.gt_boxes[off[i]:off[i + 1]])
    empty = gtlib.load_batch(case.gt, [], case.min_dim, case.max_dim, device="cpu")
    assert empty.gt_boxes.shape == (0, 4) and empty.gt_off.tolist() == [0] and empty.gt_masks.shape == (0, case.max_dim, case.max_dim)


def test_the_default_label_map_is_from_class(cases, gtlib):
    labels = gtlib.default_labels(cases[0].gt)
    assert labels == cases[0].labels and len(labels) == 81 and labels[90] == 80 and labels[0] == 0


def test_negative_crowds_differ_from_the_reference_mode_in_the_sign_only(cases, gtlib):
    case = cases[0]
    ref = gtlib.load_batch(case.gt, case.image_ids, case.min_dim, case.max_dim, hflip=case.flips, crowds="reference", device="cpu")
    neg = gtlib.load_batch(case.gt, case.image_ids, case.min_dim, case.max_dim, hflip=case.flips, device="cpu")
    crowd_of = {a["id"]: bool(a["iscrowd"]) for a in case.gt["annotations"]}
    for a, b in zip(ref[:5], neg[:5]):
        if a is not ref.gt_class_ids:
            assert torch.equal(a, b)
    flipped = (ref.gt_class_ids != neg.gt_class_ids).numpy()
    assert np.array_equal(neg.gt_class_ids.numpy(), np.where(flipped, -ref.gt_class_ids.numpy(), ref.gt_class_ids.numpy()))
    assert (ref.gt_class_ids >= 0).all()
    # two crowd rows per ordinary image, one per one-pixel image, none in the image where nothing is kept
    assert int(flipped.sum()) == 2 * 6 + 2 and sum(crowd_of.values()) > int(flipped.sum()) / 2


def test_flips_from_a_seed_and_a_generator(gtlib):
    a = gtlib._flips(5, 64)
    assert a == gtlib._flips(torch.Generator().manual_seed(5), 64) and set(a) == {True, False} and a != gtlib._flips(6, 64)
    assert gtlib._flips(None, 3) == [False] * 3 and gtlib._flips([1, 0, True], 3) == [True, False, True]
    with pytest.raises(ValueError, match="hflip has 2 entries for 3 images"):
        gtlib._flips([True, False], 3)


def test_each_error_names_its_image_or_annotation(cases, gtlib):
    case = cases[0]
    load = lambda gt, ids=(11,), **kw: gtlib.load_batch(gt, list(ids), case.min_dim, case.max_dim, device="cpu", **kw)
    with pytest.raises(ValueError, match="image id 999 is not in the data set"):
        load(case.gt, (11, 999))
    with pytest.raises(ValueError, match="crowds='sideways'"):
        load(case.gt, crowds="sideways")

    def broken(change):
        gt = copy.deepcopy(case.gt)
        ann = next(a for a in gt["annotations"] if a["image_id"] == 11 and isinstance(a["segmentation"], dict) and not a["iscrowd"]
                   and a["category_id"])
        change(ann, gt)
        return gt, ann["id"]

    gt, i = broken(lambda a, gt: a.pop("segmentation"))
    with pytest.raises(ValueError, match=f"annotation {i} has no segmentation"):
        load(gt)
    gt, i = broken(lambda a, gt: a.update(category_id=12))                 # a hole of COCO's ids (the reference: KeyError)
    with pytest.raises(ValueError, match=f"annotation {i} has category id 12"):
        load(gt)
    gt, i = broken(lambda a, gt: a["segmentation"].update(size=[31, 40]))
    with pytest.raises(ValueError, match=rf"annotation {i} is an RLE of \[31, 40\] on an image of \[30, 40\]"):
        load(gt)
    gt, i = broken(lambda a, gt: a.update(segmentation={"size": [30, 40], "counts": [5, 7]}))
    with pytest.raises(ValueError, match=f"annotation {i}: .*cover 12 pixels"):
        load(gt)
    gt, i = broken(lambda a, gt: a.update(segmentation=[[1.0, 2.0, 3.0, 4.0]]))
    with pytest.raises(ValueError, match=f"annotation {i}: the first part has 4 numbers"):
        load(gt)
    # sizes the op refuses, found before anything is launched
    gt = copy.deepcopy(case.gt)
    gt["annotations"] = [a for a in gt["annotations"] if isinstance(a["segmentation"], list)]      # polygons take any image size
    gt["images"][0].update(height=2000, width=40)                                                  # 2000 x 40 -> 64 x 1: 40 > 16
    assert gt["images"][0]["id"] == 11
    with pytest.raises(ValueError, match=r"image 11 \(2000 x 40\): shrinking to 64 x 1 is by more than 16"):
        load(gt)
    gt["images"][0].update(height=20000, width=4000)
    with pytest.raises(ValueError, match=r"image 11 \(20000 x 4000\): sizes must be in \[1, 16384\]"):
        load(gt)
    # more rows for one image than the target ops take
    gt = copy.deepcopy(case.gt)
    keep = next(a for a in gt["annotations"] if a["image_id"] == 18 and not a["iscrowd"])
    gt["annotations"] = [dict(keep, id=10000 + k) for k in range(1025)]
    with pytest.raises(ValueError, match="image 0 of the batch has 1025 ground-truth rows; the target ops take 1024"):
        load(gt, (18,))
