"""COCO evaluation on the GPU: ops.rle_iou / ops.bbox_iou / ops.coco_match (csrc/cocoeval.hip) and maskrcnn_amd.cocoeval.evaluate
against tests/golden/cocoeval.npz — the reference's own maskApi.c and cocoeval.py (tests/golden/make_golden_cocoeval.py) — and,
for inputs the fixture does not hold, against the numpy restatements of tests/test_cocoeval_host.py, which that file pins to the
same golden. Everything is integer work or separately rounded fp64: every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_cocoeval_host import (AREA_RNG, IOU_THRS, bbox_iou_ref, evaluate_img_ref, golden_eval_imgs, golden_groups,
                                golden_inputs, golden_ious, rle_iou_ref, same_eval_img, seg_counts, to_eval_img)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ_LIB = os.path.join(ROOT, "maskrcnn_amd", "csrc", "build", "variants", "sync_fuzz", "libmaskrcnn_hip.so")
DEV = torch.device("cuda:0")


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


def offsets(dt_n, gt_n):
    dt_n, gt_n = np.asarray(dt_n, dtype=np.int64), np.asarray(gt_n, dtype=np.int64)
    z = lambda v: np.concatenate([[0], np.cumsum(v)])
    return z(dt_n), z(gt_n), z(dt_n * gt_n)


def dev_offsets(offs):
    return dev(offs[0], np.int32), dev(offs[1], np.int32), dev(offs[2], np.int64)


class Fixture:
    """The golden data set laid out for grouped calls: every (image, category) that has a detection or a ground truth, in
    sorted order — groups without detections and groups without ground truths included."""

    def __init__(self):
        from maskrcnn_amd import image
        self.groups = golden_groups()
        self.keys = sorted(self.groups)
        self.dts = [x for k in self.keys for x in self.groups[k][0]]
        self.gts = [x for k in self.keys for x in self.groups[k][1]]
        self.offs = offsets([len(self.groups[k][0]) for k in self.keys], [len(self.groups[k][1]) for k in self.keys])
        self.iscrowd = np.array([g["iscrowd"] for g in self.gts], dtype=np.uint8)
        rows = lambda anns: [seg_counts(x["segmentation"]) for x in anns]
        self.dt_table, self.gt_table = image._pack_table(rows(self.dts), DEV), image._pack_table(rows(self.gts), DEV)
        boxes = lambda anns: dev(np.array([x["bbox"] for x in anns], dtype=np.float64).reshape(-1, 4))
        self.dt_boxes, self.gt_boxes = boxes(self.dts), boxes(self.gts)

    def iou(self, iou_type, **kw):
        from maskrcnn_amd import ops
        if iou_type == "segm":
            return ops.rle_iou(self.dt_table, self.gt_table, dev(self.iscrowd), *dev_offsets(self.offs), **kw)
        return ops.bbox_iou(self.dt_boxes, self.gt_boxes, dev(self.iscrowd), *dev_offsets(self.offs), **kw)

    def matrix(self, flat, k):
        d, g = len(self.groups[self.keys[k]][0]), len(self.groups[self.keys[k]][1])
        return flat[self.offs[2][k]:self.offs[2][k + 1]].reshape(g, d).T


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def blob_masks(n, h, w, seed, rmin, rmax):
    """n blob-shaped masks [n,h,w] uint8 made ON the device."""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: (torch.rand(n, generator=g) * (hi - lo) + lo).to(DEV).view(n, 1, 1)
    cy, cx, r, p1, p2 = u(0.1 * h, 0.9 * h), u(0.1 * w, 0.9 * w), u(rmin, rmax), u(0, 6), u(0, 6)
    k1, k2 = torch.randint(2, 5, (n,), generator=g).to(DEV).view(n, 1, 1), torch.randint(5, 9, (n,), generator=g).to(DEV).view(n, 1, 1)
    yy, xx = torch.arange(h, device=DEV).view(1, h, 1).float(), torch.arange(w, device=DEV).view(1, 1, w).float()
    out = torch.empty(n, h, w, dtype=torch.uint8, device=DEV)
    for i in range(0, n, 8):
        s = slice(i, i + 8)
        ang = torch.atan2(yy - cy[s], xx - cx[s])
        rad = r[s] * (1 + 0.25 * torch.sin(k1[s] * ang + p1[s]) + 0.12 * torch.cos(k2[s] * ang + p2[s]))
        out[s] = torch.hypot(yy - cy[s], xx - cx[s]) <= rad
    return out


def host_rows(num_runs, counts):
    nr, c = num_runs.cpu().numpy(), counts.cpu().numpy().view(np.uint32)
    return [c[i, :nr[i]] for i in range(len(nr))]


def match_ref(ious_flat, offs, dt_area, gt_area, crowd):
    """evaluate_img_ref for every group x area range → the four arrays ops.coco_match returns."""
    K, N, M, A, T = len(offs[0]) - 1, int(offs[0][-1]), int(offs[1][-1]), len(AREA_RNG), len(IOU_THRS)
    dtm, gtm = np.zeros((A, T, N), np.int32), np.zeros((A, T, M), np.int32)
    dtig, gtig = np.zeros((A, T, N), np.uint8), np.zeros((A, M), np.uint8)
    for k in range(K):
        d0, d1, g0, g1 = offs[0][k], offs[0][k + 1], offs[1][k], offs[1][k + 1]
        ious = ious_flat[offs[2][k]:offs[2][k] + (g1 - g0) * (d1 - d0)].reshape(g1 - g0, d1 - d0).T
        for a, rng in enumerate(AREA_RNG):
            r = evaluate_img_ref(ious, dt_area[d0:d1], gt_area[g0:g1], crowd[g0:g1], rng, IOU_THRS)
            dtm[a, :, d0:d1], gtm[a, :, g0:g1], dtig[a, :, d0:d1], gtig[a, g0:g1] = r[:4]
    return dtm, gtm, dtig, gtig


def coco_match_dev(ious, offs, dt_area, gt_area, crowd, **kw):
    from maskrcnn_amd import ops
    return ops.coco_match(ious, *dev_offsets(offs), dev(dt_area, np.float64), dev(gt_area, np.float64), dev(crowd, np.uint8),
                          dev(AREA_RNG, np.float64), dev(IOU_THRS, np.float64), **kw)


# ------------------------------------------------------------------------------------------------ against the golden
@pytest.mark.parametrize("iou_type", ["segm", "bbox"])
def test_iou_equals_the_golden_grouped_and_group_by_group(fx, iou_type):
    from maskrcnn_amd import ops
    want = golden_ious(iou_type)
    flat = fx.iou(iou_type)
    assert flat.dtype == torch.float64 and flat.shape == (int(fx.offs[2][-1]),)
    flat = flat.cpu().numpy()
    seen = 0
    for k, key in enumerate(fx.keys):
        got = fx.matrix(flat, k)
        d0, d1, g0, g1 = fx.offs[0][k], fx.offs[0][k + 1], fx.offs[1][k], fx.offs[1][k + 1]
        if d1 == d0 or g1 == g0:
            assert key not in want and got.size == 0
            continue
        assert np.array_equal(got, want[key]), (iou_type, key)
        crowd = dev(fx.iscrowd[g0:g1])
        if iou_type == "segm":      # the single-group form on this group's rows: the same bits
            one = ops.rle_iou((fx.dt_table[0][d0:d1], fx.dt_table[1][d0:d1]), (fx.gt_table[0][g0:g1], fx.gt_table[1][g0:g1]), crowd)
        else:
            one = ops.bbox_iou(fx.dt_boxes[d0:d1], fx.gt_boxes[g0:g1], crowd)
        assert one.shape == want[key].shape and np.array_equal(one.cpu().numpy(), want[key]), (iou_type, key)
        seen += 1
    assert seen == len(want)
    assert np.array_equal(fx.iou(iou_type).cpu().numpy(), flat)                   # run to run


@pytest.mark.parametrize("iou_type", ["segm", "bbox"])
def test_coco_match_equals_the_golden_grouped_and_group_by_group(fx, iou_type):
    ious = fx.iou(iou_type)
    dt_area = np.array([x["area"] for x in fx.dts], dtype=np.float64)
    gt_area = np.array([x["area"] for x in fx.gts], dtype=np.float64)
    out = [o.cpu().numpy() for o in coco_match_dev(ious, fx.offs, dt_area, gt_area, fx.iscrowd)]
    again = [o.cpu().numpy() for o in coco_match_dev(ious, fx.offs, dt_area, gt_area, fx.iscrowd)]
    assert all(np.array_equal(a, b) for a, b in zip(out, again))
    entries = {(e["image_id"], e["category_id"], e["a"]): e for e in golden_eval_imgs(iou_type) if e is not None}
    ious_host = ious.cpu().numpy()
    for k, key in enumerate(fx.keys):
        d, g = fx.groups[key]
        d0, d1, g0, g1 = fx.offs[0][k], fx.offs[0][k + 1], fx.offs[1][k], fx.offs[1][k + 1]
        one_offs = offsets([d1 - d0], [g1 - g0])
        one = [o.cpu().numpy() for o in coco_match_dev(dev(ious_host[fx.offs[2][k]:fx.offs[2][k + 1]]), one_offs, dt_area[d0:d1],
                                                       gt_area[g0:g1], fx.iscrowd[g0:g1])]
        for a, rng in enumerate(AREA_RNG):
            got = to_eval_img(key, rng, d, g, out[0][a, :, d0:d1], out[1][a, :, g0:g1], out[2][a, :, d0:d1], out[3][a, g0:g1])
            assert same_eval_img(got, entries.pop((key[0], key[1], a))), (iou_type, key, a)
        assert np.array_equal(one[0], out[0][:, :, d0:d1]) and np.array_equal(one[1], out[1][:, :, g0:g1])
        assert np.array_equal(one[2], out[2][:, :, d0:d1]) and np.array_equal(one[3], out[3][:, g0:g1])
    assert not entries                                                             # every golden entry was compared


@pytest.mark.parametrize("iou_type", ["segm", "bbox"])
def test_evaluate_end_to_end_equals_the_golden(iou_type):
    from maskrcnn_amd import cocoeval
    z = load_golden("cocoeval")
    gt, results = golden_inputs()
    ev = cocoeval.evaluate(gt, results, iou_type)
    for name in ("precision", "recall", "scores", "stats"):
        got, want = getattr(ev, name), z[f"{iou_type}_{name}"]
        assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want), name
    assert ev.summary() == z[f"{iou_type}_summary"].tolist()
    want_ious = golden_ious(iou_type)
    assert len(ev.ious) == len(gt["images"]) * len(gt["categories"])
    for key, got in ev.ious.items():
        if key in want_ious:
            assert np.array_equal(got, want_ious[key]), key
        else:
            assert len(got) == 0, key
    want_imgs = golden_eval_imgs(iou_type)
    assert len(ev.eval_imgs) == len(want_imgs)
    for i, (got, want) in enumerate(zip(ev.eval_imgs, want_imgs)):
        assert same_eval_img(got, want), i


def test_evaluate_reads_files_and_the_cli_prints_the_summary(tmp_path):
    import json
    from maskrcnn_amd import cocoeval
    z = load_golden("cocoeval")
    (tmp_path / "gt.json").write_text(str(z["gt_json"]))
    (tmp_path / "res.json").write_text(str(z["results_json"]))
    ev = cocoeval.evaluate(str(tmp_path / "gt.json"), str(tmp_path / "res.json"), "bbox")
    assert np.array_equal(ev.stats, z["bbox_stats"])
    r = subprocess.run([sys.executable, "-m", "maskrcnn_amd.cocoeval", str(tmp_path / "gt.json"), str(tmp_path / "res.json"),
                        "--type", "segm"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.splitlines() == z["segm_summary"].tolist()
    # dense ground-truth masks are encoded on the GPU: the same numbers
    from maskrcnn_amd import image
    gt = json.loads(str(z["gt_json"]))
    for ann in gt["annotations"][::2]:
        ann["segmentation"] = image.rle_decode(ann["segmentation"])
    assert np.array_equal(cocoeval.evaluate(gt, str(tmp_path / "res.json"), "segm").stats, z["segm_stats"])


def test_scoring_results_made_from_the_ground_truth_gives_ap_ar_one():
    """Every regular ground truth as its own detection, distinct scores: all true positives. pr = tp / (fp + tp + spacing(1))
    is then tp / (tp + 2^-52) >= 1 - 2^-52 and recall is exactly 1, so AP / AR lie within a few ulp of 1 (bound: 1e-12);
    AR at maxDets 1 and 10 is capped by the detections allowed per image and is only required not to exceed 1."""
    from maskrcnn_amd import cocoeval
    gt, _ = golden_inputs()
    regular = [a for a in gt["annotations"] if not a["iscrowd"]]
    for iou_type in ("segm", "bbox"):
        results = [{"image_id": a["image_id"], "category_id": a["category_id"], "score": 1.0 - 0.001 * i, "bbox": a["bbox"],
                    "segmentation": a["segmentation"]} for i, a in enumerate(regular)]
        ev = cocoeval.evaluate(gt, results, iou_type)
        for key, m in ev.ious.items():
            if len(m):
                assert (np.asarray(m).max(axis=1) == 1.0).all(), key          # a mask / box against itself is exactly 1
        for i in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11):
            assert ev.stats[i] == -1 or abs(ev.stats[i] - 1) < 1e-12, (iou_type, i, ev.stats[i])
        assert abs(ev.stats[0] - 1) < 1e-12 and abs(ev.stats[8] - 1) < 1e-12
        assert 0 < ev.stats[6] <= ev.stats[7] <= 1
        assert ev.summary()[0].endswith("= 1.000")


# ------------------------------------------------------------------------------------------------ against the restatement
def test_rle_iou_on_encoder_output_without_a_host_trip():
    """100 x 30 blob masks at 1200 x 1920 straight from ops.rle_encode's device tensors, some ground truths crowds."""
    from maskrcnn_amd import image, ops
    h, w = 1200, 1920
    dt = image.rle_masks(blob_masks(100, h, w, 1, 60, 320))
    gt = image.rle_masks(blob_masks(30, h, w, 2, 80, 400))
    crowd = (np.arange(30) % 4 == 1).astype(np.uint8)
    got = dt.iou(gt, crowd.tolist())
    assert got.shape == (100, 30) and got.dtype == torch.float64 and got.is_cuda
    want = rle_iou_ref(host_rows(dt.num_runs, dt.counts), host_rows(gt.num_runs, gt.counts), crowd)
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want > 0.3).sum() > 20 and (want == 0).sum() > 100                    # overlapping and disjoint pairs both
    assert torch.equal(ops.rle_iou(dt, (gt.num_runs, gt.counts), dev(crowd)), got)   # tensors or RleMasks; run to run
    assert torch.equal(torch.ops.maskrcnn.rle_iou(dt.num_runs, dt.counts, gt.num_runs, gt.counts, dev(crowd)), got)
    # and the matching on it: one group of 100 x 30
    areas_d, areas_g = dt.areas.cpu().numpy().astype(np.float64), gt.areas.cpu().numpy().astype(np.float64)
    offs = offsets([100], [30])
    flat = ops.rle_iou(dt, gt, dev(crowd), *dev_offsets(offs), out_len=3000)
    assert np.array_equal(flat.cpu().numpy().reshape(30, 100).T, want)
    out = [o.cpu().numpy() for o in coco_match_dev(flat, offs, areas_d, areas_g, crowd)]
    for a, b in zip(out, match_ref(flat.cpu().numpy(), offs, areas_d, areas_g, crowd)):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert (out[0] > 0).sum() > 50


def test_empty_full_and_one_pixel_masks():
    from maskrcnn_amd import image
    h, w = 37, 53
    m = torch.zeros(7, h, w, dtype=torch.uint8, device=DEV)
    m[1] = 1                                   # full
    m[2, 0, 0] = 1                             # the first pixel
    m[3, h - 1, w - 1] = 1                     # the last pixel
    m[4, 10, 20] = 1                           # one pixel inside
    m[5, 5:30, 10:40] = 1
    m[6, :, 20] = 1                            # a whole column
    enc = image.rle_masks(m)
    rows = host_rows(enc.num_runs, enc.counts)
    for crowd in (None, [0, 1, 0, 1, 1, 0, 1]):
        got = enc.iou(enc, crowd).cpu().numpy()
        assert np.array_equal(got, rle_iou_ref(rows, rows, crowd))
    assert got[0].tolist() == [0.0] * 7 and got[1, 1] == 1.0 and got[5, 1] == 1.0          # a crowd: the detection's own area
    assert got[4, 5] == 1.0 / 750 and got[5, 4] == 1.0 / 750 and got[2, 3] == 0.0
    # count lists from the host (rle_table) against encoder output
    table = image.rle_table([{"size": [h, w], "counts": r.tolist()} for r in rows], (h, w))
    assert np.array_equal(enc.iou(table).cpu().numpy(), rle_iou_ref(rows, rows))


def test_bbox_iou_against_the_restatement():
    from maskrcnn_amd import ops
    rng = np.random.default_rng(5)
    dt = np.concatenate([rng.uniform(0, 500, (300, 2)), rng.uniform(0.1, 300, (300, 2))], 1)
    gt = np.concatenate([rng.uniform(0, 500, (200, 2)), rng.uniform(0.1, 300, (200, 2))], 1)
    gt[:40] = dt[:40]                                                             # identical boxes
    gt[40:60, :2] = dt[40:60, :2] + dt[40:60, 2:]                                 # touching corners: w == 0 or h == 0
    gt[60] = [10, 10, 0, 0]                                                       # an empty box
    dt[299] = [20, 20, 0, 5]
    crowd = (rng.uniform(size=200) < 0.3).astype(np.uint8)
    got = ops.bbox_iou(dev(dt), dev(gt), dev(crowd))
    want = bbox_iou_ref(dt, gt, crowd)
    assert got.shape == (300, 200) and np.array_equal(got.cpu().numpy(), want)
    assert (want > 0).sum() > 1000 and (want == 0).sum() > 1000
    assert np.array_equal(ops.bbox_iou(dev(dt), dev(gt)).cpu().numpy(), bbox_iou_ref(dt, gt))


def small_random_problem(K, seed):
    """K groups of 0..3 detections and 0..3 ground truths: 48 x 64 block masks encoded on the device."""
    from maskrcnn_amd import image
    rng = np.random.default_rng(seed)
    dt_n, gt_n = rng.integers(0, 4, K), rng.integers(0, 4, K)
    if K > 1:
        dt_n[0], gt_n[1] = 0, 0                     # the first two groups are empty on one side each
        dt_n[-1], gt_n[-1] = 3, 0                   # ... and so is the last
    else:
        dt_n[0], gt_n[0] = 3, 2
    offs = offsets(dt_n, gt_n)
    g = torch.Generator().manual_seed(seed)
    masks = lambda n: (torch.rand(n, 6, 8, generator=g) < 0.45).to(torch.uint8).repeat_interleave(8, 1).repeat_interleave(8, 2).to(DEV)
    dt, gt = image.rle_masks(masks(int(offs[0][-1]))), image.rle_masks(masks(int(offs[1][-1])))
    crowd = (rng.uniform(size=int(offs[1][-1])) < 0.2).astype(np.uint8)
    return offs, dt, gt, crowd


@pytest.mark.parametrize("K", [1, 2500])
def test_grouped_calls_for_one_group_and_for_thousands(K):
    from maskrcnn_amd import ops
    offs, dt, gt, crowd = small_random_problem(K, 100 + K)
    out_len = int(offs[2][-1])
    flat = ops.rle_iou(dt, gt, dev(crowd), *dev_offsets(offs), out_len=out_len).cpu().numpy()
    rows_d, rows_g = host_rows(dt.num_runs, dt.counts), host_rows(gt.num_runs, gt.counts)
    want = np.zeros(out_len)
    for k in range(K):
        d0, d1, g0, g1 = offs[0][k], offs[0][k + 1], offs[1][k], offs[1][k + 1]
        want[offs[2][k]:offs[2][k + 1]] = rle_iou_ref(rows_d[d0:d1], rows_g[g0:g1], crowd[g0:g1]).T.reshape(-1)
    assert np.array_equal(flat, want) and (want > 0).sum() > out_len // 2
    # boxes of the same masks, same grouping
    bd, bg = dt.bboxes.double(), gt.bboxes.double()
    flat_b = ops.bbox_iou(bd, bg, dev(crowd), *dev_offsets(offs), out_len=out_len).cpu().numpy()
    want_b = np.zeros(out_len)
    for k in range(K):
        d0, d1, g0, g1 = offs[0][k], offs[0][k + 1], offs[1][k], offs[1][k + 1]
        want_b[offs[2][k]:offs[2][k + 1]] = bbox_iou_ref(bd[d0:d1].cpu().numpy(), bg[g0:g1].cpu().numpy(), crowd[g0:g1]).T.reshape(-1)
    assert np.array_equal(flat_b, want_b)
    # the matching; areas spread over the three size ranges
    rng = np.random.default_rng(K)
    dt_area, gt_area = rng.choice([500.0, 1024.0, 3000.0, 9216.0, 20000.0], len(rows_d)), rng.choice([500.0, 3000.0, 20000.0], len(rows_g))
    got = [o.cpu().numpy() for o in coco_match_dev(dev(flat), offs, dt_area, gt_area, crowd)]
    for a, b in zip(got, match_ref(flat, offs, dt_area, gt_area, crowd)):
        assert a.shape == b.shape and np.array_equal(a, b)


def test_a_mask_over_capacity_gives_minus_one_and_leaves_its_neighbours_exact():
    from maskrcnn_amd import image, ops
    h, w = 48, 64
    m = blob_masks(6, h, w, 9, 8, 25)
    yy, xx = torch.meshgrid(torch.arange(h, device=DEV), torch.arange(w, device=DEV), indexing="ij")
    m[2] = ((yy + xx) % 2).to(torch.uint8)                                        # a checkerboard: 3072 runs
    enc = image.RleMasks((h, w), *ops.rle_encode(m, capacity=256))
    assert int(enc.num_runs[2]) > 256 and int(enc.num_runs.max().item()) == int(enc.num_runs[2])
    full = image.rle_masks(m)                                                     # the same masks, all fitting
    rows = host_rows(full.num_runs, full.counts)
    want = rle_iou_ref(rows, rows)
    got = enc.iou(enc).cpu().numpy()
    keep = np.array([0, 1, 3, 4, 5])
    assert (got[2, :] == -1).all() and (got[:, 2] == -1).all()
    assert np.array_equal(got[np.ix_(keep, keep)], want[np.ix_(keep, keep)])
    mixed = enc.iou(full).cpu().numpy()                                           # only the detection side overflows
    assert (mixed[2] == -1).all() and np.array_equal(mixed[keep], want[keep])


def test_nothing_is_written_outside_the_outputs():
    """Sentinel bands round every output buffer, and elements of the IoU buffer that belong to no group, stay untouched."""
    from maskrcnn_amd import ops
    offs, dt, gt, crowd = small_random_problem(300, 77)
    offs = (offs[0], offs[1], offs[2] + 3 * np.arange(len(offs[2])))              # three unowned elements between matrices
    out_len, band = int(offs[2][-1]) + 5, 64
    owned = np.zeros(out_len, bool)
    for k in range(300):
        owned[offs[2][k]:offs[2][k] + (offs[0][k + 1] - offs[0][k]) * (offs[1][k + 1] - offs[1][k])] = True
    for which in ("rle", "bbox"):
        buf = torch.full((out_len + 2 * band,), -7.25, dtype=torch.float64, device=DEV)
        if which == "rle":
            ops.rle_iou(dt, gt, dev(crowd), *dev_offsets(offs), out_len=out_len, out=buf[band:band + out_len])
        else:
            ops.bbox_iou(dt.bboxes.double(), gt.bboxes.double(), dev(crowd), *dev_offsets(offs), out_len=out_len, out=buf[band:band + out_len])
        host = buf.cpu().numpy()
        assert (host[:band] == -7.25).all() and (host[band + out_len:] == -7.25).all(), which
        body = host[band:band + out_len]
        assert (body[~owned] == -7.25).all() and (body[owned] >= 0).all() and (body[owned] <= 1).all(), which
    N, M, A, T = int(offs[0][-1]), int(offs[1][-1]), len(AREA_RNG), len(IOU_THRS)
    sizes, dtypes = (A * T * N, A * T * M, A * T * N, A * M), (torch.int32, torch.int32, torch.uint8, torch.uint8)
    shapes = ((A, T, N), (A, T, M), (A, T, N), (A, M))
    bufs = [torch.full((n + 2 * band,), 99, dtype=d, device=DEV) for n, d in zip(sizes, dtypes)]
    ious = buf[band:band + out_len].clone()
    dt_area, gt_area = dt.areas.double().cpu().numpy(), gt.areas.double().cpu().numpy()
    got = coco_match_dev(ious, offs, dt_area, gt_area, crowd, out=tuple(b[band:band + n].view(s) for b, n, s in zip(bufs, sizes, shapes)))
    for b, n in zip(bufs, sizes):
        host = b.cpu().numpy()
        assert (host[:band] == 99).all() and (host[band + n:] == 99).all() and (host[band:band + n] != 99).all()
    for a, b in zip([o.cpu().numpy() for o in got], match_ref(ious.cpu().numpy(), offs, dt_area, gt_area, crowd)):
        assert np.array_equal(a, b)


def test_bad_arguments_are_refused():
    from maskrcnn_amd import image, ops
    enc = image.rle_masks(blob_masks(3, 32, 32, 3, 5, 10))
    with pytest.raises(RuntimeError, match="come together"):
        ops.rle_iou(enc, enc, None, dev([0, 3], np.int32))
    with pytest.raises(RuntimeError, match="iscrowd"):
        ops.rle_iou(enc, enc, dev([0, 1], np.uint8))
    with pytest.raises(RuntimeError, match=r"float64 \[N,4\]"):
        ops.bbox_iou(enc.bboxes, enc.bboxes)
    with pytest.raises(ValueError, match="against masks of"):
        enc.iou(image.rle_masks(blob_masks(2, 32, 40, 4, 5, 10)))


# ------------------------------------------------------------------------------------------------ schedule fuzzing
def test_kernel_tests_pass_under_schedule_fuzzing():
    """This file's kernel tests in a fresh process on the schedule-fuzzing build (tests/test_gpu_sync_fuzz.py)."""
    assert os.path.exists(FUZZ_LIB), f"{FUZZ_LIB} is missing: run __graft_entry__.build()"
    env = dict(os.environ, MRCNN_LIB=FUZZ_LIB, MRCNN_SYNC_FUZZ_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_cocoeval.py", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider",
                        "-k", "not schedule_fuzzing and not cli"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
