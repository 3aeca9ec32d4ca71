"""COCO evaluation without a GPU: the boundary of the three new entry points (header, exports, signatures, loud CPU refusal),
the input checks of image.rle_table and cocoeval.evaluate, and the host half of maskrcnn_amd.cocoeval (accumulate / summary) fed
with the golden evalImgs of tests/golden/cocoeval.npz (made by tests/golden/make_golden_cocoeval.py with the reference's own
maskApi.c and cocoeval.py). Also kept here: numpy restatements of rleIou, bbIou and evaluateImg, pinned to the golden on every
group, which tests/test_gpu_cocoeval.py uses for inputs the fixture does not hold."""
import inspect
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

T = 10   # IoU thresholds of Params


# ------------------------------------------------------------------------------------------------ restatements
def rle_iou_pair_ref(cd, cg, crowd):
    """rleIou (maskApi.c:82-95) for one pair of run lists: the merge of the two lists as array operations."""
    ed, eg = np.cumsum(np.asarray(cd, dtype=np.int64)), np.cumsum(np.asarray(cg, dtype=np.int64))
    pts = np.union1d(np.concatenate([[0], ed]), eg)
    start, length = pts[:-1], np.diff(pts)
    vd = np.searchsorted(ed, start, side="right") & 1      # a position lies in the run after every end at or before it
    vg = np.searchsorted(eg, start, side="right") & 1
    i, u = int(length[(vd & vg) == 1].sum()), int(length[(vd | vg) == 1].sum())
    if i == 0:
        u = 1
    elif crowd:
        u = int(np.asarray(cd, dtype=np.int64)[1::2].sum())
    return np.float64(i) / np.float64(u)


def rle_iou_ref(dt, gt, iscrowd=None):
    """→ float64 [len(dt), len(gt)] for lists of run lists."""
    out = np.zeros((len(dt), len(gt)))
    for g, cg in enumerate(gt):
        for d, cd in enumerate(dt):
            out[d, g] = rle_iou_pair_ref(cd, cg, iscrowd is not None and bool(iscrowd[g]))
    return out


def bbox_iou_ref(dt, gt, iscrowd=None):
    """bbIou (maskApi.c:109-120), every operation rounded on its own (numpy never fuses) → float64 [m, n]."""
    D, G = np.asarray(dt, dtype=np.float64).reshape(-1, 4)[:, None, :], np.asarray(gt, dtype=np.float64).reshape(-1, 4)[None, :, :]
    crowd = np.zeros(G.shape[1], bool) if iscrowd is None else np.asarray(iscrowd, dtype=bool)
    ga, da = G[..., 2] * G[..., 3], D[..., 2] * D[..., 3]
    w = np.fmin(D[..., 2] + D[..., 0], G[..., 2] + G[..., 0]) - np.fmax(D[..., 0], G[..., 0])
    h = np.fmin(D[..., 3] + D[..., 1], G[..., 3] + G[..., 1]) - np.fmax(D[..., 1], G[..., 1])
    i = w * h
    with np.errstate(divide="ignore", invalid="ignore"):
        o = i / np.where(crowd[None, :], np.broadcast_to(da, i.shape), da + ga - i)
    return np.where((w <= 0) | (h <= 0), 0.0, o)


def evaluate_img_ref(ious, dt_area, gt_area, gt_iscrowd, rng, thrs):
    """evaluateImg (cocoeval.py:251-300) for one group and one area range, on positions instead of ids.
    ious [D,G] (or anything empty), detections sorted and cut. → dt_match int32 [T,D], gt_match int32 [T,G] (1-based positions in
    INPUT order, 0 = none), dt_ignore uint8 [T,D], gt_ignore uint8 [G] (input order), gtind (the order evalImgs lists them in)."""
    D, G, nt = len(dt_area), len(gt_area), len(thrs)
    ig_in = np.array([1 if (gt_iscrowd[g] or gt_area[g] < rng[0] or gt_area[g] > rng[1]) else 0 for g in range(G)], dtype=np.int64)
    gtind = np.argsort(ig_in, kind="mergesort")
    gtIg = ig_in[gtind]
    iscrowd = [int(gt_iscrowd[i]) for i in gtind]
    have = D > 0 and G > 0
    if have:
        ious = np.asarray(ious)[:, gtind]
    gtm, dtm, dtIg = np.zeros((nt, G)), np.zeros((nt, D)), np.zeros((nt, D))
    if have:
        for tind, t in enumerate(thrs):
            for dind in range(D):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind in range(G):
                    if gtm[tind, gind] > 0 and not iscrowd[gind]:
                        continue
                    if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                        break
                    if ious[dind, gind] < iou:
                        continue
                    iou = ious[dind, gind]
                    m = gind
                if m == -1:
                    continue
                dtIg[tind, dind] = gtIg[m]
                dtm[tind, dind] = m + 1          # position in the SORTED order, turned back below
                gtm[tind, m] = dind + 1
    a = np.array([x < rng[0] or x > rng[1] for x in dt_area], dtype=bool).reshape((1, D))
    dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, nt, 0)))
    dt_match = np.where(dtm > 0, gtind[np.maximum(dtm.astype(np.int64), 1) - 1] + 1 if G else 0, 0).astype(np.int32).reshape(nt, D)
    gt_match = np.zeros((nt, G), np.int32)
    gt_match[:, gtind] = gtm.astype(np.int32)
    return dt_match, gt_match, dtIg.astype(np.uint8), ig_in.astype(np.uint8), gtind


# ------------------------------------------------------------------------------------------------ the fixture
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
IOU_THRS = np.linspace(.5, 0.95, 10)


def golden_inputs():
    z = load_golden("cocoeval")
    return json.loads(str(z["gt_json"])), json.loads(str(z["results_json"]))


def golden_groups():
    """{(image_id, category_id): (dts, gts)} as _prepare / computeIoU order them: the data set's order, detections by
    descending score (stable) and cut at 100; result ids are 1 + the record's index, areas w*h of the box (loadRes)."""
    gt, results = golden_inputs()
    groups = {}
    for ann in gt["annotations"]:
        groups.setdefault((ann["image_id"], ann["category_id"]), ([], []))[1].append(ann)
    for i, r in enumerate(results):
        r = dict(r, id=i + 1, area=r["bbox"][2] * r["bbox"][3])
        groups.setdefault((r["image_id"], r["category_id"]), ([], []))[0].append(r)
    out = {}
    for key, (d, g) in groups.items():
        order = np.argsort([-x["score"] for x in d], kind="mergesort")
        out[key] = ([d[i] for i in order][:100], g)
    return out


def golden_ious(iou_type):
    z = load_golden("cocoeval")
    out, off = {}, 0
    for key, (d, g) in zip(z[f"{iou_type}_iou_key"].tolist(), z[f"{iou_type}_iou_shape"].tolist()):
        out[tuple(key)] = z[f"{iou_type}_iou"][off:off + d * g].reshape(d, g)
        off += d * g
    assert off == z[f"{iou_type}_iou"].size
    return out


def golden_eval_imgs(iou_type):
    """The evalImgs list of the reference run: None or a dict as evaluateImg returns it."""
    z = load_golden("cocoeval")
    p = lambda name: z[f"{iou_type}_ev_{name}"]
    out = [None] * int(p("len"))
    o = dict.fromkeys(("td", "tg", "d", "g"), 0)
    for pos, (img, cat, a, D, G) in zip(p("pos").tolist(), p("meta").tolist()):
        out[pos] = {
            "image_id": img, "category_id": cat, "aRng": AREA_RNG[a], "maxDet": 100, "a": a,
            "dtMatches": p("dtm")[o["td"]:o["td"] + T * D].reshape(T, D), "dtIgnore": p("dtig")[o["td"]:o["td"] + T * D].reshape(T, D).astype(bool),
            "gtMatches": p("gtm")[o["tg"]:o["tg"] + T * G].reshape(T, G), "gtIgnore": p("gtig")[o["g"]:o["g"] + G].astype(np.int64),
            "dtIds": p("dtids")[o["d"]:o["d"] + D].tolist(), "gtIds": p("gtids")[o["g"]:o["g"] + G].tolist(),
            "dtScores": p("dtscores")[o["d"]:o["d"] + D].tolist()}
        o["td"] += T * D; o["tg"] += T * G; o["d"] += D; o["g"] += G
    assert o["td"] == p("dtm").size and o["tg"] == p("gtm").size and o["d"] == p("dtids").size and o["g"] == p("gtids").size
    return out


def same_eval_img(got, want):
    """Exact equality of two evalImgs entries (None or dict), array by array."""
    if got is None or want is None:
        return got is None and want is None
    return (got["image_id"] == want["image_id"] and got["category_id"] == want["category_id"]
            and list(got["aRng"]) == list(want["aRng"]) and got["maxDet"] == want["maxDet"]
            and list(got["dtIds"]) == list(want["dtIds"]) and list(got["gtIds"]) == list(want["gtIds"])
            and list(got["dtScores"]) == list(want["dtScores"])
            and all(np.asarray(got[k]).shape == np.asarray(want[k]).shape
                    and np.array_equal(np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64))
                    for k in ("dtMatches", "gtMatches", "dtIgnore", "gtIgnore")))


def to_eval_img(key, rng, d, g, dt_match, gt_match, dt_ignore, gt_ignore):
    """An evalImgs entry from the position form (what evaluate_img_ref returns and ops.coco_match computes): ids for positions,
    ground truths listed regular first (the stable argsort of the ignore flags)."""
    gtind = np.argsort(np.asarray(gt_ignore, dtype=np.int64), kind="mergesort")
    gt_ids, dt_ids = np.array([x["id"] for x in g] + [0]), np.array([x["id"] for x in d] + [0])
    return {"image_id": key[0], "category_id": key[1], "aRng": rng, "maxDet": 100,
            "dtIds": [x["id"] for x in d], "gtIds": [g[i]["id"] for i in gtind], "dtScores": [x["score"] for x in d],
            "dtMatches": np.where(dt_match > 0, gt_ids[dt_match - 1], 0),
            "gtMatches": np.where(gt_match > 0, dt_ids[gt_match - 1], 0)[:, gtind],
            "dtIgnore": np.asarray(dt_ignore), "gtIgnore": np.asarray(gt_ignore)[gtind]}


def seg_counts(seg):
    from maskrcnn_amd import image
    return image.rle_counts(seg)


# ------------------------------------------------------------------------------------------------ tests
def test_golden_fixture_covers_the_cases():
    gt, results = golden_inputs()
    groups = golden_groups()
    sizes = {(i["height"], i["width"]) for i in gt["images"]}
    assert len(gt["images"]) >= 12 and len(sizes) == 3 and max(sizes) == (240, 320)
    cats = [c["id"] for c in gt["categories"]]
    assert len(cats) == 4 and any(all(a["category_id"] != c for a in gt["annotations"]) for c in cats)
    areas = np.array([a["area"] for a in gt["annotations"]])
    assert (areas < 32 ** 2).any() and ((areas > 32 ** 2) & (areas < 96 ** 2)).any() and (areas > 96 ** 2).any()
    assert any(a["iscrowd"] for a in gt["annotations"])
    assert any(isinstance(a["segmentation"]["counts"], list) for a in gt["annotations"])
    assert any(isinstance(a["segmentation"]["counts"], str) for a in gt["annotations"])
    per_group = {}
    for r in results:
        per_group[r["image_id"], r["category_id"]] = per_group.get((r["image_id"], r["category_id"]), 0) + 1
    assert max(per_group.values()) > 100                                         # the maxDet cut
    scores = [r["score"] for r in results]
    assert len(set(scores)) < len(scores)                                        # tied scores
    with_dt, with_gt = {r["image_id"] for r in results}, {a["image_id"] for a in gt["annotations"]}
    ids = {i["id"] for i in gt["images"]}
    assert ids - with_dt - with_gt and (with_gt - with_dt) and (with_dt - with_gt)
    for t in ("segm", "bbox"):
        vals = np.concatenate([v.reshape(-1) for v in golden_ious(t).values()])
        assert (vals == 0.5).any() and (vals == 0.75).any() and (vals == 0).any(), t
    firsts = [seg_counts(a["segmentation"]) for a in gt["annotations"]] + [seg_counts(r["segmentation"]) for r in results]
    assert any(c[0] == 0 and c.size > 2 for c in firsts)                          # first pixel on
    assert any(c.size == 1 for c in firsts) and any(c.size == 2 and c[0] == 0 for c in firsts)   # an empty and a full mask
    assert len(groups) >= 30


def test_header_declares_and_library_exports_the_cocoeval_entry_points():
    from maskrcnn_amd import _lib
    declared, protos = _lib.declared_symbols(), _lib.header_prototypes()
    want = {"mrcnn_rle_iou_workspace_bytes": 4, "mrcnn_rle_iou_f64": 18, "mrcnn_bbox_iou_f64": 12, "mrcnn_coco_match": 20}
    for name, nargs in want.items():
        assert name in declared and name in protos, name
        assert hasattr(_lib.lib, name), name
        assert len(protos[name][1]) == nargs, name
    assert _lib.header_abi_version() >= 19 and _lib.lib.mrcnn_abi_version() == _lib.header_abi_version()
    ws = _lib.lib.mrcnn_rle_iou_workspace_bytes       # sizing needs no GPU
    assert ws(0, 8, 0, 8) == 0 and ws(-1, 8, 2, 8) == 0
    assert ws(100, 7682, 30, 5000) >= 2 * 4 * (100 * 7682 + 30 * 5000)


def test_cocoeval_source_is_built_without_fp_contraction():
    import importlib.util, os
    from maskrcnn_amd import _lib
    spec = importlib.util.spec_from_file_location("_mrcnn_build_for_test", os.path.join(_lib.PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "-ffp-contract=off" in b.SOURCES["cocoeval.hip"]
    assert os.path.exists(os.path.join(b.CSRC, "cocoeval.hip"))


def test_public_interface():
    from maskrcnn_amd import cocoeval, image, ops
    for name in ("rle_iou", "bbox_iou", "coco_match"):
        assert name in ops.__all__ and callable(getattr(ops, name)), name
    assert hasattr(torch.ops.maskrcnn, "rle_iou") and hasattr(torch.ops.maskrcnn, "bbox_iou")
    assert callable(image.rle_table) and callable(image.RleMasks.iou)
    assert list(inspect.signature(image.RleMasks.iou).parameters) == ["self", "other", "iscrowd"]
    sig = inspect.signature(cocoeval.evaluate).parameters
    assert list(sig) == ["gt", "results", "iou_type", "device"] and sig["iou_type"].default == "segm"
    p = cocoeval.Params("bbox")
    assert np.array_equal(p.iouThrs, np.linspace(.5, .95, 10)) and np.array_equal(p.recThrs, np.linspace(0, 1, 101))
    assert p.maxDets == [1, 10, 100] and p.useCats == 1 and p.areaRng == AREA_RNG
    with pytest.raises(ValueError):
        cocoeval.Params("keypoints")


def test_iou_and_match_refuse_cpu_tensors():
    from maskrcnn_amd import ops
    nr, cnt = torch.tensor([3], dtype=torch.int32), torch.tensor([[2, 3, 4]], dtype=torch.int32)
    boxes = torch.zeros(2, 4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.rle_iou((nr, cnt), (nr, cnt))
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        torch.ops.maskrcnn.rle_iou(nr, cnt, nr, cnt)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.bbox_iou(boxes, boxes)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        torch.ops.maskrcnn.bbox_iou(boxes, boxes)
    off = torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.coco_match(torch.zeros(1, dtype=torch.float64), off, off, off.long(), torch.ones(1, dtype=torch.float64),
                       torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.uint8),
                       torch.tensor(AREA_RNG, dtype=torch.float64), torch.from_numpy(IOU_THRS))


def test_rle_table_validates_its_input():
    from maskrcnn_amd import image
    with pytest.raises(ValueError, match="cover 13 pixels"):
        image.rle_table([[4, 4, 4], [5, 4, 4]], (3, 4), device="cpu")            # one pixel too many
    with pytest.raises(ValueError, match="empty run"):
        image.rle_table([[3, 0, 4, 5]], (3, 4), device="cpu")                    # a zero-length run inside
    with pytest.raises(ValueError, match="empty run"):
        image.rle_table([[3, 9, 0]], (3, 4), device="cpu")                       # ... or at the end
    with pytest.raises(ValueError, match="is \\[4, 3\\]"):
        image.rle_table([{"size": [4, 3], "counts": [12]}], (3, 4), device="cpu")
    with pytest.raises(ValueError, match="capacity"):
        image.rle_table([[1, 2, 3, 6]], (3, 4), device="cpu", capacity=3)
    # a leading empty run is a mask whose first pixel is on: accepted; strings, dicts and lists mix
    gt, _ = golden_inputs()
    ann = next(a for a in gt["annotations"] if isinstance(a["segmentation"]["counts"], str))
    h, w = ann["segmentation"]["size"]
    num_runs, counts = image.rle_table([[0, h * w], ann["segmentation"], ann["segmentation"]["counts"], [h * w]], (h, w), device="cpu")
    want = image.rle_counts(ann["segmentation"])
    assert num_runs.tolist() == [2, want.size, want.size, 1] and counts.dtype == torch.int32 and counts.shape == (4, max(2, want.size))
    assert np.array_equal(counts[1, :want.size].numpy().view(np.uint32), want) and counts[0].tolist()[:2] == [0, h * w]
    assert not counts[3, 1:].any()


def test_polygon_ground_truth_is_refused_for_segm_only():
    from maskrcnn_amd import cocoeval
    gt, results = golden_inputs()
    gt["annotations"][3]["segmentation"] = [[10.0, 10.0, 40.0, 10.0, 40.0, 30.0]]
    with pytest.raises(NotImplementedError, match="polygon"):
        cocoeval.evaluate(gt, results, "segm", device="cpu")
    with pytest.raises(NotImplementedError, match="polygon"):
        cocoeval.load_results([{"image_id": 2, "category_id": 1, "score": 0.5, "segmentation": [[1.0, 1.0, 5.0, 1.0, 5.0, 5.0]]}], "segm")
    with pytest.raises(ValueError, match="Results do not correspond"):
        cocoeval.evaluate(gt, [dict(results[0], image_id=987654)], "bbox", device="cpu")


def test_rle_area_and_bbox_restatement_equals_the_reference_codec():
    from maskrcnn_amd import cocoeval
    z = load_golden("rle")
    for k, name in enumerate(z["names"].tolist()):
        h, w = (int(v) for v in z["shapes"][k])
        area, bbox = cocoeval._rle_area_bbox(z["counts"][z["cnt_off"][k]:z["cnt_off"][k + 1]], h, w)
        assert area == int(z["areas"][k]) and bbox == [float(v) for v in z["bboxes"][k]], name


@pytest.mark.parametrize("iou_type", ["segm", "bbox"])
def test_accumulate_and_summary_from_the_golden_eval_imgs(iou_type):
    """The host half alone: the reference's evalImgs in, its precision / recall / scores / stats / printed lines out."""
    from maskrcnn_amd import cocoeval
    z = load_golden("cocoeval")
    gt, _ = golden_inputs()
    p = cocoeval.Params(iou_type)
    p.imgIds = sorted(i["id"] for i in gt["images"])
    p.catIds = sorted(c["id"] for c in gt["categories"])
    precision, recall, scores = cocoeval.accumulate(golden_eval_imgs(iou_type), p)
    for got, name in ((precision, "precision"), (recall, "recall"), (scores, "scores")):
        want = z[f"{iou_type}_{name}"]
        assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want), name
    assert precision.shape == (10, 101, 4, 4, 3) and (precision > 0).any() and (precision == -1).any()
    stats, lines = cocoeval.summarize(precision, recall, p)
    assert stats.shape == (12,) and np.array_equal(stats, z[f"{iou_type}_stats"])
    assert lines == z[f"{iou_type}_summary"].tolist() and len(lines) == 12
    assert lines[0].startswith(" Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = ")


def test_iou_restatements_equal_the_golden_on_every_group():
    groups = golden_groups()
    for iou_type in ("segm", "bbox"):
        want = golden_ious(iou_type)
        seen = 0
        for key, (d, g) in groups.items():
            if not d or not g:
                assert key not in want
                continue
            crowd = [a["iscrowd"] for a in g]
            if iou_type == "segm":
                got = rle_iou_ref([seg_counts(x["segmentation"]) for x in d], [seg_counts(x["segmentation"]) for x in g], crowd)
            else:
                got = bbox_iou_ref([x["bbox"] for x in d], [x["bbox"] for x in g], crowd)
            assert got.shape == want[key].shape and np.array_equal(got, want[key]), (iou_type, key)
            seen += 1
        assert seen == len(want) >= 15


@pytest.mark.parametrize("iou_type", ["segm", "bbox"])
def test_evaluate_img_restatement_equals_the_golden_on_every_entry(iou_type):
    groups, ious = golden_groups(), golden_ious(iou_type)
    entries = [e for e in golden_eval_imgs(iou_type) if e is not None]
    assert len(entries) >= 100
    matched = 0
    for e in entries:
        key = (e["image_id"], e["category_id"])
        d, g = groups[key]
        dtm, gtm, dtig, gtig, gtind = evaluate_img_ref(ious.get(key, []), [x["area"] for x in d], [x["area"] for x in g],
                                                       [x["iscrowd"] for x in g], e["aRng"], IOU_THRS)
        got = to_eval_img(key, e["aRng"], d, g, dtm, gtm, dtig, gtig)
        assert same_eval_img(got, e), (key, e["a"])
        matched += int((dtm > 0).sum())
    assert matched > 500


@pytest.mark.parametrize("iou_type", ["segm", "bbox"])
def test_grouping_and_rebuilding_stages_equal_the_golden_without_a_gpu(iou_type):
    """cocoeval._group and cocoeval._rebuild, the host stages either side of evaluate's device calls: the flat order and the
    offsets of the first against golden_groups, and the second — fed the golden IoUs and what evaluate_img_ref computes, laid
    out as ops.rle_iou / ops.coco_match return them — against the golden ious and evalImgs."""
    from maskrcnn_amd import cocoeval
    gt, results = golden_inputs()
    p = cocoeval.Params(iou_type)
    p.imgIds, p.catIds = list(np.unique([i["id"] for i in gt["images"]])), list(np.unique([c["id"] for c in gt["categories"]]))
    g = cocoeval._group(gt["annotations"], cocoeval.load_results(results, iou_type), p)
    groups, want_ious = golden_groups(), golden_ious(iou_type)
    assert g.keys == sorted(groups) and len(g.keys) >= 30
    for k, key in enumerate(g.keys):
        d, gg = groups[key]
        assert [x["id"] for x in g.dts[key]] == [x["id"] for x in d] and [x["id"] for x in g.gts[key]] == [x["id"] for x in gg], key
        assert g.dt_flat[g.dt_off[k]:g.dt_off[k + 1]] == g.dts[key] and g.gt_flat[g.gt_off[k]:g.gt_off[k + 1]] == g.gts[key], key
        assert (g.dt_n[k], g.gt_n[k], g.out_off[k + 1] - g.out_off[k]) == (len(d), len(gg), len(d) * len(gg)), key
    assert len(g.dt_flat) == g.dt_off[-1] and len(g.gt_flat) == g.gt_off[-1] and g.dt_n.max() == 100
    assert g.dt_off.dtype == g.gt_off.dtype == g.out_off.dtype == np.int64 and g.dt_off[0] == g.gt_off[0] == g.out_off[0] == 0
    with pytest.raises(NotImplementedError, match="annotation 7: polygon"):
        cocoeval._group([dict(gt["annotations"][0], id=7, segmentation=[[1.0, 1.0, 5.0, 1.0, 5.0, 5.0]])], [], p, refuse_polygons=True)

    A, N, M = len(AREA_RNG), int(g.dt_off[-1]), int(g.gt_off[-1])
    ious_flat = np.full(int(g.out_off[-1]), np.nan)
    dt_match, gt_match = np.zeros((A, T, N), np.int32), np.zeros((A, T, M), np.int32)
    dt_ignore, gt_ignore = np.zeros((A, T, N), np.uint8), np.zeros((A, M), np.uint8)
    for k, key in enumerate(g.keys):
        d, gg = groups[key]
        if key in want_ious:
            ious_flat[g.out_off[k]:g.out_off[k + 1]] = want_ious[key].T.reshape(-1)          # ground truth slowest
        ds, gs = slice(g.dt_off[k], g.dt_off[k + 1]), slice(g.gt_off[k], g.gt_off[k + 1])
        for a, rng in enumerate(AREA_RNG):
            dt_match[a, :, ds], gt_match[a, :, gs], dt_ignore[a, :, ds], gt_ignore[a, gs], _ = evaluate_img_ref(
                want_ious.get(key, []), [x["area"] for x in d], [x["area"] for x in gg], [x["iscrowd"] for x in gg], rng, IOU_THRS)
    assert not np.isnan(ious_flat).any()
    ious, eval_imgs = cocoeval._rebuild(g, p, ious_flat, dt_match, gt_match, dt_ignore, gt_ignore)
    assert set(ious) == {(i, c) for i in p.imgIds for c in p.catIds}
    for key, v in ious.items():
        assert np.array_equal(v, want_ious[key]) if key in want_ious else (isinstance(v, list) and v == []), key
    want = golden_eval_imgs(iou_type)
    assert len(eval_imgs) == len(want) == len(p.catIds) * A * len(p.imgIds)
    assert all(same_eval_img(x, y) for x, y in zip(eval_imgs, want)) and sum(e is not None for e in eval_imgs) >= 100
    ev = cocoeval.CocoEval(p, ious, eval_imgs)                                                # and the rest of evaluate on them
    assert np.array_equal(ev.stats, load_golden("cocoeval")[f"{iou_type}_stats"])


def test_one_hip_runtime_whatever_is_imported_first():
    """`python -m maskrcnn_amd.cocoeval` imports the package before torch: the library must still share torch's HIP runtime (two
    copies of libamdhip64 in one process: the second one's launches fail with "no ROCm-capable device is detected")."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import maskrcnn_amd.cocoeval, torch\n"
            "print(sorted({l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l}))")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    paths = eval(r.stdout.strip().splitlines()[-1])
    assert len(paths) == 1, paths
