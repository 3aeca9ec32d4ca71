"""COCO polygons to run lengths, the host side: the parity formulation of rleFrPoly and the n-way event formulation of rleMerge
— what csrc/poly.hip's kernels rely on — restated in numpy and pinned to tests/golden/poly.npz (the reference's own maskApi.c,
tests/golden/make_golden_poly.py), the host key bound, the packing and the refusals of image.rle_from_polygons and
cocoeval.ann_to_rle, and the C ABI. No GPU."""
import ctypes
import inspect
import json
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import load_golden


# ------------------------------------------------------------------------------------------------ the fixture
class Golden:
    def __init__(self):
        z = load_golden("poly")
        self.z = z
        self.names = z["case_names"].tolist()
        off, coff = z["case_off"], z["case_cnt_off"]
        self.xy = [z["case_xy"][off[i]:off[i + 1]] for i in range(len(self.names))]
        self.h, self.w = z["case_h"].astype(int).tolist(), z["case_w"].astype(int).tolist()
        self.counts = [z["case_cnt"][coff[i]:coff[i + 1]] for i in range(len(self.names))]
        self.fma = z["case_fma"].tolist()
        goff = z["group_off"]
        self.group_names = z["group_names"].tolist()
        self.members = [z["group_members"][goff[g]:goff[g + 1]].tolist() for g in range(len(self.group_names))]
        cut = lambda name: [z[name][z[name + "_off"][g]:z[name + "_off"][g + 1]] for g in range(len(self.group_names))]
        self.union, self.inter = cut("group_union"), cut("group_inter")

    def index(self, name):
        return self.names.index(name)


_GOLDEN = []


def golden() -> Golden:
    if not _GOLDEN:
        _GOLDEN.append(Golden())
    return _GOLDEN[0]


# ------------------------------------------------------------------------------------------------ the restatements
def _fma(a, b, c) -> float:
    """a*b + c in exact rational arithmetic, rounded once: a fused multiply-add."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _grid(c, fma):
    t = 5.0 * c + .5
    if fma:   # only a value next to an integer can be cast to another one
        for i in np.nonzero(np.abs(t - np.rint(t)) < 1e-6 * np.maximum(1.0, np.abs(t)))[0]:
            t[i] = _fma(5.0, c[i], .5)
    return np.trunc(t).astype(np.int64)


def _minor(a0, s, t, fma):
    r = float(a0) + s * t.astype(np.float64)
    if fma:
        for i in np.nonzero(np.abs((r + .5) - np.rint(r + .5)) < 1e-6 * np.maximum(1.0, np.abs(r)))[0]:
            r[i] = _fma(s, float(t[i]), float(a0))
    return np.trunc(r + .5).astype(np.int64)


def poly_keys_ref(xy, h, w, fma=False, nan_as=-2 ** 31):
    """Steps 1-3 of rleFrPoly (maskApi.c:162-191): the kept column crossings' keys x*h + y, in boundary order. nan_as: what the
    point of a zero-length edge gets as its minor coordinate ((int)NaN in the reference)."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    X, Y = _grid(xy[:, 0].copy(), fma), _grid(xy[:, 1].copy(), fma)
    k, us, vs = len(X), [], []
    for j in range(k):
        xs, xe, ys, ye = int(X[j]), int(X[(j + 1) % k]), int(Y[j]), int(Y[(j + 1) % k])
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        d = np.arange(max(dx, dy) + 1, dtype=np.int64)
        if dx >= dy:
            t = dx - d if flip else d
            us.append(t + xs)
            vs.append(np.full(1, nan_as, np.int64) if dx == 0 else _minor(ys, float(ye - ys) / float(dx), t, fma))
        else:
            t = dy - d if flip else d
            vs.append(t + ys)
            us.append(_minor(xs, float(xe - xs) / float(dy), t, fma))
    u, v = np.concatenate(us), np.concatenate(vs)
    j = np.nonzero(u[1:] != u[:-1])[0] + 1
    xd = (np.where(u[j] < u[j - 1], u[j], u[j] - 1).astype(np.float64) + .5) / 5.0 - .5
    keep = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    yd = np.ceil(np.clip((np.minimum(v[j], v[j - 1]).astype(np.float64) + .5) / 5.0 - .5, 0, h))
    return xd[keep].astype(np.int64) * h + yd[keep].astype(np.int64)


def fr_poly_ref(xy, h, w, fma=False, nan_as=-2 ** 31) -> np.ndarray:
    """The parity rule: the run boundaries are the distinct keys below h*w that occur an odd number of times; the runs are their
    differences from 0 up to h*w."""
    keys = poly_keys_ref(xy, h, w, fma, nan_as)
    vals, cnt = np.unique(keys[keys < h * w], return_counts=True)
    return np.diff(np.concatenate([[0], vals[cnt % 2 == 1], [h * w]])).astype(np.uint32)


def merge_ref(rows, intersect) -> np.ndarray:
    """rleMerge as ONE n-way pass: every toggle is a signed event, the events are summed per position and prefix-summed into a
    coverage count; a boundary falls where coverage > 0 (union) or coverage == n (intersection) changes."""
    n = len(rows)
    if n == 1:
        return np.asarray(rows[0], dtype=np.uint32).copy()
    total = int(np.asarray(rows[0], dtype=np.int64).sum())
    pos = [np.cumsum(np.asarray(r, dtype=np.int64))[:-1] for r in rows]
    sign = [np.where(np.arange(p.size) % 2 == 0, 1, -1) for p in pos]
    vals, inv = np.unique(np.concatenate(pos), return_inverse=True)
    cov = np.cumsum(np.bincount(inv, weights=np.concatenate(sign), minlength=vals.size)).astype(np.int64)
    on = cov == n if intersect else cov > 0
    b = vals[on != np.concatenate([[False], on[:-1]])]
    return np.diff(np.concatenate([[0], b, [total]])).astype(np.uint32)


def frbbox_polygon(bb):
    xs, ys = float(bb[0]), float(bb[1])
    xe, ye = xs + float(bb[2]), ys + float(bb[3])
    return [xs, ys, xs, ye, xe, ye, xe, ys]


def eval_inputs():
    z = golden().z
    return json.loads(str(z["gt_json"])), json.loads(str(z["results_json"]))


# ------------------------------------------------------------------------------------------------ the fixture itself
def test_golden_fixture_covers_the_cases():
    g = golden()
    for name in ("img1x1_cover", "h1", "w1", "triangle_int", "rect_half", "triangle_frac", "out_left", "out_right", "out_top",
                 "out_bottom", "over_left", "over_right", "over_top", "over_bottom", "over_corner_tl", "over_corner_br", "k1", "k2",
                 "repeat_first", "repeat_middle", "repeat_closing", "collinear", "bowtie", "star5", "spike", "slope_1_2",
                 "slope_inv_7_10", "serpentine"):
        assert name in g.names, name
    assert g.counts[g.index("pixel0_on")][0] == 0 and g.counts[g.index("whole_image")].tolist() == [0, 30 * 40]
    for name in ("out_left", "out_right", "out_top", "k1"):
        i = g.index(name)
        assert g.counts[i].tolist() == [g.h[i] * g.w[i]], name
    assert g.counts[g.index("serpentine")].size > 8192 and len(g.xy[g.index("serpentine")]) == 128
    assert sum(g.fma) >= 4 and sum(n.startswith("random_") for n in g.names) == 300
    for i, c in enumerate(g.counts):
        assert int(c.astype(np.int64).sum()) == g.h[i] * g.w[i] and (c[1:] > 0).all(), g.names[i]
    # the two key aliases: a crossing at y == h in an inner column (the key is the top of the next column) and in the last one
    for name, last in (("y_eq_h_inner_column", False), ("y_eq_h_last_column", True)):
        i = g.index(name)
        keys = poly_keys_ref(g.xy[i], g.h[i], g.w[i])
        at_h = keys[keys % g.h[i] == 0] // g.h[i]
        assert (keys == g.h[i] * g.w[i]).any() == last and ((at_h > 0) & (at_h < g.w[i])).any(), name
    assert sorted({len(m) for m in g.members}) == [1, 2, 3, 5, 12]
    assert any(u[0] == 0 for u in g.union) and any(x.size == 1 for x in g.inter)
    assert len(g.z["box_bb"]) == 12 and len(g.z["ann_ids"]) > 40


def test_parity_restatement_equals_the_reference_on_every_case():
    g = golden()
    for i, name in enumerate(g.names):
        got = fr_poly_ref(g.xy[i], g.h[i], g.w[i])
        assert got.dtype == np.uint32 and np.array_equal(got, g.counts[i]), name
    # the point of a zero-length edge never reaches the output, whatever (int)NaN is
    for name in ("repeat_first", "repeat_middle", "repeat_closing", "repeat_triple", "k1"):
        i = g.index(name)
        for nan_as in (0, 2 ** 31 - 1, 12345):
            assert np.array_equal(fr_poly_ref(g.xy[i], g.h[i], g.w[i], nan_as=nan_as), g.counts[i]), (name, nan_as)


def test_a_fused_multiply_add_differs_on_every_flagged_case():
    g = golden()
    flagged = [i for i, f in enumerate(g.fma) if f]
    assert len(flagged) >= 4
    for i in flagged:
        assert not np.array_equal(fr_poly_ref(g.xy[i], g.h[i], g.w[i], fma=True), g.counts[i]), g.names[i]


def test_nway_merge_restatement_equals_the_reference_on_every_group():
    g = golden()
    for k, name in enumerate(g.group_names):
        rows = [g.counts[m] for m in g.members[k]]
        assert np.array_equal(merge_ref(rows, False), g.union[k]), name
        assert np.array_equal(merge_ref(rows, True), g.inter[k]), name


def test_frbbox_is_the_four_vertex_polygon():
    z = golden().z
    for b in range(len(z["box_bb"])):
        want = z["box_cnt"][z["box_cnt_off"][b]:z["box_cnt_off"][b + 1]]
        assert np.array_equal(fr_poly_ref(frbbox_polygon(z["box_bb"][b]), int(z["box_h"][b]), int(z["box_w"][b])), want), b


def test_host_key_bound_is_never_below_the_key_count():
    from maskrcnn_amd import image, ops
    g = golden()
    xy, off, hs, ws = image._pack_polygons([x.reshape(-1).tolist() for x in g.xy], list(zip(g.h, g.w)))
    bounds = ops.poly_host_bounds(xy, off, hs, ws)
    assert bounds.shape == (len(g.names),)
    for i, name in enumerate(g.names):
        keys = poly_keys_ref(g.xy[i], g.h[i], g.w[i]).size
        assert bounds[i] >= keys and bounds[i] + 1 >= g.counts[i].size, (name, int(bounds[i]), keys)
    assert bounds[g.index("serpentine")] > ops.rle_from_poly_onchip_keys()


# ------------------------------------------------------------------------------------------------ packing and refusals
def test_rle_from_polygons_packing():
    from maskrcnn_amd import image
    polys = [[1, 2, 3, 4, 5, 6], [7.5, 8.5, 9, 10, 11], [0, 0]]        # the second has an odd trailing number: len // 2
    xy, off, hs, ws = image._pack_polygons(polys, (20, 30))
    assert off.tolist() == [0, 3, 5, 6] and hs.tolist() == [20] * 3 and ws.tolist() == [30] * 3
    assert xy.dtype == np.float64 and xy.tolist() == [[1, 2], [3, 4], [5, 6], [7.5, 8.5], [9, 10], [0, 0]]
    _, _, hs, ws = image._pack_polygons(polys, [(20, 30), (1, 2), (16384, 7)])
    assert hs.tolist() == [20, 1, 16384] and ws.tolist() == [30, 2, 7]
    dev_xy, dev_off, dev_h, dev_w = image._polygons_to_device(xy, off, hs, ws, "cpu")   # one buffer; the integers are exact
    assert dev_xy.dtype == torch.float64 and dev_xy.shape == (6, 2) and np.array_equal(dev_xy.numpy(), xy)
    assert dev_off.dtype == torch.int32 and dev_off.tolist() == [0, 3, 5, 6]
    assert dev_h.tolist() == [20, 1, 16384] and dev_w.tolist() == [30, 2, 7] and dev_w.dtype == torch.int32
    with pytest.raises(ValueError, match="one per polygon"):
        image._pack_polygons(polys, [(20, 30), (1, 2)])


def test_rle_from_polygons_refusals_happen_on_the_host():
    from maskrcnn_amd import image
    tri = [1, 1, 9, 1, 5, 8]
    for bad, match in (([1, 1, float("nan"), 1, 5, 8], "not finite"), ([1, 1, float("inf"), 1, 5, 8], "not finite"),
                       ([1, 1, 2.0 ** 31 / 5, 1, 5, 8], r"below 2\^31"), ([1, 1, 9, -2.0 ** 31 / 5 - 1, 5, 8], r"below 2\^31"),
                       ([], "not one vertex"), ([3], "not one vertex")):
        with pytest.raises(ValueError, match=match):
            image.rle_from_polygons([tri, bad], (20, 30), device="cpu")
    for size in ((0, 30), (20, 0), (16385, 30), (20, 16385)):
        with pytest.raises(ValueError, match="outside"):
            image.rle_from_polygons([tri], size, device="cpu")
    with pytest.raises(ValueError, match="boundary points"):            # 2^24 points fit, one more does not
        image.rle_from_polygons([[0, 0, (2 ** 23) / 5.0, 0]], (20, 30), device="cpu")
    with pytest.raises(ValueError, match="not finite"):
        image.rle_from_bboxes([[1, 1, float("nan"), 4]], (20, 30), device="cpu")


def test_largest_accepted_values_pass_the_host_checks():
    from maskrcnn_amd import image, ops
    edge = (2 ** 23 - 1) / 5.0                                          # two edges of 2^23 points each: exactly 2^24
    xy, off, hs, ws = image._pack_polygons([[0, 0, edge, 0], [-(2.0 ** 31 - 2) / 5, 0, -(2.0 ** 31 - 2) / 5, 1]], (16384, 16384))
    b = ops.poly_host_bounds(xy, off, hs, ws, error=ValueError)
    assert b.tolist() == [2 * ((2 ** 23 - 1) // 5 + 1), 2]


def test_ann_to_rle_refusals_name_the_annotation():
    from maskrcnn_amd import cocoeval
    gt, _ = eval_inputs()
    poly = [a for a in gt["annotations"] if isinstance(a["segmentation"], list)]
    for seg, match in (([[1, 2, 3, 4], [1, 1, 9, 1, 5, 8]], "4 numbers"), ([[1, 2]], "2 numbers"), ([[]], "0 numbers"),
                       ([], "list of"), ([[1, 1, 9, 1, 5, 8], [4]], "no vertex"), ([[1, 1, 9, 1, float("nan"), 8]], "not finite")):
        bad = json.loads(json.dumps(gt))
        bad["annotations"][gt["annotations"].index(poly[3])]["segmentation"] = seg
        with pytest.raises(ValueError, match=f"annotation {poly[3]['id']}: .*{match}"):
            cocoeval.ann_to_rle(bad, device="cpu")
    rle_only = dict(gt, annotations=[a for a in gt["annotations"] if not isinstance(a["segmentation"], list)])
    out = cocoeval.ann_to_rle(rle_only, device="cpu")                   # nothing to rasterise: no GPU needed, a copy
    assert out["annotations"] == rle_only["annotations"] and out["annotations"][0] is not rle_only["annotations"][0]


def test_polygons_are_still_refused_by_default_and_the_keyword_is_checked():
    from maskrcnn_amd import cocoeval
    gt, results = eval_inputs()
    with pytest.raises(NotImplementedError, match="polygon"):
        cocoeval.evaluate(gt, results, "segm", device="cpu")
    with pytest.raises(NotImplementedError, match="polygon"):
        cocoeval.evaluate(gt, results, "segm", device="cpu", polygons="error")
    with pytest.raises(ValueError, match="polygons="):
        cocoeval.evaluate(gt, results, "segm", device="cpu", polygons="dense")
    with pytest.raises(NotImplementedError, match="polygon"):           # result records: refused in either mode
        cocoeval.load_results([{"image_id": 2, "category_id": 1, "score": 0.5, "segmentation": [[1.0, 1.0, 5.0, 1.0, 5.0, 5.0]]}], "segm")
    assert list(inspect.signature(cocoeval.evaluate).parameters)[:4] == ["gt", "results", "iou_type", "device"]
    assert cocoeval.evaluate.__kwdefaults__ == {"polygons": "error"}    # keyword-only, beside the pinned positional interface
    with pytest.raises(TypeError):
        cocoeval.evaluate(gt, results, "segm", "cpu", "rasterize")
    ap = inspect.getsource(cocoeval.main)
    assert "--polygons" in ap and "rasterize" in ap


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_and_library_exports_the_polygon_entry_points():
    from maskrcnn_amd import _lib
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_size_t
    want = {
        "mrcnn_rle_from_poly_onchip_keys": (i32, []),
        "mrcnn_rle_from_poly_workspace_bytes": (sz, [i32, i32]),
        "mrcnn_rle_from_poly_f64": (ctypes.c_int, [vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, sz, vp]),
        "mrcnn_rle_merge_workspace_bytes": (sz, [i32, i32]),
        "mrcnn_rle_merge": (ctypes.c_int, [vp, vp, i32, i32, vp, i32, i32, i32, vp, vp, vp, sz, vp]),
    }
    declared, protos = _lib.declared_symbols(), _lib.header_prototypes()
    for name, sig in want.items():
        assert name in declared and hasattr(_lib.lib, name), name
        assert protos[name] == sig, (name, protos[name])
    assert _lib.header_abi_version() >= 20 and _lib.lib.mrcnn_abi_version() == _lib.header_abi_version()
    lib = _lib.lib                                                      # sizing and the query need no GPU
    assert lib.mrcnn_rle_from_poly_onchip_keys() >= 1024
    assert lib.mrcnn_rle_from_poly_workspace_bytes(0, 0) == 0 and lib.mrcnn_rle_from_poly_workspace_bytes(3, 10) >= 4 * 13
    assert lib.mrcnn_rle_from_poly_workspace_bytes(2 ** 22 + 1, 10) == 0 and lib.mrcnn_rle_from_poly_workspace_bytes(1, 2 ** 28 + 1) == 0
    assert lib.mrcnn_rle_merge_workspace_bytes(0, 8) == 0 and lib.mrcnn_rle_merge_workspace_bytes(10, 100) >= 2 * 4 * 1000
    # host-side limits are refused before anything is launched
    for args in ((None, 0, None, None, None, -1, 8), (None, 0, None, None, None, 2 ** 22 + 1, 8), (None, 2 ** 28 + 1, None, None, None, 1, 8),
                 (None, 3, None, None, None, 1, 0)):
        assert lib.mrcnn_rle_from_poly_f64(*args, None, None, None, None, 0, None) == -1, args
        assert b"rle_from_poly" in lib.mrcnn_last_error()
    assert lib.mrcnn_rle_from_poly_f64(None, 0, None, None, None, 0, 8, None, None, None, None, 0, None) == 0   # n == 0
    assert lib.mrcnn_rle_merge(None, None, 0, 8, None, 0, 0, 8, None, None, None, 0, None) == 0                 # no groups
    assert lib.mrcnn_rle_merge(None, None, 0, 8, None, 1, 2, 8, None, None, None, 0, None) == -1                # intersect = 2


def test_poly_source_is_built_without_fp_contraction():
    import importlib.util, os
    from maskrcnn_amd import _lib
    spec = importlib.util.spec_from_file_location("_mrcnn_build_for_poly_test", os.path.join(_lib.PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "-ffp-contract=off" in b.SOURCES["poly.hip"] and os.path.exists(os.path.join(b.CSRC, "poly.hip"))


def test_public_interface_and_cpu_tensors_are_refused():
    from maskrcnn_amd import cocoeval, image, ops
    for name in ("rle_from_poly", "rle_merge"):
        assert name in ops.__all__ and callable(getattr(ops, name)) and hasattr(torch.ops.maskrcnn, name), name
    assert list(inspect.signature(ops.rle_from_poly).parameters) == ["xy", "vert_off", "heights", "widths", "capacity"]
    assert list(inspect.signature(ops.rle_merge).parameters) == ["num_runs", "counts", "group_off", "intersect", "capacity"]
    assert list(inspect.signature(image.rle_from_polygons).parameters) == ["polys", "sizes", "device"]
    assert list(inspect.signature(image.rle_from_bboxes).parameters) == ["boxes", "size", "device"]
    assert "ann_to_rle" in cocoeval.__all__
    xy, off = torch.zeros(3, 2, dtype=torch.float64), torch.tensor([0, 3], dtype=torch.int32)
    hw = torch.tensor([8], dtype=torch.int32)
    nr, cnt = torch.tensor([1], dtype=torch.int32), torch.tensor([[64]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.rle_from_poly(xy, off, hw, hw)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        torch.ops.maskrcnn.rle_from_poly(xy, off, hw, hw)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.rle_merge(nr, cnt, torch.tensor([0, 1], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        torch.ops.maskrcnn.rle_merge(nr, cnt, torch.tensor([0, 1], dtype=torch.int32))
