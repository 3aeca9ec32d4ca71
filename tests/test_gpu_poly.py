"""COCO polygons to run lengths on the GPU: ops.rle_from_poly / ops.rle_merge (csrc/poly.hip), image.rle_from_polygons /
rle_from_bboxes, cocoeval.ann_to_rle and evaluate(polygons="rasterize") against tests/golden/poly.npz — the reference's own
rleFrPoly, rleFrBbox, rleMerge and cocoeval.py (tests/golden/make_golden_poly.py). Integer work and separately rounded fp64: every
comparison is exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_poly_host import eval_inputs, golden, poly_keys_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ_LIB = os.path.join(ROOT, "maskrcnn_amd", "csrc", "build", "variants", "sync_fuzz", "libmaskrcnn_hip.so")
DEV = torch.device("cuda:0")
POISON = 0x5A5A5A5A


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


def poly_args(xys, hs, ws):
    """Device arguments of ops.rle_from_poly for a list of [k,2] vertex arrays."""
    off = np.concatenate([[0], np.cumsum([len(x) for x in xys])])
    xy = np.concatenate(xys) if len(xys) else np.zeros((0, 2))
    return dev(xy, np.float64), dev(off, np.int32), dev(hs, np.int32), dev(ws, np.int32)


def host_rows(num_runs, counts):
    nr, c = num_runs.cpu().numpy(), counts.cpu().numpy().view(np.uint32)
    return nr, [c[i, :max(int(nr[i]), 0)] for i in range(len(nr))]


def same_rows(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


class Fixture:
    """Every golden case through ONE ops.rle_from_poly call, made once and shared."""

    def __init__(self):
        from maskrcnn_amd import ops
        self.g = g = golden()
        self.args = poly_args(g.xy, g.h, g.w)
        self.num_runs, self.counts, self.num_keys = ops.rle_from_poly(*self.args)
        self.nr, self.rows = host_rows(self.num_runs, self.counts)
        self.keys = self.num_keys.cpu().numpy()


@pytest.fixture(scope="module")
def fx():
    return Fixture()


# ------------------------------------------------------------------------------------------------ rle_from_poly
def test_from_poly_equals_the_golden_for_all_cases_in_one_call(fx):
    from maskrcnn_amd import ops
    g = fx.g
    assert fx.num_runs.dtype == torch.int32 and fx.counts.dtype == torch.int32 and fx.num_keys.dtype == torch.int32
    assert fx.counts.shape[0] == len(g.names) and fx.counts.shape[1] >= max(c.size for c in g.counts)
    for i, name in enumerate(g.names):
        assert fx.nr[i] == g.counts[i].size and np.array_equal(fx.rows[i], g.counts[i]), name
    # num_keys is the number of crossings step 3 keeps, and it tells which path ran
    onchip = ops.rle_from_poly_onchip_keys()
    for i in list(range(60)) + [g.index("random_7"), g.index("random_299")]:
        assert fx.keys[i] == poly_keys_ref(g.xy[i], g.h[i], g.w[i]).size, g.names[i]
    assert fx.keys[g.index("serpentine")] > onchip                         # sorted range by range
    twenty = next(i for i, x in enumerate(g.xy) if len(x) == 20 and g.names[i].startswith("random_") and fx.keys[i] > 0)
    assert 0 < fx.keys[twenty] <= onchip                                   # sorted on chip in one piece
    assert sum(k > onchip for k in fx.keys) == 1


def test_from_poly_equals_the_golden_for_each_case_alone(fx):
    from maskrcnn_amd import ops
    g = fx.g
    outs = [ops.rle_from_poly(*poly_args([g.xy[i]], [g.h[i]], [g.w[i]])) for i in range(len(g.names))]
    for i, (nr, cnt, nk) in enumerate(outs):
        nr_h, rows = host_rows(nr, cnt)
        assert nr_h[0] == g.counts[i].size and np.array_equal(rows[0], g.counts[i]) and int(nk[0]) == fx.keys[i], g.names[i]


def test_torch_op_and_explicit_capacity_give_the_same_table(fx):
    g = fx.g
    sel = [i for i, n in enumerate(g.names) if n != "serpentine"][:80]
    cap = max(g.counts[i].size for i in sel)
    nr, cnt, nk = torch.ops.maskrcnn.rle_from_poly(*poly_args([g.xy[i] for i in sel], [g.h[i] for i in sel], [g.w[i] for i in sel]), cap)
    assert cnt.shape == (len(sel), cap)
    nr_h, rows = host_rows(nr, cnt)
    assert same_rows(rows, [g.counts[i] for i in sel]) and np.array_equal(nk.cpu().numpy(), fx.keys[sel])


def test_from_polygons_and_from_bboxes_equal_the_reference(fx):
    from maskrcnn_amd import image
    g, z = fx.g, fx.g.z
    sel = [i for i, n in enumerate(g.names) if n != "serpentine"]
    polys = [g.xy[i].reshape(-1).tolist() + ([99.0] if i % 3 == 0 else []) for i in sel]      # an odd trailing number is dropped
    nr, rows = host_rows(*image.rle_from_polygons(polys, [(g.h[i], g.w[i]) for i in sel]))
    assert same_rows(rows, [g.counts[i] for i in sel])
    want = [z["box_cnt"][z["box_cnt_off"][b]:z["box_cnt_off"][b + 1]] for b in range(len(z["box_bb"]))]
    for b in range(len(want)):                                                               # sizes differ: box by box
        nr, rows = host_rows(*image.rle_from_bboxes(z["box_bb"][b:b + 1], (int(z["box_h"][b]), int(z["box_w"][b]))))
        assert np.array_equal(rows[0], want[b]), b
    same = [b for b in range(len(want)) if (int(z["box_h"][b]), int(z["box_w"][b])) == (30, 40)]
    nr, rows = host_rows(*image.rle_from_bboxes(z["box_bb"][same], (30, 40)))
    assert len(same) >= 8 and same_rows(rows, [want[b] for b in same])


def test_the_dense_path_agrees(fx):
    """The reference's mask of 50 random cases, decoded on the host and encoded again by ops.rle_encode — the other way to a
    run-length table on this GPU — equals the polygon kernel's rows."""
    from maskrcnn_amd import image, ops
    g = fx.g
    rng = np.random.default_rng(3)
    for i in rng.choice([i for i, n in enumerate(g.names) if n.startswith("random_")], 50, replace=False):
        mask = image.rle_decode(g.counts[i], (g.h[i], g.w[i]))
        enc = ops.rle_encode(dev(mask.astype(np.uint8))[None], capacity=max(2, g.counts[i].size))
        nr, rows = host_rows(enc[0], enc[1])
        assert np.array_equal(rows[0], fx.rows[i]), g.names[i]


@pytest.mark.parametrize("n", [0, 1, 3000])
def test_one_call_for_no_part_one_part_and_thousands(fx, n):
    from maskrcnn_amd import ops
    g = fx.g
    idx = [(7 * j) % len(g.names) for j in range(n)]                       # the golden cases cycled: mixed image sizes
    nr, cnt, nk = ops.rle_from_poly(*poly_args([g.xy[i] for i in idx], [g.h[i] for i in idx], [g.w[i] for i in idx]))
    assert nr.shape == (n,) and nk.shape == (n,) and cnt.shape[0] == n
    nr_h, rows = host_rows(nr, cnt)
    assert same_rows(rows, [g.counts[i] for i in idx]) and np.array_equal(nk.cpu().numpy(), fx.keys[idx])
    if n == 3000:
        assert sum(g.names[i] == "serpentine" for i in idx) >= 5


def test_two_runs_are_bit_identical(fx):
    from maskrcnn_amd import ops
    again = ops.rle_from_poly(*fx.args)
    live = torch.arange(fx.counts.size(1), device=DEV)[None, :] < fx.num_runs[:, None]
    assert torch.equal(again[0], fx.num_runs) and torch.equal(again[2], fx.num_keys)
    assert torch.equal(again[1][live], fx.counts[live])


def raw_from_poly(args, capacity, band=64, extra_ws=256):
    """mrcnn_rle_from_poly_f64 on buffers of this test's own: poisoned guard bands round every output, poisoned rows, and a
    poisoned tail behind the workspace."""
    from maskrcnn_amd import _lib
    xy, off, hs, ws_ = args
    n, v = hs.numel(), xy.shape[0]
    i32 = lambda count: torch.full((count + 2 * band,), POISON, dtype=torch.int32, device=DEV)
    num_runs, num_keys, counts = i32(n), i32(n), i32(n * capacity)
    need = int(_lib.lib.mrcnn_rle_from_poly_workspace_bytes(n, v))
    wsb = torch.full((need + extra_ws,), 0x5A, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib.mrcnn_rle_from_poly_f64(xy.data_ptr(), v, off.data_ptr(), hs.data_ptr(), ws_.data_ptr(), n, capacity,
                                                num_runs[band:].data_ptr(), counts[band:].data_ptr(), num_keys[band:].data_ptr(),
                                                wsb.data_ptr(), need, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for buf, count in ((num_runs, n), (num_keys, n), (counts, n * capacity)):
        host = buf.cpu().numpy()
        assert (host[:band] == POISON).all() and (host[band + count:] == POISON).all()
    assert (wsb[need:].cpu().numpy() == 0x5A).all()
    return (num_runs[band:band + n].cpu().numpy(), counts[band:band + n * capacity].cpu().numpy().view(np.uint32).reshape(n, capacity),
            num_keys[band:band + n].cpu().numpy())


def test_a_part_over_capacity_reports_its_runs_and_nothing_is_written_outside(fx):
    g = fx.g
    sel = [g.index(n) for n in ("triangle_int", "star5", "rect_frac", "serpentine", "bowtie", "random_11")]
    want = [g.counts[i] for i in sel]
    args = poly_args([g.xy[i] for i in sel], [g.h[i] for i in sel], [g.w[i] for i in sel])
    for victim in (1, 3):                                                  # an on-chip part, then the range-by-range one
        cap = want[victim].size - 1                                        # one run short
        nr, cnt, nk = raw_from_poly(args, cap)
        fits = [j for j in range(len(sel)) if want[j].size <= cap]
        assert victim not in fits and len(fits) >= (2 if victim == 1 else 5)
        for j in range(len(sel)):
            assert nr[j] == want[j].size and nk[j] == fx.keys[sel[j]], (victim, j)          # the true counts, fitting or not
            if j in fits:
                assert np.array_equal(cnt[j, :nr[j]], want[j]) and (cnt[j, nr[j]:] == POISON).all(), (victim, j)
            else:
                assert (cnt[j] == POISON).all(), (victim, j)                                # the row is untouched
    nr, cnt, nk = raw_from_poly(args, want[3].size)                        # exactly enough: everything is written
    for j in range(len(sel)):
        assert np.array_equal(cnt[j, :nr[j]], want[j]) and (cnt[j, nr[j]:] == POISON).all()


def test_a_part_with_more_vertices_than_the_on_chip_vertex_cache(fx):
    """3 000 and 2 049 vertices: the scanned edge counts of such a part live in the workspace, not in LDS. Against the numpy
    restatement, which tests/test_poly_host.py pins to the reference; 2 048 vertices, the last size that stays on chip, too.
    And the sizes of the on-chip sort: rectangles with exactly 257 keys below h*w (one more than the workgroup has threads),
    with rle_from_poly_onchip_keys() of them (the sort's capacity, no padding) and with one more (range by range)."""
    from maskrcnn_amd import ops
    from test_poly_host import fr_poly_ref, poly_keys_ref
    g = fx.g
    onchip = ops.rle_from_poly_onchip_keys()
    # a rectangle over c pixel columns has 2c crossings; with its lower edge on y == h of the LAST column one of them is the
    # alias key h*w, which is not sorted
    rect = lambda x0, y0, x1, y1: np.array([[x0, y0], [x0, y1], [x1, y1], [x1, y0]], dtype=np.float64)
    sized = [(rect(11, 1, 140, 4), 4, 140, 257), (rect(2, .5, 2 + onchip // 2, 1.5), 2, onchip // 2 + 4, onchip),
             (rect(0, 1, onchip // 2 + 1, 2), 2, onchip // 2 + 1, onchip + 1)]
    for xy, h, w, m in sized:
        assert int((poly_keys_ref(xy, h, w) < h * w).sum()) == m
    nr, cnt, nk = raw_from_poly(poly_args([s[0] for s in sized], [s[1] for s in sized], [s[2] for s in sized]), onchip + 8)
    for j, (xy, h, w, m) in enumerate(sized):
        want = fr_poly_ref(xy, h, w)
        assert nr[j] == want.size and np.array_equal(cnt[j, :nr[j]], want) and (cnt[j, nr[j]:] == POISON).all(), m
        assert nk[j] == poly_keys_ref(xy, h, w).size and want.size >= m
    rng = np.random.default_rng(11)
    def ring(k, h, w):
        a = np.sort(rng.uniform(0, 2 * np.pi, k))
        r = rng.uniform(0.2, 0.55, k)
        return np.round(np.stack([w / 2 + r * w * np.cos(a), h / 2 + r * h * np.sin(a)], 1), 2)
    tri = g.xy[g.index("triangle_int")]
    xys = [tri, ring(3000, 300, 400), ring(2049, 120, 90), ring(2048, 120, 90), tri]
    hs, ws = [33, 300, 120, 120, 33], [37, 400, 90, 90, 37]
    want = [fr_poly_ref(x, h, w) for x, h, w in zip(xys, hs, ws)]
    nr, cnt, nk = raw_from_poly(poly_args(xys, hs, ws), max(c.size for c in want) + 3)
    for j in range(5):
        assert nr[j] == want[j].size and np.array_equal(cnt[j, :nr[j]], want[j]) and (cnt[j, nr[j]:] == POISON).all(), j
    assert want[1].size > 500 and nk[1] >= want[1].size - 1


def test_parts_past_a_limit_are_refused_on_the_device_and_neighbours_stay_exact(fx):
    """With a capacity the call reads nothing back, so a part past a documented limit reports num_runs = num_keys = -1."""
    g = fx.g
    tri, i0 = g.xy[g.index("triangle_int")], g.index("triangle_int")
    far = 2.0 ** 31 / 5
    xys = [tri, tri, tri, np.array([[1, 1], [np.nan, 4], [5, 8]]), np.array([[1, 1], [far, 4], [5, 8]]),
           np.array([[0, 0], [2.0 ** 23 / 5, 0]]), np.array([[1, 1], [np.inf, 4], [5, 8]]), tri, tri, tri]
    hs = [33, 0, 33, 33, 33, 33, 33, 16385, 33, 33]
    ws = [37, 37, 16385, 37, 37, 37, 37, 37, 0, 37]
    nr, cnt, nk = raw_from_poly(poly_args(xys, hs, ws), 64)
    good = [0, 9]
    for j in range(10):
        if j in good:
            assert nr[j] == g.counts[i0].size and np.array_equal(cnt[j, :nr[j]], g.counts[i0]) and nk[j] == fx.keys[i0], j
        else:
            assert nr[j] == -1 and nk[j] == -1 and (cnt[j] == POISON).all(), j
    # offsets that do not increase, or point outside the vertices: refused part by part, nothing is read out of bounds
    xy, _, h3, w3 = poly_args([tri, tri, tri], [33] * 3, [37] * 3)
    for off, bad in (([0, 3, 3, 9], [1]), ([0, 3, 2, 9], [1]), ([0, 3, 6, 10], [2]), ([-1, 3, 6, 9], [0])):
        nr, cnt, nk = raw_from_poly((xy, dev(off, np.int32), h3, w3), 64)
        for j in range(3):
            if j in bad:
                assert nr[j] == -1 and nk[j] == -1, (off, j)
            elif off[j + 1] - off[j] == 3 and off[j] % 3 == 0:
                assert np.array_equal(cnt[j, :nr[j]], g.counts[i0]), (off, j)


# ------------------------------------------------------------------------------------------------ rle_merge
def group_table(fx, groups):
    """The member rows of `groups`, gathered from the shared table on the device, and their offsets."""
    g = fx.g
    members = [m for k in groups for m in g.members[k]]
    cap = max(g.counts[m].size for m in members)
    idx = dev(members, np.int64)
    off = np.concatenate([[0], np.cumsum([len(g.members[k]) for k in groups])])
    return fx.num_runs[idx], fx.counts[idx, :cap].contiguous(), dev(off, np.int32)


@pytest.mark.parametrize("intersect", [False, True])
def test_merge_equals_the_golden_grouped_and_group_by_group(fx, intersect):
    from maskrcnn_amd import ops
    g = fx.g
    want = g.inter if intersect else g.union
    every = list(range(len(g.group_names)))
    nr, rows = host_rows(*ops.rle_merge(*group_table(fx, every), intersect=intersect))
    for k in every:
        assert nr[k] == want[k].size and np.array_equal(rows[k], want[k]), g.group_names[k]
    for k in every:
        out = torch.ops.maskrcnn.rle_merge(*group_table(fx, [k]), intersect) if k % 2 else ops.rle_merge(*group_table(fx, [k]), intersect)
        nr1, rows1 = host_rows(*out)
        assert np.array_equal(rows1[0], want[k]), g.group_names[k]
    again = ops.rle_merge(*group_table(fx, every), intersect=intersect)
    assert np.array_equal(host_rows(*again)[0], nr) and same_rows(host_rows(*again)[1], rows)     # run to run


def test_merge_of_long_rows_empty_groups_and_rows_over_capacity(fx):
    from maskrcnn_amd import _lib, ops
    from test_poly_host import merge_ref
    g = fx.g
    # the serpentine (32 257 runs) with itself and with a 512 x 516 rectangle: more events than a workgroup has threads, by far
    s = g.index("serpentine")
    h, w = g.h[s], g.w[s]
    extra = [np.array([[100, 50], [400, 50], [400, 300], [100, 300]], dtype=np.float64), np.array([[-5, -5], [600, -5], [600, 600], [-5, 600]], dtype=np.float64)]
    nr, cnt, _ = ops.rle_from_poly(*poly_args([g.xy[s]] + extra, [h] * 3, [w] * 3))
    rows = host_rows(nr, cnt)[1]
    assert np.array_equal(rows[0], g.counts[s])
    off = dev([0, 2, 2, 3, 3], np.int32)                                     # groups: {snake, rect}, {}, {full}, {}
    for intersect in (False, True):
        m_nr, m_rows = host_rows(*ops.rle_merge(nr, cnt, off, intersect))
        assert m_nr.tolist()[1::2] == [0, 0] and np.array_equal(m_rows[0], merge_ref(rows[:2], intersect)) and m_rows[0].size > 8192
        assert np.array_equal(m_rows[2], rows[2])                           # a group of one: a copy
    # capacity one short: the true num_runs, the row untouched, the neighbours exact, guard bands and the workspace tail intact
    every = list(range(len(g.group_names)))
    t_nr, t_cnt, t_off = group_table(fx, every)
    victim = int(np.argmax([u.size for u in g.union]))
    cap, band, G = g.union[victim].size - 1, 64, len(every)
    out_nr = torch.full((G + 2 * band,), POISON, dtype=torch.int32, device=DEV)
    out_cnt = torch.full((G * cap + 2 * band,), POISON, dtype=torch.int32, device=DEV)
    need = int(_lib.lib.mrcnn_rle_merge_workspace_bytes(t_nr.numel(), t_cnt.size(1)))
    wsb = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib.mrcnn_rle_merge(t_nr.data_ptr(), t_cnt.data_ptr(), t_nr.numel(), t_cnt.size(1), t_off.data_ptr(), G, 0, cap,
                                        out_nr[band:].data_ptr(), out_cnt[band:].data_ptr(), wsb.data_ptr(), need,
                                        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    nr_h, cnt_h = out_nr.cpu().numpy(), out_cnt.cpu().numpy().view(np.uint32)
    assert (nr_h[:band] == POISON).all() and (nr_h[band + G:] == POISON).all() and (wsb[need:].cpu().numpy() == 0x5A).all()
    assert (cnt_h[:band] == POISON).all() and (cnt_h[band + G * cap:] == POISON).all()
    body = cnt_h[band:band + G * cap].reshape(G, cap)
    for k in every:
        assert nr_h[band + k] == g.union[k].size, g.group_names[k]
        if g.union[k].size > cap:
            assert (body[k] == POISON).all()
        else:
            assert np.array_equal(body[k, :g.union[k].size], g.union[k]) and (body[k, g.union[k].size:] == POISON).all()
    assert (body[victim] == POISON).all()
    # a member that was over ITS capacity when it was made: the group reports -1; the other group of the call is exact
    members = sorted(g.members[victim], key=lambda m: g.counts[m].size)    # the longest last
    assert len(members) >= 3 and g.counts[members[-1]].size > g.counts[members[0]].size
    short = ops.rle_from_poly(*poly_args([g.xy[m] for m in members], [40] * len(members), [50] * len(members)),
                              capacity=g.counts[members[-1]].size - 1)
    assert int(short[0][-1]) == short[1].size(1) + 1
    m_nr, m_rows = host_rows(*ops.rle_merge(short[0], short[1], dev([0, 1, len(members)], np.int32), capacity=4096))
    assert m_nr[1] == -1 and np.array_equal(m_rows[0], g.counts[members[0]])


# ------------------------------------------------------------------------------------------------ annToRLE and the evaluation
def test_ann_to_rle_equals_the_reference_annotation_by_annotation(fx):
    from maskrcnn_amd import cocoeval
    z = fx.g.z
    gt, _ = eval_inputs()
    out = cocoeval.ann_to_rle(gt)
    by_id = {a["id"]: a for a in out["annotations"]}
    sizes = {img["id"]: [img["height"], img["width"]] for img in gt["images"]}
    for n, ann_id in enumerate(z["ann_ids"].tolist()):
        seg = by_id[ann_id]["segmentation"]
        want = z["ann_cnt"][z["ann_cnt_off"][n]:z["ann_cnt_off"][n + 1]]
        assert seg["size"] == sizes[by_id[ann_id]["image_id"]] and seg["counts"] == want.tolist(), ann_id
    for a, b in zip(gt["annotations"], out["annotations"]):               # the input is not changed; dicts are left as they are
        assert (a["segmentation"] == b["segmentation"]) == isinstance(a["segmentation"], dict) and a["id"] == b["id"]
    assert sum(isinstance(a["segmentation"], list) for a in gt["annotations"]) == len(z["ann_ids"])


def check_against_golden(ev, z):
    for name in ("precision", "recall", "scores", "stats"):
        got, want = getattr(ev, name), z[f"segm_{name}"]
        assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want), name
    assert ev.summary() == z["segm_summary"].tolist()
    seen, at = 0, 0
    for key, shape in zip(z["segm_iou_key"].tolist(), z["segm_iou_shape"].tolist()):
        want = z["segm_iou"][at:at + shape[0] * shape[1]].reshape(shape)
        at += shape[0] * shape[1]
        assert np.array_equal(ev.ious[tuple(key)], want), key
        seen += 1
    assert seen == sum(1 for v in ev.ious.values() if len(v)) and seen > 20


def test_evaluate_on_polygon_ground_truth_equals_the_golden(fx, tmp_path):
    from maskrcnn_amd import cocoeval
    z = fx.g.z
    gt, results = eval_inputs()
    ev = cocoeval.evaluate(gt, results, "segm", polygons="rasterize")
    check_against_golden(ev, z)
    via = cocoeval.evaluate(cocoeval.ann_to_rle(gt), results, "segm")       # rasterised first, then the RLE-only path
    check_against_golden(via, z)
    for key in ev.ious:
        assert np.array_equal(np.asarray(ev.ious[key]), np.asarray(via.ious[key])), key
    (tmp_path / "gt.json").write_text(str(z["gt_json"]))
    (tmp_path / "res.json").write_text(str(z["results_json"]))
    r = subprocess.run([sys.executable, "-m", "maskrcnn_amd.cocoeval", str(tmp_path / "gt.json"), str(tmp_path / "res.json"),
                        "--type", "segm", "--polygons", "rasterize"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.splitlines() == z["segm_summary"].tolist()


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused(fx):
    from maskrcnn_amd import ops
    g = fx.g
    tri = g.xy[g.index("triangle_int")]
    xy, off, hs, ws = poly_args([tri, tri], [33, 33], [37, 37])
    with pytest.raises(RuntimeError, match="float64"):
        ops.rle_from_poly(xy.float(), off, hs, ws)
    with pytest.raises(RuntimeError, match="int32"):
        ops.rle_from_poly(xy, off.long(), hs, ws)
    with pytest.raises(RuntimeError, match="int32"):
        ops.rle_from_poly(xy, off, hs.long(), ws)
    with pytest.raises(RuntimeError, match="offsets"):
        ops.rle_from_poly(xy, off[:2], hs, ws)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.rle_from_poly(xy.cpu(), off, hs, ws)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.rle_from_poly(xy, off, hs, ws.cpu())
    with pytest.raises(RuntimeError, match="start at 0"):
        ops.rle_from_poly(xy, dev([1, 3, 6], np.int32), hs, ws)
    with pytest.raises(RuntimeError, match="no vertex"):
        ops.rle_from_poly(xy, dev([0, 6, 6], np.int32), hs, ws)
    for bad_h, bad_w in ((0, 37), (16385, 37), (33, 0), (33, 16385)):       # the first size past each limit
        with pytest.raises(RuntimeError, match="outside"):
            ops.rle_from_poly(xy, off, dev([33, bad_h], np.int32), dev([37, bad_w], np.int32))
    nr, cnt, _ = ops.rle_from_poly(xy, off, dev([33, 16384], np.int32), dev([16384, 37], np.int32))   # the last sizes inside them
    assert nr.tolist()[0] >= 1 and nr.tolist()[1] >= 1
    for bad in (np.nan, np.inf, 2.0 ** 31 / 5):
        with pytest.raises(RuntimeError, match="finite|2\\^31"):
            ops.rle_from_poly(dev(np.concatenate([tri, [[1.0, bad]], tri[:2]])), off, hs, ws)
    with pytest.raises(RuntimeError, match="boundary points"):
        ops.rle_from_poly(dev([[0, 0], [2.0 ** 23 / 5, 0]], np.float64), dev([0, 2], np.int32), hs[:1], ws[:1])
    with pytest.raises(ops.MaskrcnnHipError, match="capacity"):
        ops.rle_from_poly(xy, off, hs, ws, capacity=0)
    with pytest.raises(RuntimeError, match="group_off"):
        ops.rle_merge(fx.num_runs, fx.counts, dev([0, 2], np.int64))
    with pytest.raises(RuntimeError, match="non-decreasing"):
        ops.rle_merge(fx.num_runs, fx.counts, dev([0, 3, 2], np.int32))
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.rle_merge(fx.num_runs.cpu(), fx.counts.cpu(), dev([0, 2], np.int32))
    nr, _ = ops.rle_merge(fx.num_runs, fx.counts, dev([0, 2, 999999], np.int32), capacity=8)   # sync-free: refused on the device
    assert nr.tolist()[1] == -1


# ------------------------------------------------------------------------------------------------ schedule fuzzing
def test_kernel_tests_pass_under_schedule_fuzzing():
    """This file's kernel tests in a fresh process on the schedule-fuzzing build (tests/test_gpu_sync_fuzz.py)."""
    assert os.path.exists(FUZZ_LIB), f"{FUZZ_LIB} is missing: run __graft_entry__.build()"
    env = dict(os.environ, MRCNN_LIB=FUZZ_LIB, MRCNN_SYNC_FUZZ_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_poly.py", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider",
                        "-k", "not schedule_fuzzing and not evaluate_on_polygon"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
