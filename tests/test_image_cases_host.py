"""tests/image_cases.py on the host: the tables reach every regime they name, every mutant of the references is noticed by the
cases' data, and the references are Pillow's own results (live) — so that what tests/test_gpu_image_edges.py compares the
kernels with is known to be right, and known to be able to fail."""
import numpy as np
import pytest

import image_cases as ic


# ---------------------------------------------------------------------------------------------------------------- tables
def test_ids_are_unique_and_tables_are_reached():
    for table in (ic.PASTE_CASES, ic.RESIZE_CASES, ic.MOLD_CASES):
        ids = [c.id for c in table]
        assert len(set(ids)) == len(ids)
    assert len(set(ic.PASTE_TABLE)) == len(ic.PASTE_TABLE)
    reached = set()
    for case in ic.PASTE_CASES:
        per_det = ic.paste_regimes(case)
        assert len(per_det) == len(case.dets)
        for det, r in zip(case.dets, per_det):
            assert r, f"{case.id}: {det} reaches nothing the table names"
            assert ic.det_valid(case, det) != any(x.startswith("invalid:") for x in r), (case.id, det, sorted(r))
        reached |= set().union(*per_det)
    assert reached - set(ic.PASTE_TABLE) == set()
    assert [t for t in ic.PASTE_TABLE if t not in reached] == []
    # every invalid slot has valid neighbours in its call
    for case in ic.PASTE_CASES:
        assert any(ic.det_valid(case, d) for d in case.dets), case.id
    # the two constants either side of the threshold are there, all off and all on
    fills = {d.fill for c in ic.PASTE_CASES for d in c.dets}
    assert fills == {"", "grey127", "grey128"}
    assert int(ic.f2l(np.array([ic.GREY_127 * ic.f32(255)]))[0]) == 127 and int(ic.f2l(np.array([ic.GREY_128 * ic.f32(255)]))[0]) == 128


def test_store_width_and_routes_are_the_launchers_answers():
    """The cases' expectations against the host queries of the library (no GPU): the store width of every paste case, and the
    launch sequence of every resize case — every one of the five reached by the kinds of case it allows."""
    from maskrcnn_amd import ops
    assert tuple(ops.RESIZE_ROUTES) == ic.ROUTES
    for case in ic.PASTE_CASES:
        assert ops.paste_store_width(case.W, case.out_offset) == case.store_width, case.id
    assert {(c.W % 16 == 0, c.out_offset, c.store_width) for c in ic.PASTE_CASES} == {(True, 0, 16), (False, 0, 4), (True, 4, 4)}
    for case in ic.RESIZE_CASES:
        assert ops.resize_route(case.n, case.in_h, case.in_w, case.c, case.out_h, case.out_w, case.dst_offset, 0) == case.route, case.id
        if case.n > 1:
            assert case.in_w > 4 or case.c > 1      # a [N,H,W<=4] tensor reads as [H,W,C] in ops.resize_bilinear_u8
    for route, kinds in ic.ROUTE_KINDS.items():
        for kind in kinds:
            assert any(c.route == route and kind in c.kinds for c in ic.RESIZE_CASES), (route, kind)
    for case in ic.RESIZE_CASES:                     # the kinds say what the shapes are
        if "shrink" in case.kinds:
            assert case.out_h < case.in_h or case.out_w < case.in_w, case.id
        if "enlarge" in case.kinds:
            assert case.out_h > case.in_h or case.out_w > case.in_w, case.id
        if "identity" in case.kinds:
            assert (case.out_h, case.out_w) == (case.in_h, case.in_w), case.id
    # an unaligned workspace alone drops the v-fast kernel, an unaligned dst the fused one too
    assert ops.resize_route(1, 10, 12, 1, 23, 32, 0, 0) == "fused" and ops.resize_route(1, 10, 12, 1, 23, 32, 0, 8) == "fused"
    assert ops.resize_route(1, 40, 12, 1, 17, 32, 0, 8) == "hfast_vgeneric" and ops.resize_route(1, 10, 12, 3, 20, 32, 8, 0) == "generic"
    for bad in ((0, 10, 12, 1, 20, 32), (1, 0, 12, 1, 20, 32), (1, 10, 12, 5, 20, 32), (1, 10, 12, 1, 20, 16385)):
        with pytest.raises(RuntimeError, match="resize_route"):
            ops.resize_route(*bad)
    have = {(c.c, c.data) for c in ic.RESIZE_CASES}
    assert {(2, "random"), (4, "random"), (2, "alpha255"), (4, "alpha255")} <= have
    shapes = {(c.in_h, c.in_w, c.c, c.out_h, c.out_w) for c in ic.RESIZE_CASES}
    assert {(16384, 3, 1, 1, 3), (3, 16384, 1, 3, 1), (1, 16384, 2, 1, 16384), (5, 1, 4, 16384, 1), (2, 2, 1, 16384, 16),
            (7, 16384, 1, 7, 15), (1, 1, 1, 37, 53)} <= shapes
    assert {c.out_w for c in ic.RESIZE_CASES if c.route == "fused"} >= {16, 240, 272, 528}
    assert {c.dst_offset for c in ic.RESIZE_CASES} == {0, 1, 4}


def test_planted_bytes_sit_where_only_a_tiles_last_row_or_column_reads_them(oracle):
    """The fused kernel skips a tile whose input footprint (rows bounds[first] .. bounds[last] + 3) is all zero. Each plant_* case
    is zero over the footprint of one tile except for ONE byte that, of the tile's rows (columns), only the last reads; its twin
    has 0 there. plant_row3: that row has three taps and the byte is under the third — whose coefficient is 0, as it is for every
    enlarging size (Pillow's window is two taps wide; a third appears only where two truncations round apart), so the tile's
    output stays zero although it is not skipped. plant_row / plant_col: the last tap with a weight; no out_w <= 4096 that is a
    multiple of 16 has a three-tap column at the end of a 256-column tile, so there is no plant_col3."""
    for i in range(1, 64):
        for o in range(i, 4 * i):
            b, k = oracle.resample_coeffs(i, o)
            assert k.shape[1] == 3 and not k[:, 2].any()
    for case in (c for c in ic.RESIZE_CASES if c.data.startswith("plant")):
        twin = case.data.endswith("_twin")
        (py, px), (ty, tx) = ic.plant_position(case)
        _, view = ic.resize_inputs(case)
        img = view[0, :, :, 0]
        bv, kv = oracle.resample_coeffs(case.in_h, case.out_h)
        bh, kh = oracle.resample_coeffs(case.in_w, case.out_w)
        y0, y1 = ty * ic.FV_ROWS, min((ty + 1) * ic.FV_ROWS, case.out_h)
        x0, x1 = tx * ic.FV_COLS, min((tx + 1) * ic.FV_COLS, case.out_w)
        r0, r1 = bv[y0, 0], min(bv[y1 - 1, 0] + 3, case.in_h)
        c0, c1 = bh[x0, 0], min(bh[x1 - 1, 0] + 3, case.in_w)
        foot = img[r0:r1, c0:c1]
        assert r0 <= py < r1 and c0 <= px < c1
        assert int(np.count_nonzero(foot)) == (0 if twin else 1) and img[py, px] == (0 if twin else 255)
        assert np.count_nonzero(img) == (1 if twin else 2)                      # another tile has something to do
        rows, row_wise = (bv, True) if "row" in case.data else (bh, False)
        first, last, p = (y0, y1 - 1, py) if row_wise else (x0, x1 - 1, px)
        readers = [yy for yy in range(first, last + 1) if rows[yy, 0] <= p < rows[yy, 0] + rows[yy, 1]]
        assert readers == [last]
        tap = p - rows[last, 0]
        kk = kv if row_wise else kh
        if "row3" in case.data:
            assert tap == 2 and rows[last, 1] == 3 and kk[last, 2] == 0
        else:
            assert tap == rows[last, 1] - 1 and kk[last, tap] != 0
            if not twin:                                                         # the byte reaches the tile's output
                out = ic.resize_ref(case)[0, :, :, 0]
                assert out[y0:y1, x0:x1].any()


def test_mean_needs_double():
    p = np.arange(256, dtype=np.float64)
    for m in ic.MEAN_DOUBLE:
        in_double = (p - m).astype(np.float32)
        in_float = p.astype(np.float32) - np.float32(m)
        assert (in_double != in_float).any()
    big = ic.mold_case("canvas_over_2_21_pixels")
    assert big.out_h * big.out_w > 2 ** 21 and big.out_h * big.out_w == 2113536
    first, last = big.top * big.out_w + big.left, (big.top + big.new_h - 1) * big.out_w + big.left + big.new_w - 1
    assert first < 2 ** 21 <= (big.top + big.new_h - 1) * big.out_w + big.left < last
    ref = ic.mold_ref(ic.mold_case("one_pixel_resized"))
    assert ref.shape == (1, 3, 5, 7) and ref[0, 0, 0, 0] == np.float32(-ic.MEAN_PIXEL[0])


# --------------------------------------------------------------------------------------------------------------- mutants
def test_numpy_resample_is_the_oracles(oracle):
    rng = np.random.default_rng(5)
    for (h, w, c, oh, ow) in ((10, 12, 1, 20, 25), (28, 28, 1, 9, 40), (64, 5, 1, 1, 90), (31, 45, 3, 9, 13), (7, 9, 4, 7, 9),
                              (1, 1, 1, 5, 3)):
        a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        assert np.array_equal(ic.resample_np(a, oh, ow), oracle.pil_resize_u8(a, oh, ow))
        b, k = ic.coeffs(h, oh)
        ob, ok = oracle.resample_coeffs(h, oh)
        assert np.array_equal(b, ob) and np.array_equal(k, ok)


def test_every_mutant_changes_a_reference():
    """Which case notices which mistake (the first in table order; most are noticed by many):
        ge_127          axes_28x28_nchw   pixels at grey 127 exactly; in box_values the grey-127 constant mask turns all on
        round_f2l       axes_28x28_nchw   k/255 * 255 just under k, and 0.5 + n/255 values whose product ends in .5 or more
        int_then_sub    box_values        (16.6, 48.6): 31 rows become 32
        sub_f32         box_values        (0.3, 20.3): 19 rows become 20
        one_pass        axes_28x28_nchw   the 8-bit intermediate's rounding moves pixels across 127 / 128
        v_then_h        axes_28x28_nchw   the same rounding, taken in the other order
        no_stretch      axes_28x28_nchw   every shrinking box
        shift_col       axes_28x28_nchw   shift_row the same
        next_class      axes_28x28_nchw   the classes hold different random masks
        transpose_mask  axes_28x28_nchw   and mask_5x64 / mask_64x5, where the strides differ
        premultiply     hgeneric_vfast_la among the resize cases with c = 2 / 4 and random alpha (the paste has no alpha)"""
    paste_plain = {c.id: ic.paste_ref(c) for c in ic.PASTE_CASES}
    small = [c for c in ic.RESIZE_CASES if "extreme" not in c.kinds]
    resize_plain = {c.id: ic.resize_ref(c) for c in small}
    caught = {}
    for mut in ic.MUTANTS:
        for c in ic.PASTE_CASES:
            if mut != "premultiply" and not np.array_equal(ic.paste_ref(c, mut), paste_plain[c.id]):
                caught[mut] = c.id
                break
        else:
            for c in small:
                if not np.array_equal(ic.resize_ref(c, mut), resize_plain[c.id]):
                    caught[mut] = c.id
                    break
    assert set(caught) == set(ic.MUTANTS), sorted(set(ic.MUTANTS) - set(caught))
    assert caught["int_then_sub"] == caught["sub_f32"] == "box_values"
    assert caught["premultiply"] in ("hgeneric_vfast_la", "hgeneric_vfast_rgba", "generic_la", "generic_rgba")
    for mut in ("one_pass", "v_then_h", "no_stretch", "shift_col", "shift_row"):      # the resize cases notice these too
        assert any(not np.array_equal(ic.resize_ref(c, mut), resize_plain[c.id]) for c in small), mut
    # the mistakes about geometry are noticed by the boxes built for them, each by itself
    bv = ic.paste_case("box_values")
    for mut, note in (("sub_f32", "float64 difference"), ("int_then_sub", "int(y2 - y1) = 31")):
        i = next(i for i, d in enumerate(bv.dets) if d.note.startswith(note))
        assert not np.array_equal(ic.paste_ref(bv, mut)[i], paste_plain[bv.id][i])
    on, off = (next(i for i, d in enumerate(bv.dets) if d.fill == f) for f in ("grey128", "grey127"))
    assert paste_plain[bv.id][on].sum() == 50 * 100 and paste_plain[bv.id][off].sum() == 0
    assert ic.paste_ref(bv, "ge_127")[off].sum() == 50 * 100


# ------------------------------------------------------------------------------------------------------- Pillow, live
def test_paste_reference_is_the_oracles_full_masks(oracle):
    import torch
    for case in ic.PASTE_CASES:
        base, ids, boxes = ic.paste_inputs(case)
        masks = ic.mask_view(case, base)
        masks = masks.transpose(0, 3, 1, 2) if case.layout == "nhwc" else masks
        valid = [i for i, d in enumerate(case.dets) if ic.det_valid(case, d)]
        want = oracle.full_masks(torch.from_numpy(ids[valid]), torch.from_numpy(boxes[valid]),
                                 torch.from_numpy(np.ascontiguousarray(masks[valid])), case.H, case.W).numpy()
        ref = ic.paste_ref(case)
        assert np.array_equal(ref[valid], want.astype(np.uint8)), case.id
        invalid = [i for i in range(len(case.dets)) if i not in valid]
        assert not ref[invalid].any()


def test_oracle_f32_to_l8_maps_nan_to_zero(oracle):
    nan = np.float32("nan")
    a = np.array([nan, -nan, np.inf, -np.inf, 127.99999, 128.0, -0.0, 0.0, 1e-45, 254.99998, 255.0, 1e30, -1e30, 0.99999994], np.float32)
    assert oracle.f32_to_l8(a).tolist() == [0, 0, 255, 0, 127, 128, 0, 0, 0, 254, 255, 255, 0, 0]


def test_paste_reference_is_pillows_literal_sequence(oracle):
    """data.py:291-308 with Pillow itself: fromarray(F).convert('L'), .resize, paste into zeros, > 127 — every valid slot of every
    case, the non-finite masks included (NaN is 0 through Pillow on x86 as well)."""
    Image = pytest.importorskip("PIL.Image")
    for case in ic.PASTE_CASES:
        base, ids, boxes = ic.paste_inputs(case)
        masks = ic.mask_view(case, base)
        masks = masks.transpose(0, 3, 1, 2) if case.layout == "nhwc" else masks
        ref = ic.paste_ref(case)
        for i, det in enumerate(case.dets):
            if not ic.det_valid(case, det):
                continue
            y1, x1, y2, x2 = (float(v) for v in boxes[i])
            with np.errstate(over="ignore", invalid="ignore"):
                img = Image.fromarray(np.ascontiguousarray(masks[i, det.cls]) * np.float32(255.0)).convert("L")
            img = img.resize((int(x2 - x1), int(y2 - y1)), Image.BILINEAR)
            full = Image.new("L", (case.W, case.H), 0)
            full.paste(img, (int(x1), int(y1)))
            assert np.array_equal(ref[i], (np.array(full) > 127).astype(np.uint8)), (case.id, i, det)


def _pil_per_band(Image, img, out_h, out_w):
    bands = [np.array(Image.fromarray(np.ascontiguousarray(img[:, :, ch])).resize((out_w, out_h), Image.BILINEAR))
             for ch in range(img.shape[2])]
    return np.stack(bands, 2)


def test_resize_reference_is_pillows(oracle):
    """c in {1, 3}: Image.resize. c in {2, 4}: a per-band Pillow resize always; Image.resize (LA / RGBA: premultiplied by alpha
    around the resample) where alpha is 255, and NOT where alpha is random — which is what the documentation says."""
    Image = pytest.importorskip("PIL.Image")
    seen = set()
    for case in ic.RESIZE_CASES:
        _, view = ic.resize_inputs(case)
        ref = ic.resize_ref(case)
        for i in range(case.n):
            img = np.ascontiguousarray(view[i])
            if case.c in (1, 3):
                src = img[:, :, 0] if case.c == 1 else img
                want = np.array(Image.fromarray(src).resize((case.out_w, case.out_h), Image.BILINEAR)).reshape(ref[i].shape)
                assert np.array_equal(ref[i], want), case.id
                continue
            assert np.array_equal(ref[i], _pil_per_band(Image, img, case.out_h, case.out_w)), case.id
            whole = np.array(Image.fromarray(img, "LA" if case.c == 2 else "RGBA").resize((case.out_w, case.out_h), Image.BILINEAR))
            opaque = bool((img[..., -1] == 255).all())
            if case.id == "la_1x16384_identity":
                continue                                     # the same size: Pillow copies, alpha or not
            assert np.array_equal(ref[i], whole) == opaque, (case.id, opaque)
            seen.add((case.c, opaque))
    assert seen == {(2, True), (2, False), (4, True), (4, False)}
