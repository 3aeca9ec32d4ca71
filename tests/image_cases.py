"""The image kernels (csrc/image.hip: paste_masks_kernel, the five launch sequences of mrcnn_resize_bilinear_u8, mold_kernel) as
case tables that reach every regime ON PURPOSE, with data built so that one specific mistake changes the result, and plain
references that can be told to make each of those mistakes. tests/test_image_cases_host.py checks the tables, the mutants and
the references (against Pillow live) without a GPU; tests/test_gpu_image_edges.py runs the cases.

  * PASTE_CASES    one canvas and a handful of detections each; paste_regimes(case) derives from the boxes alone which branches
                   of paste_masks_kernel every detection reaches (tap loops per axis, 256-column chunks, 32-row tiles, store width,
                   validity), PASTE_TABLE is the list the union must cover.
  * RESIZE_CASES   (n, in_h, in_w, c, out_h, out_w, crop, dst_offset) with the launch sequence each is meant to take
                   (ops.resize_route says which one the launcher does take).
  * MOLD_CASES     (n, in_h, in_w, new_h, new_w, top, left, out_h, out_w, mean).
  * paste_ref / resize_ref / mold_ref    restatements on oracle.pil_resize_u8 / oracle.f32_to_l8 that take `mut`, one of MUTANTS.

Pure numpy; the oracle (the C restatement of Pillow's resample) is imported inside the functions that need it."""
import dataclasses
import functools
import math
import zlib

import numpy as np

f32 = np.float32
TILE_ROWS, CHUNK = 32, 256            # paste_masks_kernel
FV_ROWS, FV_COLS = 16, 256            # resample_hv1_u8_fused
PRECISION_BITS = 22
MEAN_PIXEL = (123.7, 116.8, 103.9)    # config.py: MEAN_PIXEL
# float(double(p) - mean) != float(p) - float(mean) for these (checked by the host test): the subtraction must be in double
MEAN_DOUBLE = (1.0 / 3.0, 100.00000381, 127.5000001)

MUTANTS = ("ge_127", "round_f2l", "int_then_sub", "sub_f32", "one_pass", "v_then_h", "no_stretch", "shift_col", "shift_row",
           "next_class", "transpose_mask", "premultiply")
RESAMPLE_MUTANTS = ("one_pass", "v_then_h", "no_stretch")


def _rng(case_id, salt=0):
    return np.random.default_rng([zlib.crc32(case_id.encode()), salt])


# ---------------------------------------------------------------------------------------------------------------------
# Pillow's 8-bit BILINEAR resample in numpy, with the mistakes a kernel could make (mut). With mut None it equals
# oracle.pil_resize_u8 (the host test checks that); the references use the oracle for mut None and this for the mutants.
# ---------------------------------------------------------------------------------------------------------------------
def coeffs(in_size, out_size, stretch=True):
    """precompute_coeffs + normalize_coeffs_8bpc → bounds [out,2] (xmin, count), kk [out,ksize]. stretch False: the support is
    not widened by the scale when shrinking (mutant no_stretch)."""
    scale = float(f32(in_size)) / out_size
    fs = max(scale, 1.0) if stretch else 1.0
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * (1.0 / fs))) for x in range(cnt)]
        ww = 0.0
        for v in w:
            ww += v
        w = [v / ww if ww != 0.0 else v for v in w]
        bounds[xx] = (xmin, cnt)
        kk[xx, :cnt] = [int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
    return bounds, kk


def _pass(a, bounds, kk, axis, exact):
    """One pass along `axis` of a [h,w,c] array. exact: keep the real-valued sum (no 8-bit rounding)."""
    a = np.moveaxis(a, axis, 0)
    out = np.empty((len(bounds),) + a.shape[1:], np.float64 if exact else np.uint8)
    for xx, (xmin, cnt) in enumerate(bounds):
        k = kk[xx, :cnt].reshape((cnt,) + (1,) * (a.ndim - 1))
        if exact:
            out[xx] = (a[xmin:xmin + cnt].astype(np.float64) * k).sum(0) / (1 << PRECISION_BITS)
        else:
            ss = (1 << (PRECISION_BITS - 1)) + (a[xmin:xmin + cnt].astype(np.int64) * k).sum(0)
            out[xx] = np.clip(ss >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resample_np(image, out_h, out_w, mut=None):
    """uint8 [h,w] or [h,w,c] → [out_h,out_w(,c)]: horizontal pass into an 8-bit intermediate, then the vertical pass.
    mut: one_pass (no 8-bit intermediate: one rounding at the end), v_then_h (vertical first), no_stretch."""
    a = np.asarray(image, np.uint8)
    squeeze = a.ndim == 2
    if squeeze:
        a = a[:, :, None]
    stretch = mut != "no_stretch"
    bh, kh = coeffs(a.shape[1], out_w, stretch)
    bv, kv = coeffs(a.shape[0], out_h, stretch)
    if mut == "one_pass":
        out = _pass(_pass(a, bh, kh, 1, True), bv, kv, 0, True)
        out = np.clip(np.floor(out + 0.5), 0, 255).astype(np.uint8)
    elif mut == "v_then_h":
        out = _pass(_pass(a, bv, kv, 0, False), bh, kh, 1, False)
    else:
        out = _pass(_pass(a, bh, kh, 1, False), bv, kv, 0, False)
    return out[:, :, 0] if squeeze else out


def _resize(image, out_h, out_w, mut):
    if mut in RESAMPLE_MUTANTS:
        return resample_np(image, out_h, out_w, mut)
    from oracle import oracle
    return oracle.pil_resize_u8(image, out_h, out_w)


# ---------------------------------------------------------------------------------------------------------------------
# paste_masks
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Det:
    box: tuple      # (y1, x1, y2, x2) as written; the kernel sees float32(box)
    cls: int
    note: str = ""
    fill: str = ""      # "grey127" / "grey128": the selected class's whole mask is that constant


@dataclasses.dataclass(frozen=True)
class PasteCase:
    id: str
    H: int
    W: int
    mh: int
    mw: int
    C: int
    layout: str             # "nchw" [N,C,mh,mw] (the reference's) or "nhwc" [N,mh,mw,C]
    view: str               # "contiguous", "class2" (every second class of a tensor with 2C classes), "slice_mh" (rows 1..mh of mh+3)
    out_offset: int         # bytes `out` is placed past a 16-byte boundary
    dets: tuple
    nonfinite: bool = False

    @property
    def store_width(self):
        return 16 if self.W % 16 == 0 and self.out_offset % 16 == 0 else 4


def box32(det):
    """The four coordinates as the doubles the kernel and the reference compute with: float32 values widened."""
    return tuple(float(f32(v)) for v in det.box)


def box_geometry(det, mut=None):
    """(bh, bw, top, left) as data.py:295-303 computes them (Python float = double), or None when a coordinate has no int."""
    y1, x1, y2, x2 = box32(det)
    if not all(math.isfinite(v) for v in (y1, x1, y2, x2)):
        return None
    if mut == "int_then_sub":
        bh, bw = int(y2) - int(y1), int(x2) - int(x1)
    elif mut == "sub_f32":
        bh, bw = int(f32(y2) - f32(y1)), int(f32(x2) - f32(x1))
    else:
        bh, bw = int(y2 - y1), int(x2 - x1)
    return bh, bw, int(y1), int(x1)


def det_valid(case, det, mut=None):
    """Whether the reference can paste this detection: a box of at least one pixel inside the canvas (int(-0.5) == 0 is inside,
    -1 is not) and a class the mask tensor has. Everything else is an all-zero mask by this project's definition."""
    g = box_geometry(det, mut)
    if g is None:
        return False
    bh, bw, top, left = g
    y1, x1 = box32(det)[:2]
    return (bh >= 1 and bw >= 1 and y1 > -1 and x1 > -1 and top + bh <= case.H and left + bw <= case.W
            and 0 <= det.cls < case.C)


def _ksize(in_size, out_size):
    return int(math.ceil(max(float(f32(in_size)) / out_size, 1.0))) * 2 + 1


def _axis_kind(in_size, out_size):
    if out_size > in_size:
        return "enlarge"
    if out_size == in_size:
        return "equal"
    return "shrink5" if _ksize(in_size, out_size) == 5 else "shrink7+"


AXIS_KINDS = ("enlarge", "equal", "shrink5", "shrink7+")
NONFINITE_BOX_VALUES = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf"), "3e9": 3e9}

PASTE_TABLE = tuple(
    [f"axis:h={h},v={v}" for h in AXIS_KINDS for v in AXIS_KINDS] + ["axis:ksize129"] +
    ["chunks:1", "chunks:2", "chunks:3", "left%16==0", "left%16!=0", "px4:left%4!=0", "right:on_group", "right:off_group",
     "lastcol:chunk255", "lastcol:chunk256", "right==W"] +
    ["rows:one_tile", "rows:all_three", "top:on_tile_start", "bottom:on_tile_end", "onerow:first_of_tile", "onerow:last_of_tile",
     "bottom==H"] +
    ["store:16", "store:4_by_width", "store:4_by_pointer"] +
    [f"mask:{s}" for s in ("28x28", "1x1", "64x64", "5x64", "64x5")] +
    ["layout:nchw", "layout:nhwc", "view:nchw_class2", "view:nhwc_class2", "view:slice_mh", "cls:0", "cls:C-1"] +
    ["box:fractional", "box:f64_sub_19_f32_sub_20", "box:int_sub_31_sub_int_32", "box:y1=-0.5"] +
    ["invalid:h_trunc_0", "invalid:w_trunc_0", "invalid:h=0.99", "invalid:reversed", "invalid:y1=-1", "invalid:past_bottom_by_1",
     "invalid:past_right_by_1", "invalid:cls=-1", "invalid:cls=C"] +
    [f"invalid:{name}@{pos}" for name in NONFINITE_BOX_VALUES for pos in range(4)] +
    ["invalid:wraps_int_sum"])


def paste_regimes(case):
    """For every detection of the case, the set of regimes (names of PASTE_TABLE) it reaches — from the boxes, the class ids and
    the case's canvas, mask size and layout alone; nothing here looks at a note or at an id."""
    px = case.store_width
    per_det = []
    for det in case.dets:
        r = set()
        y1, x1, y2, x2 = box32(det)
        if det_valid(case, det):
            bh, bw, top, left = box_geometry(det)
            r.add(f"axis:h={_axis_kind(case.mw, bw)},v={_axis_kind(case.mh, bh)}")
            if _ksize(case.mw, bw) == 129 or _ksize(case.mh, bh) == 129:
                r.add("axis:ksize129")
            cb = (left // px) * px
            nchunks = -(-(left + bw - cb) // CHUNK)
            if nchunks <= 3:
                r.add(f"chunks:{nchunks}")
            r.add("left%16==0" if left % 16 == 0 else "left%16!=0")
            if px == 4 and case.W % 16 != 0 and left % 4 != 0:
                r.add("px4:left%4!=0")
            r.add("right:on_group" if (left + bw) % px == 0 else "right:off_group")
            if left + bw - 1 - cb == 255:
                r.add("lastcol:chunk255")
            if left + bw - 1 - cb == 256:
                r.add("lastcol:chunk256")
            if left + bw == case.W:
                r.add("right==W")
            if top // TILE_ROWS == (top + bh - 1) // TILE_ROWS:
                r.add("rows:one_tile")
            if top < TILE_ROWS and top + bh > 2 * TILE_ROWS and case.H <= 3 * TILE_ROWS:
                r.add("rows:all_three")
            if top % TILE_ROWS == 0:
                r.add("top:on_tile_start")
            if (top + bh) % TILE_ROWS == 0:
                r.add("bottom:on_tile_end")
            if bh == 1 and top % TILE_ROWS == 0:
                r.add("onerow:first_of_tile")
            if bh == 1 and top % TILE_ROWS == TILE_ROWS - 1:
                r.add("onerow:last_of_tile")
            if top + bh == case.H and case.H % TILE_ROWS != 0:
                r.add("bottom==H")
            r.add("store:16" if px == 16 else "store:4_by_width" if case.W % 16 else "store:4_by_pointer")
            r.add(f"mask:{case.mh}x{case.mw}")
            r.add(f"layout:{case.layout}")
            if case.view == "class2":
                r.add(f"view:{case.layout}_class2")
            if case.view == "slice_mh":
                r.add("view:slice_mh")
            if det.cls == 0:
                r.add("cls:0")
            if det.cls == case.C - 1:
                r.add("cls:C-1")
            if any(v != math.floor(v) for v in (y1, x1, y2, x2)):
                r.add("box:fractional")
            if int(y2 - y1) == 19 and int(f32(y2) - f32(y1)) == 20:
                r.add("box:f64_sub_19_f32_sub_20")
            if int(y2 - y1) == 31 and int(y2) - int(y1) == 32:
                r.add("box:int_sub_31_sub_int_32")
            if y1 == -0.5 and top == 0:
                r.add("box:y1=-0.5")
        else:
            vals = (y1, x1, y2, x2)
            finite = all(math.isfinite(v) for v in vals)
            for name, bad in NONFINITE_BOX_VALUES.items():
                for pos, v in enumerate(vals):
                    others_ok = all(math.isfinite(o) and abs(o) < 1e6 for i, o in enumerate(vals) if i != pos)
                    if others_ok and (v == float(f32(bad)) or (v != v and bad != bad)):
                        r.add(f"invalid:{name}@{pos}")
                        # the slots whose int sum top + bh (left + bw) would wrap or saturate: the far corner, top, left >= 1
                        if name in ("3e9", "+inf") and pos >= 2 and y1 >= 1 and x1 >= 1:
                            r.add("invalid:wraps_int_sum")
            if finite and max(abs(v) for v in vals) < 1e6:
                in_class = 0 <= det.cls < case.C
                if not in_class:
                    r.add("invalid:cls=-1" if det.cls == -1 else "invalid:cls=C" if det.cls == case.C else "invalid:cls")
                elif y2 < y1 or x2 < x1:
                    r.add("invalid:reversed")
                elif int(y2 - y1) == 0 or int(x2 - x1) == 0:
                    if int(y2 - y1) == 0:
                        r.add("invalid:h_trunc_0")
                        if abs((y2 - y1) - 0.99) < 1e-5:
                            r.add("invalid:h=0.99")
                    if int(x2 - x1) == 0:
                        r.add("invalid:w_trunc_0")
                elif y1 == -1 or x1 == -1:
                    r.add("invalid:y1=-1")
                elif y1 >= 0 and x1 >= 0 and int(y1) + int(y2 - y1) == case.H + 1 and int(x1) + int(x2 - x1) <= case.W:
                    r.add("invalid:past_bottom_by_1")
                elif y1 >= 0 and x1 >= 0 and int(x1) + int(x2 - x1) == case.W + 1 and int(y1) + int(y2 - y1) <= case.H:
                    r.add("invalid:past_right_by_1")
        per_det.append(frozenset(r))
    return per_det


def _d(y1, x1, y2, x2, cls=0, note=""):
    return Det((y1, x1, y2, x2), cls, note)


def _hw(top, left, bh, bw, cls=0, note="", fill=""):
    return Det((top, left, top + bh, left + bw), cls, note, fill)


def _constants(top, left, bh, bw):
    """Two detections whose whole masks are the constants either side of the threshold: all off, all on."""
    return (_hw(top, left, bh, bw, 0, "grey 127 everywhere: all off", "grey127"),
            _hw(top, left, bh, bw, 1, "grey 128 everywhere: all on", "grey128"))


def _axes_dets():
    """All sixteen horizontal x vertical tap-loop combinations of a 28 x 28 mask, side by side on the canvas."""
    size = {"enlarge": 33, "equal": 28, "shrink5": 20, "shrink7+": 9}
    dets, left = [], 1
    for hi, hk in enumerate(AXIS_KINDS):
        for vi, vk in enumerate(AXIS_KINDS):
            dets.append(_hw((7 * hi + 5 * vi) % (80 - size[vk] + 1), left, size[vk], size[hk], (hi + vi) % 3, f"{hk} x {vk}"))
            left += size[hk] + 3
    return tuple(dets)


# chunk and row-tile regimes on the W = 544 canvas with 16-byte stores (and, by pointer, with 4-byte stores)
_CHUNK_DETS_544 = (
    _hw(35, 16, 20, 240, 0, "one chunk, left % 16 == 0, inside one row tile"),
    _hw(5, 3, 70, 253, 1, "last column at chunk column 255; right edge 256 on a group border; all three row tiles"),
    _hw(32, 3, 32, 254, 2, "last column at chunk column 256: a second chunk of one column; exactly the middle row tile"),
    _hw(70, 10, 10, 534, 0, "three chunks, right edge == W, bottom edge == H in the ragged tile"),
    _hw(64, 100, 1, 300, 1, "one row, the first of a tile; two chunks from chunk start 96"),
    _hw(31, 257, 1, 40, 2, "one row, the last of a tile"),
    _hw(0, 500, 64, 41, 0, "top and bottom on tile borders, right edge off a group border"),
)
# the same on W = 532 (W % 16 != 0: 4-byte stores, chunk starts at multiples of 4)
_CHUNK_DETS_532 = (
    _hw(35, 5, 20, 100, 0, "left % 4 != 0"),
    _hw(5, 6, 70, 254, 1, "chunk start 4; last column at chunk column 255; right edge 260 on a group border"),
    _hw(32, 6, 32, 255, 2, "last column at chunk column 256"),
    _hw(70, 2, 10, 530, 0, "three chunks, right edge == W == 532, bottom edge == H"),
    _hw(64, 101, 1, 300, 1, "one row, the first of a tile; right edge 401 off a group border"),
    _hw(31, 258, 1, 41, 2, "one row, the last of a tile"),
    _hw(0, 491, 64, 41, 0, "right edge == W from a left that is no multiple of 4"),
)
_BOX_VALUE_DETS = (
    _d(0.3, 10.25, 20.3, 50.75, 0, "float64 difference of the fp32 values truncates to 19, an fp32 subtraction gives 20"),
    _d(16.6, 70.5, 48.6, 110.25, 1, "int(y2 - y1) = 31, int(y2) - int(y1) = 32"),
    _d(-0.5, 130.0, 30.25, 170.0, 2, "y1 = -0.5 is valid with top == 0"),
    _d(40.75, -0.5, 79.99, 27.6, 0, "x1 = -0.5 is valid with left == 0; equal width 28"),
    _d(10.9, 200.9, 60.1, 260.1, 1, "every corner fractional"),
    _d(0.3, 300.6, 20.3, 332.6, 2, "both subtraction traps in one box"),
) + _constants(7, 350, 50, 100) + _constants(60, 460, 9, 13)


def _invalid_dets(H, W, C):
    good = (_hw(3, 5, 30, 40, 0, "valid neighbour"), _hw(40, 300, 33, 29, C - 1, "valid neighbour"))
    bad = [
        _d(10, 20, 10.5, 60, 0, "height truncates to 0"),
        _d(10, 20, 50, 20.75, 1, "width truncates to 0"),
        _d(10.0, 20, 10.99, 60, 0, "height 0.99"),
        _d(50, 20, 10, 60, 1, "reversed in y"),
        _d(10, 60, 50, 20, 0, "reversed in x"),
        _d(-1, 20, 30, 60, 0, "y1 = -1"),
        _d(10, -1, 30, 60, 0, "x1 = -1"),
        _d(H - 20, 20, H + 1, 60, 1, "one pixel past the bottom edge"),
        _d(10, W - 40, 30, W + 1, 0, "one pixel past the right edge"),
        _d(10, 20, 50, 60, -1, "class id -1"),
        _d(10, 20, 50, 60, C, "class id C"),
    ]
    for name, v in NONFINITE_BOX_VALUES.items():
        for pos in range(4):
            box = [5.0, 5.0, 50.0, 50.0]      # top, left >= 1: with 3e9 / +inf at the far corner the int sum would wrap
            box[pos] = v
            bad.append(Det(tuple(box), pos % C, f"{name} in position {pos}"))
    dets = []
    for i, d in enumerate(bad):                # valid neighbours among the invalid slots
        if i % 9 == 0:
            dets.append(good[(i // 9) % 2])
        dets.append(d)
    dets.append(good[1])
    return tuple(dets)


PASTE_CASES = (
    PasteCase("axes_28x28_nchw", 80, 544, 28, 28, 3, "nchw", "contiguous", 0, _axes_dets()),
    PasteCase("chunks_544_nhwc", 80, 544, 28, 28, 3, "nhwc", "contiguous", 0, _CHUNK_DETS_544),
    PasteCase("chunks_532_nchw", 80, 532, 28, 28, 3, "nchw", "contiguous", 0, _CHUNK_DETS_532),
    PasteCase("chunks_544_out_plus_4", 80, 544, 28, 28, 3, "nchw", "contiguous", 4, _CHUNK_DETS_544),
    PasteCase("box_values", 80, 544, 28, 28, 3, "nhwc", "contiguous", 0, _BOX_VALUE_DETS),
    PasteCase("box_values_532", 80, 532, 28, 28, 3, "nchw", "class2", 0, _BOX_VALUE_DETS),
    PasteCase("mask_1x1", 80, 544, 1, 1, 2, "nchw", "contiguous", 0,
              (_hw(0, 0, 80, 544, 0, "the whole canvas from one value"), _hw(10, 17, 1, 1, 1, "equal: one pixel"),
               _hw(33, 250, 30, 13, 0), _hw(79, 543, 1, 1, 1, "the last pixel")) + _constants(40, 300, 20, 200)),
    PasteCase("mask_64x64_nhwc_class2", 80, 544, 64, 64, 4, "nhwc", "class2", 0,
              (_hw(2, 7, 70, 300, 0, "enlarge both"), _hw(8, 320, 64, 64, 3, "equal both"),
               _hw(3, 400, 40, 1, 1, "one column from 64: ksize 129"), _hw(77, 410, 1, 90, 2, "one row from 64: ksize 129"),
               _hw(40, 405, 33, 47, 3, "ksize 5 both"), _hw(0, 460, 9, 7, 0, "ksize 17 x 21"))),
    PasteCase("mask_5x64_nchw_class2", 80, 532, 5, 64, 3, "nchw", "class2", 0,
              (_hw(1, 2, 5, 64, 0, "equal"), _hw(10, 70, 3, 400, 2, "rows shrink, columns enlarge over two chunks"),
               _hw(20, 9, 60, 31, 1, "rows enlarge, columns shrink"), _hw(40, 480, 1, 1, 2, "one pixel"))),
    PasteCase("mask_64x5_nhwc_slice_mh", 80, 544, 64, 5, 3, "nhwc", "slice_mh", 0,
              (_hw(1, 2, 64, 5, 0, "equal"), _hw(10, 70, 31, 400, 2, "rows shrink, columns enlarge"),
               _hw(0, 500, 80, 3, 1, "rows enlarge, columns shrink"), _hw(40, 480, 1, 1, 2, "one pixel"))),
    PasteCase("mask_28x28_nchw_slice_mh", 80, 544, 28, 28, 3, "nchw", "slice_mh", 0, _CHUNK_DETS_544[:3]),
    PasteCase("invalid_slots", 80, 544, 28, 28, 3, "nchw", "contiguous", 0, _invalid_dets(80, 544, 3)),
    PasteCase("invalid_slots_532", 80, 532, 28, 28, 3, "nhwc", "contiguous", 0, _invalid_dets(80, 532, 3)),
    PasteCase("nonfinite_masks", 80, 544, 28, 28, 3, "nchw", "contiguous", 0,
              (_hw(3, 5, 60, 200, 0), _hw(20, 250, 28, 28, 1), _hw(1, 300, 13, 20, 2), _hw(30, 330, 50, 214, 0)), nonfinite=True),
)

GREY_127 = f32(0.5)              # 0.5 * 255 = 127.5 → 127: every pixel off
GREY_128 = f32(128.5 / 255.0)    # → 128: every pixel on


def planted_values(nonfinite):
    """Mask values where clamp, truncation and the threshold decide: k/255 for k = 127, 128 with both fp32 neighbours (the fp32
    product with 255 lands on either side of the integer), the ends of the clamp, and, where asked, the non-finite ones."""
    vals = []
    for k in (127, 128):
        v = f32(k / 255.0)
        vals += [np.nextafter(v, f32(0)), v, np.nextafter(v, f32(1))]
    vals += [f32(0.0), f32(-0.0), f32(1.0), np.nextafter(f32(1), f32(2)), f32(2.0), f32(-0.25), f32(1e-45)]
    if nonfinite:
        vals += [f32("nan"), f32("inf"), f32("-inf"), -f32("nan")]
    return np.array(vals, f32)


@functools.lru_cache(maxsize=None)
def _paste_base(case_id):
    case = paste_case(case_id)
    rng = _rng(case.id)
    n = len(case.dets)
    cb = case.C * (2 if case.view == "class2" else 1)
    mhb = case.mh + (3 if case.view == "slice_mh" else 0)
    base = (f32(0.5) + rng.integers(-40, 41, (n, cb, mhb, case.mw)).astype(f32) / f32(255)).astype(f32)
    sel = mask_view(case, base, layout="nchw")              # [n, C, mh, mw] view of base
    plant = planted_values(case.nonfinite)
    for i, det in enumerate(case.dets):
        for c in range(case.C):
            m = sel[i, c]
            if m.size >= 4 * len(plant):                     # m is a view: the writes go to base
                ys, xs = np.unravel_index(rng.choice(m.size, 2 * len(plant), replace=False), m.shape)
                m[ys, xs] = np.concatenate([plant, plant])
        if det.fill:
            sel[i, det.cls] = {"grey127": GREY_127, "grey128": GREY_128}[det.fill]    # two whole masks pin `> 127`
    if case.layout == "nhwc":
        base = np.ascontiguousarray(base.transpose(0, 2, 3, 1))
    base.setflags(write=False)
    return base


def mask_view(case, base, layout=None):
    """The [N,C,mh,mw] / [N,mh,mw,C] tensor the kernel is given, as a view of the base tensor (numpy or torch: slicing only)."""
    layout = layout or case.layout
    if case.view == "class2":
        return base[:, ::2] if layout == "nchw" else base[..., ::2]
    if case.view == "slice_mh":
        return base[:, :, 1:1 + case.mh] if layout == "nchw" else base[:, 1:1 + case.mh]
    return base


def paste_inputs(case):
    """→ (base fp32 tensor, read-only; the masks are mask_view(case, base)), class_ids int64 [N], boxes fp32 [N,4]."""
    ids = np.array([d.cls for d in case.dets], np.int64)
    with np.errstate(over="ignore"):
        boxes = np.array([d.box for d in case.dets], np.float64).astype(f32)
    return _paste_base(case.id), ids, boxes


def paste_case(case_id):
    return next(c for c in PASTE_CASES if c.id == case_id)


def f2l(a, mut=None):
    """mask * 255.0 in fp32 → 'L' (clamp, truncate; NaN is 0). round_f2l: rounds to nearest instead."""
    from oracle import oracle
    a = np.ascontiguousarray(a, f32)
    if mut == "round_f2l":
        with np.errstate(invalid="ignore"):
            r = np.where(a > 0, np.minimum(np.floor(a.astype(np.float64) + 0.5), 255), 0)
        return np.nan_to_num(r, nan=0.0).astype(np.uint8)
    return oracle.f32_to_l8(a)


def paste_ref(case, mut=None):
    """data.py:287-314 for the case → uint8 0 / 1 [N,H,W]; invalid slots all zero. mut: one of MUTANTS (those that do not
    apply to the paste leave it as it is)."""
    base, ids, _ = paste_inputs(case)
    masks = mask_view(case, base)
    if case.layout == "nhwc":
        masks = masks.transpose(0, 3, 1, 2)
    out = np.zeros((len(case.dets), case.H, case.W), np.uint8)
    for i, det in enumerate(case.dets):
        if not det_valid(case, det):
            continue                                        # decided without the mutant: a mutant does not widen what is valid
        bh, bw, top, left = box_geometry(det, mut)
        cls = (det.cls + 1) % case.C if mut == "next_class" else det.cls
        m = np.ascontiguousarray(masks[i, cls])
        if mut == "transpose_mask":
            m = m.reshape(case.mw, case.mh).T
        with np.errstate(over="ignore", invalid="ignore"):
            img = f2l(m * f32(255.0), mut)                                      # :291, :294
        if bh < 1 or bw < 1 or top + bh > case.H or left + bw > case.W:       # a mutant geometry may not fit: leave the slot empty
            continue
        img = _resize(img, bh, bw, mut)                                        # :295
        full = np.zeros((case.H, case.W), np.uint8)
        if mut == "shift_col":
            full[top:top + bh, left + 1:left + bw] = img[:, :bw - 1]
        elif mut == "shift_row":
            full[top + 1:top + bh, left:left + bw] = img[:bh - 1]
        else:
            full[top:top + bh, left:left + bw] = img                           # :305
        out[i] = (full >= 127) if mut == "ge_127" else (full > 127)            # :308
    return out


# ---------------------------------------------------------------------------------------------------------------------
# resize
# ---------------------------------------------------------------------------------------------------------------------
ROUTES = ("fused", "hfast_vfast", "hfast_vgeneric", "hgeneric_vfast", "generic")      # == ops.RESIZE_ROUTES


@dataclasses.dataclass(frozen=True)
class ResizeCase:
    id: str
    n: int
    in_h: int
    in_w: int
    c: int
    out_h: int
    out_w: int
    crop: tuple          # (top, left, bottom, right) rows / columns of the base tensor around the images: a strided view
    dst_offset: int      # bytes dst is placed past a 16-byte boundary
    route: str           # the launch sequence the case is meant to take
    kinds: tuple         # of "enlarge", "shrink", "ragged", "identity", "extreme"
    data: str = "random"   # "random", "alpha255", "plant_row3", "plant_row", "plant_col" (+ "_twin": the planted byte is 0)


def _rc(id, n, in_h, in_w, c, out_h, out_w, route, kinds, crop=(0, 0, 0, 0), dst_offset=0, data="random"):
    return ResizeCase(id, n, in_h, in_w, c, out_h, out_w, crop, dst_offset, route, tuple(kinds.split()), data)


RESIZE_CASES = (
    # ---- fused: one channel, enlarging (or equal) both ways, out_w % 16 == 0, aligned dst
    _rc("fused_up_ragged", 1, 10, 12, 1, 23, 32, "fused", "enlarge ragged"),
    _rc("fused_identity", 1, 40, 48, 1, 40, 48, "fused", "identity ragged"),
    _rc("fused_identity_256", 1, 16, 256, 1, 16, 256, "fused", "identity"),
    _rc("fused_w16", 1, 7, 5, 1, 19, 16, "fused", "enlarge ragged"),
    _rc("fused_w240", 1, 9, 100, 1, 21, 240, "fused", "enlarge ragged"),
    _rc("fused_w272", 1, 30, 90, 1, 37, 272, "fused", "enlarge ragged"),
    _rc("fused_w528", 1, 11, 200, 1, 18, 528, "fused", "enlarge ragged"),
    _rc("fused_n3_crop", 3, 20, 24, 1, 50, 64, "fused", "enlarge ragged", crop=(3, 5, 2, 7)),
    _rc("fused_in_w_1", 1, 9, 1, 1, 20, 32, "fused", "enlarge ragged"),
    _rc("fused_plant_row3", 1, 7, 40, 1, 95, 48, "fused", "enlarge ragged", data="plant_row3"),
    _rc("fused_plant_row3_twin", 1, 7, 40, 1, 95, 48, "fused", "enlarge ragged", data="plant_row3_twin"),
    _rc("fused_plant_row", 1, 12, 40, 1, 40, 48, "fused", "enlarge ragged", data="plant_row"),
    _rc("fused_plant_row_twin", 1, 12, 40, 1, 40, 48, "fused", "enlarge ragged", data="plant_row_twin"),
    _rc("fused_plant_col", 1, 9, 200, 1, 20, 528, "fused", "enlarge ragged", data="plant_col"),
    _rc("fused_plant_col_twin", 1, 9, 200, 1, 20, 528, "fused", "enlarge ragged", data="plant_col_twin"),
    _rc("fused_2x2_to_16384x16", 1, 2, 2, 1, 16384, 16, "fused", "enlarge extreme"),
    # ---- h-fast + v-fast: one channel, not shrinking in width, 16-byte rows, but shrinking in height
    _rc("hfast_vfast_up_w", 1, 40, 12, 1, 17, 32, "hfast_vfast", "enlarge shrink ragged"),
    _rc("hfast_vfast_long_rows", 1, 9, 300, 1, 5, 4112, "hfast_vfast", "enlarge shrink ragged"),
    _rc("hfast_vfast_in_w_1", 1, 9, 1, 1, 5, 32, "hfast_vfast", "enlarge shrink ragged", crop=(1, 2, 3, 4)),
    # ---- h-fast + v-generic: out_w % 4 == 0 but not % 16, or an unaligned dst
    _rc("hfast_vgeneric_up", 1, 10, 12, 1, 23, 36, "hfast_vgeneric", "enlarge ragged"),
    _rc("hfast_vgeneric_down_h", 1, 30, 12, 1, 7, 36, "hfast_vgeneric", "shrink ragged"),
    _rc("hfast_vgeneric_in_h_1", 1, 1, 9, 1, 32, 20, "hfast_vgeneric", "enlarge ragged"),
    _rc("unaligned_dst_1", 1, 10, 12, 1, 23, 32, "hfast_vgeneric", "enlarge ragged", dst_offset=1),
    _rc("unaligned_dst_4", 3, 20, 24, 1, 50, 64, "hfast_vgeneric", "enlarge ragged", crop=(3, 5, 2, 7), dst_offset=4),
    # ---- h-generic + v-fast: several channels or shrinking in width, 16-byte rows
    _rc("hgeneric_vfast_rgb_up", 1, 10, 12, 3, 20, 32, "hgeneric_vfast", "enlarge ragged"),
    _rc("hgeneric_vfast_down", 1, 50, 100, 1, 20, 32, "hgeneric_vfast", "shrink ragged"),
    _rc("hgeneric_vfast_la", 1, 10, 12, 2, 20, 24, "hgeneric_vfast", "enlarge ragged"),
    _rc("hgeneric_vfast_rgba", 1, 10, 12, 4, 20, 24, "hgeneric_vfast", "enlarge ragged"),
    _rc("hgeneric_vfast_rgba_alpha255", 1, 10, 12, 4, 20, 24, "hgeneric_vfast", "enlarge ragged", data="alpha255"),
    _rc("hgeneric_vfast_n3_crop_down", 3, 33, 70, 1, 12, 48, "hgeneric_vfast", "shrink ragged", crop=(2, 3, 4, 5)),
    _rc("la_1x16384_identity", 1, 1, 16384, 2, 1, 16384, "hgeneric_vfast", "identity extreme"),
    # ---- generic + generic
    _rc("generic_la", 1, 10, 12, 2, 20, 25, "generic", "enlarge ragged"),
    _rc("generic_la_alpha255", 1, 10, 12, 2, 20, 25, "generic", "enlarge ragged", data="alpha255"),
    _rc("generic_rgba", 1, 10, 12, 4, 20, 25, "generic", "enlarge ragged"),
    _rc("generic_rgb_down", 1, 31, 45, 3, 9, 13, "generic", "shrink ragged"),
    _rc("generic_rgb_crop", 1, 31, 45, 3, 40, 51, "generic", "enlarge ragged", crop=(1, 2, 3, 4)),
    _rc("generic_1x1_to_37x53", 1, 1, 1, 1, 37, 53, "generic", "enlarge ragged"),
    _rc("generic_n3_crop_odd", 3, 20, 24, 1, 13, 31, "generic", "shrink ragged", crop=(3, 5, 2, 7)),
    _rc("generic_16384x3_to_1x3", 1, 16384, 3, 1, 1, 3, "generic", "shrink extreme"),
    _rc("generic_3x16384_to_3x1", 1, 3, 16384, 1, 3, 1, "generic", "shrink extreme"),
    _rc("generic_5x1x4_to_16384x1", 1, 5, 1, 4, 16384, 1, "generic", "enlarge extreme"),
    _rc("generic_7x16384_to_7x15", 1, 7, 16384, 1, 7, 15, "generic", "shrink extreme"),
)
# what every route must be reached by ("shrink where the route allows": the fused route never shrinks)
ROUTE_KINDS = {"fused": ("enlarge", "ragged", "identity"), "hfast_vfast": ("enlarge", "shrink", "ragged"),
               "hfast_vgeneric": ("enlarge", "shrink", "ragged"), "hgeneric_vfast": ("enlarge", "shrink", "ragged"),
               "generic": ("enlarge", "shrink", "ragged")}


def resize_case(case_id):
    return next(c for c in RESIZE_CASES if c.id == case_id)


def only_last_row_reads(in_size, out_size, tile):
    """Input indices that, of all the output rows of one tile of `tile` rows, only the tile's LAST row reads — the footprint
    entries `bounds[last] + 3` (the zero-tile test of resample_hv1_u8_fused) exists for. → [(tile index, input index, tap
    index, coefficient)], the highest tap first per tile. Enlarging, Pillow's window is int(c + 1.5) - int(c - 0.5): two taps,
    three only where the two truncations round apart — and then the third coefficient is 0 (the host test pins that)."""
    from oracle import oracle
    bounds, kk = oracle.resample_coeffs(in_size, out_size)
    found = []
    for t in range(-(-out_size // tile)):
        y0, y1 = t * tile, min((t + 1) * tile, out_size)
        read = set()
        for yy in range(y0, y1 - 1):
            read.update(range(bounds[yy, 0], bounds[yy, 0] + bounds[yy, 1]))
        last = y1 - 1
        for tap in reversed(range(bounds[last, 1])):
            idx = int(bounds[last, 0]) + tap
            if idx not in read:
                found.append((t, idx, tap, int(kk[last, tap])))
    return found


def plant_position(case):
    """(row, column) of the planted byte of a plant_* case and the (tile row, tile column) that reads it through its last row
    (column) only."""
    kind = case.data.replace("_twin", "")
    if kind == "plant_row3":          # a last row with three taps: the byte sits under the third, whose coefficient is 0
        t, idx, tap, k = next(f for f in only_last_row_reads(case.in_h, case.out_h, FV_ROWS) if f[2] == 2)
        return (idx, case.in_w // 2), (t, 0)
    if kind == "plant_row":           # the last tap with a non-zero coefficient
        t, idx, tap, k = next(f for f in only_last_row_reads(case.in_h, case.out_h, FV_ROWS) if k_nonzero(f))
        return (idx, case.in_w // 2), (t, 0)
    if kind == "plant_col":
        t, idx, tap, k = next(f for f in only_last_row_reads(case.in_w, case.out_w, FV_COLS) if k_nonzero(f))
        return (case.in_h // 2, idx), (0, t)
    raise ValueError(case.data)


def k_nonzero(found):
    return found[3] != 0


@functools.lru_cache(maxsize=None)
def _resize_base(case_id):
    case = resize_case(case_id)
    t, l, b, r = case.crop
    shape = (case.n, t + case.in_h + b, l + case.in_w + r, case.c)
    rng = _rng(case.id.replace("_twin", ""))
    if case.data.startswith("plant"):
        # zero, except the planted byte (0 in the twin) and one byte that another tile reads, so that the image is not empty
        base = np.zeros(shape, np.uint8)
        (py, px), tile = plant_position(case)
        oy, ox = (0, 0) if tile != (0, 0) else (case.in_h - 1, case.in_w - 1)
        base[0, t + oy, l + ox, 0] = 200
        base[0, t + py, l + px, 0] = 0 if case.data.endswith("_twin") else 255
    else:
        base = rng.integers(0, 256, shape, dtype=np.uint8)
        if case.data == "alpha255":
            base[..., -1] = 255
    base.setflags(write=False)
    return base


def resize_inputs(case):
    """→ (base uint8 [n, H, W, c], view [n, in_h, in_w, c] of it: what the kernel is pointed at, strides and all)."""
    base = _resize_base(case.id)
    t, l, _, _ = case.crop
    return base, base[:, t:t + case.in_h, l:l + case.in_w]


def _premultiplied_resize(img, out_h, out_w):
    """What a resize that treats the last channel as alpha does (Pillow's LA / RGBA): premultiply, resample, divide."""
    from oracle import oracle
    a = img[..., -1:].astype(np.int64)
    pre = img.copy()
    pre[..., :-1] = (img[..., :-1].astype(np.int64) * a + 127) // 255
    out = oracle.pil_resize_u8(pre, out_h, out_w)
    oa = out[..., -1:].astype(np.int64)
    out[..., :-1] = np.where(oa > 0, np.minimum((out[..., :-1].astype(np.int64) * 255 + oa // 2) // np.maximum(oa, 1), 255), 0)
    return out


def resize_ref(case, mut=None):
    """uint8 [n, out_h, out_w, c]: every image, every channel on its own, through Pillow's 8-bit BILINEAR resample."""
    _, view = resize_inputs(case)
    out = np.empty((case.n, case.out_h, case.out_w, case.c), np.uint8)
    for i in range(case.n):
        img = np.ascontiguousarray(view[i])
        if mut == "premultiply" and case.c in (2, 4):
            out[i] = _premultiplied_resize(img, case.out_h, case.out_w)
            continue
        got = _resize(img, case.out_h, case.out_w, mut)
        if mut == "shift_col" and case.out_w > 1:
            got = np.concatenate([got[:, :1], got[:, :-1]], 1)
        if mut == "shift_row" and case.out_h > 1:
            got = np.concatenate([got[:1], got[:-1]], 0)
        out[i] = got
    return out


# ---------------------------------------------------------------------------------------------------------------------
# mold
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class MoldCase:
    id: str
    n: int
    in_h: int
    in_w: int
    new_h: int
    new_w: int
    top: int
    left: int
    out_h: int
    out_w: int
    mean: tuple = MEAN_PIXEL


MOLD_CASES = (
    MoldCase("resize_odd_pads", 1, 10, 12, 23, 31, 3, 5, 40, 47),
    MoldCase("no_resize_at_origin", 1, 10, 12, 10, 12, 0, 0, 16, 21),
    MoldCase("resize_at_origin", 1, 10, 12, 15, 16, 0, 0, 15, 16),
    MoldCase("shrink_flush_bottom_right", 1, 40, 50, 13, 17, 37 - 13, 41 - 17, 37, 41),
    MoldCase("no_resize_flush_bottom_right", 1, 13, 9, 13, 9, 20 - 13, 30 - 9, 20, 30),
    MoldCase("n3_resize", 3, 8, 6, 12, 9, 1, 2, 17, 13),
    MoldCase("n3_no_resize", 3, 8, 6, 8, 6, 5, 3, 17, 13),
    MoldCase("one_pixel", 1, 1, 1, 1, 1, 2, 3, 5, 7),
    MoldCase("one_pixel_resized", 1, 1, 1, 3, 4, 1, 1, 5, 7),
    MoldCase("mean_needs_double", 1, 16, 16, 16, 16, 1, 1, 19, 18, MEAN_DOUBLE),
    MoldCase("mean_needs_double_resized", 1, 10, 12, 23, 31, 3, 5, 40, 47, MEAN_DOUBLE),
    # 129 x 16384 = 2,113,536 pixels > 2^21 = 8192 blocks x 256 threads: the second trip of mold_kernel's grid-stride loop.
    # Linear pixel 2^21 is (128, 0): the 9 x 11 image covers rows 120 .. 128 from column 0, on both sides of it
    MoldCase("canvas_over_2_21_pixels", 1, 5, 7, 9, 11, 120, 0, 129, 16384),
)


def mold_case(case_id):
    return next(c for c in MOLD_CASES if c.id == case_id)


@functools.lru_cache(maxsize=None)
def mold_inputs(case_id):
    case = mold_case(case_id)
    a = _rng(case.id).integers(0, 256, (case.n, case.in_h, case.in_w, 3), dtype=np.uint8)
    if case.id.startswith("mean_needs_double") and (case.new_h, case.new_w) == (case.in_h, case.in_w):
        a.reshape(-1)[:256] = np.arange(256)                # every byte value under every mean
    a.setflags(write=False)
    return a


def mold_ref(case):
    """float32 [n,3,out_h,out_w]: oracle.mold_image of the oracle's resize, zero-padded to the canvas."""
    from oracle import oracle
    src = mold_inputs(case.id)
    out = np.empty((case.n, 3, case.out_h, case.out_w), f32)
    for i in range(case.n):
        img = src[i]
        if (case.new_h, case.new_w) != (case.in_h, case.in_w):
            img = oracle.pil_resize_u8(img, case.new_h, case.new_w)
        canvas = np.zeros((case.out_h, case.out_w, 3), np.uint8)
        canvas[case.top:case.top + case.new_h, case.left:case.left + case.new_w] = img
        out[i] = oracle.mold_image(canvas, case.mean)[0].numpy()
    return out
