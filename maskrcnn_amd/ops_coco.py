"""Bindings of the ops on COCO run-length tables: the evaluation's IoU and matching (csrc/cocoeval.hip), polygons (csrc/poly.hip)
the string codec (csrc/codec.hip)
and the training masks made from such tables (csrc/gt_masks.hip). ops.py re-exports every name here; argument checks and registration are _binding.py's.
The encoder that makes such tables from detection masks, rle_encode (csrc/rle.hip), is on detect()'s path and stays in ops.py
with its rle_default_capacity, which callers replace on the ops module."""
from __future__ import annotations

import numpy as np
import torch

from ._binding import _launch, _need_gpu, _on_device, _ptr, _ptr0, _stream, checked, checked_out, register, workspace
from ._lib import lib


# --------------------------------------------------------------------------------------------------
# COCO evaluation: grouped RLE / box IoU and the matching of evaluateImg (csrc/cocoeval.hip)
# --------------------------------------------------------------------------------------------------
def _table_tensors(obj, op: str):
    """(num_runs, counts) of an image.RleMasks (or anything else with both attributes) or the two tensors themselves, unchecked."""
    if hasattr(obj, "num_runs") and hasattr(obj, "counts"):
        return obj.num_runs, obj.counts
    if not (isinstance(obj, (tuple, list)) and len(obj) == 2 and all(isinstance(t, torch.Tensor) for t in obj)):
        raise RuntimeError(f"{op}: expected an RleMasks or the (num_runs, counts) tensors")
    return obj


def rle_table(obj, op: str):
    """The run-list table every op here reads, checked for the op named `op`: (num_runs int32 [N], counts int32 [N,capacity >= 1]),
    contiguous, on the device — of an image.RleMasks or of the two tensors themselves; uint32 counts are read as int32."""
    num_runs, counts = _table_tensors(obj, op)
    if counts.dtype == getattr(torch, "uint32", None):
        counts = counts.view(torch.int32)
    num_runs = checked(op, "num_runs", num_runs, torch.int32, ("N",))
    return num_runs, checked(op, "counts", counts, torch.int32, (num_runs.size(0), ("capacity", 1)), hint=" (or uint32)")


def _group_offsets(op, m: int, n: int, dt_off, gt_off, out_off, out_len, dev):
    """The three offset tensors of a grouped call (int32, int32, int64, [K+1] each, on the device) and the output length;
    all None = ONE group of every detection against every ground truth."""
    given = [o is not None for o in (dt_off, gt_off, out_off)]
    if not any(given):
        dt_off = torch.tensor([0, m], dtype=torch.int32, device=dev)
        gt_off = torch.tensor([0, n], dtype=torch.int32, device=dev)
        out_off = torch.tensor([0, m * n], dtype=torch.int64, device=dev)
        return dt_off, gt_off, out_off, m * n, True
    if not all(given):
        raise RuntimeError(f"{op}: dt_off, gt_off and out_off come together")
    dt_off = checked(op, "dt_off", dt_off, torch.int32, (("K+1", 1),))
    gt_off = checked(op, "gt_off", gt_off, torch.int32, (dt_off.numel(),))
    out_off = checked(op, "out_off", out_off, torch.int64, (dt_off.numel(),))
    if out_len is None:
        out_len = int(out_off[-1])   # one host read; pass out_len to stay asynchronous
    return dt_off, gt_off, out_off, int(out_len), False


@_on_device
def _rle_iou(dt_num_runs: torch.Tensor, dt_counts: torch.Tensor, gt_num_runs: torch.Tensor, gt_counts: torch.Tensor,
             iscrowd: torch.Tensor | None = None, dt_off: torch.Tensor | None = None, gt_off: torch.Tensor | None = None,
             out_off: torch.Tensor | None = None, out_len: int | None = None, out: torch.Tensor | None = None):
    dnr, dc = rle_table((dt_num_runs, dt_counts), "rle_iou")
    gnr, gc = rle_table((gt_num_runs, gt_counts), "rle_iou")
    m, n, dev = dnr.size(0), gnr.size(0), dnr.device
    crowd = checked("rle_iou", "iscrowd", iscrowd, (torch.uint8, torch.bool), (n,), optional=True, bool_as_uint8=True)
    dt_off, gt_off, out_off, out_len, single = _group_offsets("rle_iou", m, n, dt_off, gt_off, out_off, out_len, dev)
    res = checked_out("rle_iou", "out", out, torch.float64, (("out_len", out_len),), dev, zeros=True)
    nbytes = int(lib.mrcnn_rle_iou_workspace_bytes(m, dc.size(1), n, gc.size(1)))
    ws = workspace(nbytes, dev)
    _launch(lib.mrcnn_rle_iou_f64,
            (dnr.data_ptr(), dc.data_ptr(), m, dc.size(1), gnr.data_ptr(), gc.data_ptr(), n, gc.size(1), _ptr(crowd),
             dt_off.data_ptr(), gt_off.data_ptr(), out_off.data_ptr(), dt_off.numel() - 1, res.data_ptr(), out_len,
             ws.data_ptr(), nbytes, _stream()),
            lambda: (0, (m, n, out_len), 4 * (dc.numel() + gc.numel()) + 8 * out_len, "rle_iou"))
    return res[:m * n].view(n, m).t() if single else res


def rle_iou(dt, gt, iscrowd: torch.Tensor | None = None, dt_off=None, gt_off=None, out_off=None, out_len=None, out=None):
    """maskUtils.iou on run-length masks (rleIou of cocoapi/common/maskApi.c:77-96, the same bits) on the GPU. dt and gt are
    image.RleMasks or their (num_runs int32 [N], counts [N,capacity]) device tensors — what rle_encode returns, no host trip.
    iscrowd: uint8 [len(gt)]. Without offsets: every detection against every ground truth → float64 [m, n] (a Fortran-order
    view, as _mask.pyx:239 returns). Grouped (include/maskrcnn_hip.h): dt_off / gt_off int32 [K+1] and out_off int64 [K+1]
    device tensors name K groups; → the flat float64 [out_len] buffer with group k's o[g*m + d] matrix at out_off[k] (elements
    of no group stay 0). A pair with a mask that did not fit its capacity is -1."""
    return _rle_iou(*_table_tensors(dt, "rle_iou"), *_table_tensors(gt, "rle_iou"), iscrowd, dt_off, gt_off, out_off, out_len, out)


@_on_device
def bbox_iou(dt: torch.Tensor, gt: torch.Tensor, iscrowd: torch.Tensor | None = None, dt_off=None, gt_off=None, out_off=None,
             out_len=None, out=None):
    """maskUtils.iou on boxes (bbIou of maskApi.c:109-120, operation by operation in fp64) for float64 (x, y, w, h) boxes
    dt [m,4] and gt [n,4] on the GPU; single-group and grouped forms and the result layout as rle_iou."""
    _need_gpu(dt, gt)
    dt, gt = (checked("bbox_iou", name, b, torch.float64, ("N", 4)) for name, b in (("dt", dt), ("gt", gt)))
    m, n, dev = dt.size(0), gt.size(0), dt.device
    crowd = checked("bbox_iou", "iscrowd", iscrowd, (torch.uint8, torch.bool), (n,), optional=True, bool_as_uint8=True)
    dt_off, gt_off, out_off, out_len, single = _group_offsets("bbox_iou", m, n, dt_off, gt_off, out_off, out_len, dev)
    res = checked_out("bbox_iou", "out", out, torch.float64, (("out_len", out_len),), dev, zeros=True)
    _launch(lib.mrcnn_bbox_iou_f64,
            (dt.data_ptr(), m, gt.data_ptr(), n, _ptr(crowd), dt_off.data_ptr(), gt_off.data_ptr(), out_off.data_ptr(),
             dt_off.numel() - 1, res.data_ptr(), out_len, _stream()),
            lambda: (0, (m, n, out_len), 32 * (m + n) + 8 * out_len, "bbox_iou"))
    return res[:m * n].view(n, m).t() if single else res


@_on_device
def coco_match(ious: torch.Tensor, dt_off: torch.Tensor, gt_off: torch.Tensor, out_off: torch.Tensor, dt_area: torch.Tensor,
               gt_area: torch.Tensor, gt_iscrowd: torch.Tensor, area_ranges: torch.Tensor, thresholds: torch.Tensor, out=None):
    """The matching of COCOeval.evaluateImg (cocoeval.py:251-300) for every group x area range x IoU threshold in one launch.
    ious: the flat float64 buffer of a grouped rle_iou / bbox_iou with the same offsets; dt_area float64 [N] (detections of a
    group sorted by descending score, cut at maxDet), gt_area float64 [M], gt_iscrowd uint8 [M], area_ranges float64 [A,2],
    thresholds float64 [T], all on the device. → (dt_match int32 [A,T,N], gt_match int32 [A,T,M], dt_ignore uint8 [A,T,N],
    gt_ignore uint8 [A,M]); matches are 1-based positions within the group in input order, 0 = none. `out` = those four
    tensors, preallocated."""
    op, f64 = "coco_match", torch.float64
    _need_gpu(ious, dt_off, gt_off, out_off, dt_area, gt_area, gt_iscrowd, area_ranges, thresholds)
    ious, dt_area, gt_area = (checked(op, name, v, f64, None) for name, v in (("ious", ious), ("dt_area", dt_area), ("gt_area", gt_area)))
    n_dt, n_gt, dev = dt_area.numel(), gt_area.numel(), dt_area.device
    gt_iscrowd = checked(op, "gt_iscrowd", gt_iscrowd, (torch.uint8, torch.bool), None, bool_as_uint8=True)
    if gt_iscrowd.numel() != n_gt:
        raise RuntimeError(f"{op}: gt_iscrowd must be as long as gt_area ({n_gt}), got {gt_iscrowd.numel()}")
    area_ranges = checked(op, "area_ranges", area_ranges, f64, (("A", 1), 2))
    thresholds = checked(op, "thresholds", thresholds, f64, (("T", 1),))
    dt_off, gt_off, out_off, _, _ = _group_offsets(op, n_dt, n_gt, dt_off, gt_off, out_off, 0, dev)
    a, t = area_ranges.size(0), thresholds.numel()
    spec = (("dt_match", torch.int32, (a, t, n_dt)), ("gt_match", torch.int32, (a, t, n_gt)),
            ("dt_ignore", torch.uint8, (a, t, n_dt)), ("gt_ignore", torch.uint8, (a, n_gt)))
    if out is not None and len(out) != len(spec):
        raise RuntimeError(f"{op}: out must hold {len(spec)} tensors ({', '.join(s[0] for s in spec)}), got {len(out)}")
    outs = tuple(checked_out(op, name, None if out is None else o, dtype, shape, dev, zeros=True)
                 for (name, dtype, shape), o in zip(spec, out or spec))
    _launch(lib.mrcnn_coco_match,
            (_ptr0(ious), ious.numel(), dt_off.data_ptr(), gt_off.data_ptr(), out_off.data_ptr(), dt_off.numel() - 1, _ptr0(dt_area),
             n_dt, _ptr0(gt_area), _ptr0(gt_iscrowd), n_gt, area_ranges.data_ptr(), a, thresholds.data_ptr(), t,
             *[_ptr0(o) for o in outs], _stream()),
            lambda: (0, (dt_off.numel() - 1, a, t), 8 * ious.numel(), "coco_match"))
    return outs


register("rle_iou(Tensor dt_num_runs, Tensor dt_counts, Tensor gt_num_runs, Tensor gt_counts, Tensor? iscrowd=None, "
         "Tensor? dt_off=None, Tensor? gt_off=None, Tensor? out_off=None, int? out_len=None) -> Tensor", _rle_iou)
register("bbox_iou(Tensor dt, Tensor gt, Tensor? iscrowd=None, Tensor? dt_off=None, Tensor? gt_off=None, "
         "Tensor? out_off=None, int? out_len=None) -> Tensor", bbox_iou)


# --------------------------------------------------------------------------------------------------
# COCO polygons to run lengths: rleFrPoly and rleMerge, grouped (csrc/poly.hip)
# --------------------------------------------------------------------------------------------------
POLY_MAX_DIM = 16384
POLY_MAX_PART_POINTS = 1 << 24


def poly_host_bounds(xy, vert_off, heights, widths, who: str = "rle_from_poly", error=RuntimeError):
    """The limits of mrcnn_rle_from_poly_f64 (include/maskrcnn_hip.h) checked on host copies of its arguments — numpy: xy float64
    [V,2], vert_off [n+1], heights / widths [n] — and, per part, a conservative bound on the keys the kernel can keep: the sum over
    the edges of |dX| // 5 + 1 (a crossing falls on a pixel column only where u = 2 mod 5). The bound sizes tables; no value computed
    here reaches an output. Raises `error` at the first value past a limit."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    off = np.asarray(vert_off, dtype=np.int64).reshape(-1)
    hs, ws = np.asarray(heights, dtype=np.int64).reshape(-1), np.asarray(widths, dtype=np.int64).reshape(-1)
    n, v = hs.size, xy.shape[0]
    if off.size != n + 1 or ws.size != n:
        raise error(f"{who}: vert_off has {off.size} entries and widths {ws.size} for {n} parts")
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    if off[0] != 0 or off[-1] != v:
        raise error(f"{who}: vert_off must start at 0 and end at the number of vertices {v}, got {int(off[0])} .. {int(off[-1])}")
    k = np.diff(off)
    if (k < 1).any():
        raise error(f"{who}: part {int(np.argmax(k < 1))} has no vertex (vert_off must increase)")
    for name, a in (("height", hs), ("width", ws)):
        if ((a < 1) | (a > POLY_MAX_DIM)).any():
            i = int(np.argmax((a < 1) | (a > POLY_MAX_DIM)))
            raise error(f"{who}: part {i} has {name} {int(a[i])}, outside [1, {POLY_MAX_DIM}]")
    if not np.isfinite(xy).all():
        raise error(f"{who}: vertex {int(np.argmax(~np.isfinite(xy).all(1)))} is not finite")
    g = np.trunc(5.0 * xy + .5)                       # the grid vertices, as floats: no integer can overflow here
    if (np.abs(5.0 * xy + .5) >= 2.0 ** 31).any():
        raise error(f"{who}: vertex {int(np.argmax((np.abs(5.0 * xy + .5) >= 2.0 ** 31).any(1)))}: |5*v + .5| must stay below 2^31")
    nxt = np.arange(1, v + 1)
    nxt[off[1:] - 1] = off[:-1]                       # the closing edge of every part
    d = np.abs(g[nxt] - g)
    sums = lambda per_edge: np.add.reduceat(per_edge, off[:-1])
    points = sums(d.max(1) + 1)
    if (points > POLY_MAX_PART_POINTS).any():
        i = int(np.argmax(points > POLY_MAX_PART_POINTS))
        raise error(f"{who}: part {i} has {int(points[i])} boundary points, more than {POLY_MAX_PART_POINTS}")
    return sums(np.floor(d[:, 0] / 5.0) + 1).astype(np.int64)


def rle_from_poly_onchip_keys() -> int:
    """Keys of one part that rle_from_poly sorts on chip in one piece; a part with more is sorted range by range."""
    return int(lib.mrcnn_rle_from_poly_onchip_keys())


@_on_device
def rle_from_poly(xy: torch.Tensor, vert_off: torch.Tensor, heights: torch.Tensor, widths: torch.Tensor,
                  capacity: int | None = None):
    """maskUtils.frPyObjects on polygons (rleFrPoly of cocoapi/common/maskApi.c:162-202, the same bits) for n polygon parts in one
    call on the GPU. xy float64 [V,2] (or flat [2V]): all parts' vertices; vert_off int32 [n+1]: part i owns vertices
    [vert_off[i], vert_off[i+1]); heights / widths int32 [n]: every part has its own image size. All device tensors.
    → (num_runs int32 [n], counts int32 [n,capacity], num_keys int32 [n]): the run-list table ops.rle_iou and ops.rle_merge read, and
    the column crossings each part kept before the parity rule. A part with more runs than capacity reports its true num_runs and
    its row is not written (uninitialised memory here). capacity=None: the arguments are read back once, checked against the limits
    of include/maskrcnn_hip.h (RuntimeError at the first value past one) and the capacity is the host's key bound + 1, which no part
    exceeds. With a capacity the call never synchronises; a part past a limit then reports num_runs = num_keys = -1."""
    _need_gpu(xy, vert_off, heights, widths)
    op = "rle_from_poly"
    xy = checked(op, "xy", xy, torch.float64, ("V", 2) if xy.dim() == 2 or xy.numel() % 2 else ("2V",))
    vert_off, heights, widths = (checked(op, name, t, torch.int32, ("n",))
                                 for name, t in (("vert_off", vert_off), ("heights", heights), ("widths", widths)))
    n, v = heights.numel(), xy.numel() // 2
    if vert_off.numel() != n + 1 or widths.numel() != n:
        raise RuntimeError(f"{op}: {n} heights need {n} widths and {n + 1} offsets, got {widths.numel()} and {vert_off.numel()}")
    if capacity is None:
        ints = torch.cat([vert_off, heights, widths]).cpu().numpy()
        bounds = poly_host_bounds(xy.cpu().numpy(), ints[:n + 1], ints[n + 1:2 * n + 1], ints[2 * n + 1:])
        capacity = int(bounds.max()) + 1 if n else 1
    capacity = int(capacity)
    dev = xy.device
    num_runs = torch.empty(n, dtype=torch.int32, device=dev)
    num_keys = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(n, max(capacity, 0), dtype=torch.int32, device=dev)
    nbytes = int(lib.mrcnn_rle_from_poly_workspace_bytes(n, v))
    ws = workspace(nbytes, dev)
    _launch(lib.mrcnn_rle_from_poly_f64,
            (_ptr0(xy), v, vert_off.data_ptr(), _ptr0(heights), _ptr0(widths), n, capacity, _ptr0(num_runs), _ptr0(counts),
             _ptr0(num_keys), ws.data_ptr(), nbytes, _stream()),
            lambda: (0, (n, v, capacity), 16 * v + 4 * counts.numel(), "rle_from_poly"))
    return num_runs, counts, num_keys


@_on_device
def rle_merge(num_runs: torch.Tensor, counts: torch.Tensor, group_off: torch.Tensor, intersect: bool = False,
              capacity: int | None = None):
    """maskUtils.merge (rleMerge of cocoapi/common/maskApi.c:49-70, the same bits) for G groups in one call on the GPU: group g is
    the union (intersect=False) or the intersection of rows [group_off[g], group_off[g+1]) of the table (num_runs int32 [N],
    counts [N,capacity_in]); group_off int32 [G+1] on the device. → (num_runs int32 [G], counts int32 [G,capacity]). An empty group
    has num_runs 0; a group with more runs than capacity reports its true num_runs and its row is not written; a group holding a
    row that was over its own capacity reports -1. capacity=None: one read of the group sizes, and the capacity is the longest
    group's total run count, which no result exceeds. Contract as for rle_iou: the rows of a group cover the same pixel count and
    only a leading run may be empty."""
    num_runs, counts = rle_table((num_runs, counts), "rle_merge")
    group_off = checked("rle_merge", "group_off", group_off, torch.int32, (("G+1", 1),))
    n, g, dev = num_runs.size(0), group_off.numel() - 1, num_runs.device
    if capacity is None:
        nr, off = num_runs.cpu().numpy().astype(np.int64), group_off.cpu().numpy().astype(np.int64)
        if (off < 0).any() or (off > n).any() or (np.diff(off) < 0).any():
            raise RuntimeError(f"rle_merge: group_off must be non-decreasing within [0, {n}]")
        csum = np.concatenate([[0], np.cumsum(np.clip(nr, 0, counts.size(1)))])
        capacity = max(1, int((csum[off[1:]] - csum[off[:-1]]).max())) if g else 1
    capacity = int(capacity)
    out_runs = torch.empty(g, dtype=torch.int32, device=dev)
    out_counts = torch.empty(g, max(capacity, 0), dtype=torch.int32, device=dev)
    nbytes = int(lib.mrcnn_rle_merge_workspace_bytes(n, counts.size(1)))
    ws = workspace(nbytes, dev)
    _launch(lib.mrcnn_rle_merge,
            (_ptr0(num_runs), _ptr0(counts), n, counts.size(1), group_off.data_ptr(), g, 1 if intersect else 0, capacity,
             _ptr0(out_runs), _ptr0(out_counts), ws.data_ptr(), nbytes, _stream()),
            lambda: (0, (n, g, capacity), 4 * (counts.numel() + out_counts.numel()), "rle_merge"))
    return out_runs, out_counts


register("rle_from_poly(Tensor xy, Tensor vert_off, Tensor heights, Tensor widths, int? capacity=None) -> (Tensor, Tensor, Tensor)",
         rle_from_poly)
register("rle_merge(Tensor num_runs, Tensor counts, Tensor group_off, bool intersect=False, int? capacity=None) -> (Tensor, Tensor)",
         rle_merge)


# --------------------------------------------------------------------------------------------------
# The COCO RLE codec on tables: rleFrString, rleToString, rleArea + rleToBbox, rleDecode (csrc/codec.hip)
# --------------------------------------------------------------------------------------------------
# status bits of rle_from_string (include/maskrcnn_hip.h): the first five refuse the row (num_runs = -1), the last two flag it
RLE_BAD_BYTE, RLE_LONG_TOKEN, RLE_OPEN_TOKEN, RLE_BAD_SIZE, RLE_BAD_OFFSETS = 1, 2, 4, 8, 64
RLE_EMPTY_RUN, RLE_PIXEL_SUM = 16, 32


def rle_string_tokens(data, str_off) -> np.ndarray:
    """Tokens (= runs) of every string of a packed HOST buffer — numpy uint8 [total] and offsets [n+1] — as int64 [n]: the
    characters with ((b - 48) & 0x20) == 0, counted with one cumulative sum read at the offsets. No Python loop per character or
    per string; this is how a front end finds the capacity for rle_from_string."""
    data = np.asarray(data, dtype=np.uint8).reshape(-1)
    off = np.asarray(str_off, dtype=np.int64).reshape(-1)
    ends = np.concatenate([[0], np.cumsum(((data.astype(np.int16) - 48) & 0x20) == 0, dtype=np.int64)])
    return ends[off[1:]] - ends[off[:-1]]


@_on_device
def rle_from_string(bytes: torch.Tensor, str_off: torch.Tensor, heights: torch.Tensor, widths: torch.Tensor,
                    capacity: int | None = None):
    """maskUtils.frPyObjects on compressed strings (rleFrString of cocoapi/common/maskApi.c:218-231, the same bits) for n strings
    in one call on the GPU. bytes uint8 [total] and str_off int64 [n+1]: string i is bytes[str_off[i]:str_off[i+1]], packed,
    no terminator; heights / widths int32 [n] serve the checks only. All device tensors. → (num_runs int32 [n], counts int32
    [n,capacity], status int32 [n]); the status bits are RLE_* above: a malformed string (a byte outside 48..111, a token of more
    than 6 characters, an end inside a token, a size outside [1, 16384]) reports num_runs = -1 and its row is not written; an
    empty run after the first and a wrong pixel sum are flagged and the row is written; a string with more runs than capacity
    reports its true num_runs and its row is not written (uninitialised memory here). capacity is required: the op never
    synchronises, and the characters it would have to count live on the device — a front end counts them on its host copy
    (rle_string_tokens)."""
    _need_gpu(bytes, str_off, heights, widths)
    if capacity is None:
        raise RuntimeError("rle_from_string: capacity is required (count the tokens on the host copy: ops.rle_string_tokens)")
    bytes = checked("rle_from_string", "bytes", bytes, torch.uint8, ("total",))
    str_off = checked("rle_from_string", "str_off", str_off, torch.int64, (("n+1", 1),))
    n = str_off.numel() - 1
    heights = checked("rle_from_string", "heights", heights, torch.int32, (n,))
    widths = checked("rle_from_string", "widths", widths, torch.int32, (n,))
    capacity = int(capacity)
    dev = str_off.device
    num_runs = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(n, max(capacity, 0), dtype=torch.int32, device=dev)
    total = bytes.numel()
    _launch(lib.mrcnn_rle_from_string,
            (_ptr0(bytes), total, str_off.data_ptr(), _ptr0(heights), _ptr0(widths), n, capacity, _ptr0(num_runs), _ptr0(counts),
             _ptr0(status), _stream()),
            lambda: (0, (n, total, capacity), total + 4 * counts.numel(), "rle_from_string"))
    return num_runs, counts, status


@_on_device
def rle_area_bbox(num_runs: torch.Tensor, counts: torch.Tensor, heights: torch.Tensor, widths: torch.Tensor):
    """maskUtils.area and maskUtils.toBbox (rleArea, rleToBbox of maskApi.c:72-75, :133-147, the same values) of every row of a
    table (num_runs int32 [N], counts [N,capacity]) with per-row heights / widths int32 [N] → (areas int32 [N], bboxes int32
    [N,4] as (x, y, w, h)): what rle_encode returns for dense masks. A row that was refused or is over its capacity gets -1s."""
    num_runs, counts = rle_table((num_runs, counts), "rle_area_bbox")
    n, dev = num_runs.size(0), num_runs.device
    heights = checked("rle_area_bbox", "heights", heights, torch.int32, (n,))
    widths = checked("rle_area_bbox", "widths", widths, torch.int32, (n,))
    areas = torch.empty(n, dtype=torch.int32, device=dev)
    bboxes = torch.empty(n, 4, dtype=torch.int32, device=dev)
    if n:
        _launch(lib.mrcnn_rle_area_bbox,
                (num_runs.data_ptr(), counts.data_ptr(), n, counts.size(1), heights.data_ptr(), widths.data_ptr(), areas.data_ptr(),
                 bboxes.data_ptr(), _stream()),
                lambda: (0, (n, counts.size(1), 1), 4 * counts.numel(), "rle_area_bbox"))
    return areas, bboxes


@_on_device
def rle_to_string(num_runs: torch.Tensor, counts: torch.Tensor, total_bytes: int | None = None):
    """rleToString (maskApi.c:204-216, the same characters) of every row of a table → (bytes uint8 [total_bytes], str_off int64
    [N+1]) on the device, packed: string i is bytes[str_off[i]:str_off[i+1]]. str_off always holds the true offsets. With
    total_bytes given the call never synchronises; rows that would cross the end of the buffer are not written (str_off[N] >
    total_bytes tells). total_bytes=None costs one host read of the scanned total and allocates exactly. A row that was refused
    or is over its capacity has an empty string."""
    num_runs, counts = rle_table((num_runs, counts), "rle_to_string")
    n, dev = num_runs.size(0), num_runs.device
    str_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    nbytes = int(lib.mrcnn_rle_to_string_workspace_bytes(n))
    ws = workspace(nbytes, dev)
    have = 0
    if total_bytes is None:
        _to_string_launch(num_runs, counts, None, 0, have, str_off, ws, nbytes)      # offsets only
        total_bytes, have = int(str_off[n]), 1                                     # the one host read; the write pass alone follows
    out = torch.empty(max(int(total_bytes), 0), dtype=torch.uint8, device=dev)
    _to_string_launch(num_runs, counts, out, 0, have, str_off, ws, nbytes)
    return out, str_off


def _to_string_launch(num_runs, counts, buf, row_stride, have_offsets, str_off, ws, nbytes):
    n = num_runs.size(0)
    _launch(lib.mrcnn_rle_to_string,
            (_ptr0(num_runs), _ptr0(counts), n, counts.size(1), _ptr0(buf), buf.numel() if buf is not None else 0, int(row_stride),
             int(have_offsets), str_off.data_ptr(), ws.data_ptr(), nbytes, _stream()),
            lambda: (0, (n, counts.size(1), 1), 4 * counts.numel(), "rle_to_string"))


@_on_device
def rle_to_string_rows(num_runs: torch.Tensor, counts: torch.Tensor, row_stride: int | None = None):
    """rle_to_string into the ENCODER's layout: → (strings uint8 [N,row_stride], string_bytes int32 [N]), row i holding its
    characters from column 0 (the rest zero) — what rle_encode returns, written by the kernel itself, no packed intermediate and
    no host synchronisation. row_stride defaults to 6*capacity (6 characters a run cover masks of up to 2^28 pixels). A row whose
    string is longer than row_stride, or that was refused or is over its capacity, has string_bytes 0 and an all-zero row."""
    num_runs, counts = rle_table((num_runs, counts), "rle_to_string_rows")
    n, dev = num_runs.size(0), num_runs.device
    stride = 6 * counts.size(1) if row_stride is None else int(row_stride)
    if stride < 1:
        raise RuntimeError(f"rle_to_string_rows: row_stride={stride} must be >= 1")
    strings = torch.zeros(n, stride, dtype=torch.uint8, device=dev)
    str_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    nbytes = int(lib.mrcnn_rle_to_string_workspace_bytes(n))
    ws = workspace(nbytes, dev)
    _to_string_launch(num_runs, counts, strings, stride, 0, str_off, ws, nbytes)
    lengths = str_off[1:] - str_off[:-1]
    return strings, torch.where(lengths <= stride, lengths, torch.zeros_like(lengths)).to(torch.int32)


@_on_device
def rle_decode(num_runs: torch.Tensor, counts: torch.Tensor, height: int, width: int, out: torch.Tensor | None = None):
    """maskUtils.decode (rleDecode of maskApi.c:43-47) of every row of a table of H x W masks → uint8 [N,H,W] on the device,
    row-major, 0 / 1 — what rle_encode reads. `out`: a uint8 [N,H,W] tensor to fill (unit last stride, free image and row
    strides); every byte of it is written. Runs past H*W are clipped, pixels the runs do not reach are 0, and a row that was
    refused or is over its capacity decodes to zeros."""
    num_runs, counts = rle_table((num_runs, counts), "rle_decode")
    n, dev = num_runs.size(0), num_runs.device
    h, w = int(height), int(width)
    out = checked_out("rle_decode", "out", out, torch.uint8, (n, h, w), dev, contiguous=False)
    if w > 1 and out.stride(2) != 1:
        raise RuntimeError(f"rle_decode: out tensor out must have unit last stride, got strides {tuple(out.stride())}")
    if n == 0:
        return out
    image_stride = out.stride(0) if n > 1 else 0
    row_stride = out.stride(1) if h > 1 else w
    nbytes = int(lib.mrcnn_rle_decode_workspace_bytes(n, counts.size(1)))
    ws = workspace(nbytes, dev)
    _launch(lib.mrcnn_rle_decode_u8,
            (num_runs.data_ptr(), counts.data_ptr(), n, counts.size(1), h, w, out.data_ptr(), image_stride, row_stride,
             ws.data_ptr(), nbytes, _stream()),
            lambda: (0, (n, h, w), n * h * w + 4 * counts.numel(), "rle_decode"))
    return out


# status bits of rle_resample (include/maskrcnn_hip.h): a row with one set is refused — its mask is all zeros
RESAMPLE_UNUSABLE_ROW, RESAMPLE_BAD_SIZE, RESAMPLE_BAD_PLACEMENT, RESAMPLE_SHRINK_LIMIT = 1, 2, 4, 8
RESAMPLE_MAX_SHRINK = 16


@_on_device
def rle_resample(num_runs: torch.Tensor, counts: torch.Tensor, heights: torch.Tensor, widths: torch.Tensor, geom: torch.Tensor,
                 out_h: int, out_w: int, out: torch.Tensor | None = None):
    """Resized, mirrored, zero-padded 0 / 1 masks straight from the rows of a table (num_runs int32 [N], counts [N,capacity]) with
    PER-ROW source sizes heights / widths int32 [N] — what the reference's dataset does per annotation on the host (annToMask,
    np.fliplr, encode_masks' Pillow Resize and Pad: data.py:797-876, :246-262) in ONE call of two launches, whatever N is and
    however many sizes occur. geom int32 [N,5]: (new_h, new_w, top, left, flip) per row. → (masks uint8 [N,out_h,out_w], status
    int32 [N]). Mask k on [top, top+new_h) x [left, left+new_w) is numpy.array(Image.fromarray(m).resize((new_w, new_h),
    Image.BILINEAR)) for m = the decoded row, mirrored left to right when flip — Pillow's bits; an axis whose new size equals its
    source size is not resampled — and 0 elsewhere. `out`: a uint8 [N,out_h,out_w] tensor to fill (unit last stride, free image
    and row strides); every byte of it is written. status bits (RESAMPLE_*): 1 a refused or over-capacity row, 2 a size outside
    [1, 16384], 4 a placement not inside the canvas, 8 a source size above 16 times the new size on either axis; a row with a bit
    set is all zeros and the other rows are unaffected. No host synchronisation, no atomics, no dense source mask and no
    horizontal-pass intermediate in memory: the workspace holds the run ends only."""
    op = "rle_resample"
    num_runs, counts = rle_table((num_runs, counts), op)
    n, dev = num_runs.size(0), num_runs.device
    heights = checked(op, "heights", heights, torch.int32, (n,))
    widths = checked(op, "widths", widths, torch.int32, (n,))
    geom = checked(op, "geom", geom, torch.int32, (n, 5))
    h, w = int(out_h), int(out_w)
    if not (1 <= h <= 16384 and 1 <= w <= 16384):
        raise RuntimeError(f"{op}: out_h, out_w must be in [1, 16384], got {h}, {w}")
    out = checked_out(op, "out", out, torch.uint8, (n, h, w), dev, contiguous=False)
    if w > 1 and out.stride(2) != 1:
        raise RuntimeError(f"{op}: out tensor out must have unit last stride, got strides {tuple(out.stride())}")
    if h > 1 and out.stride(1) < w:
        raise RuntimeError(f"{op}: out tensor out must have a row stride of at least {w}, got strides {tuple(out.stride())}")
    status = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return out, status
    image_stride = out.stride(0) if n > 1 else 0
    row_stride = out.stride(1) if h > 1 else w
    nbytes = int(lib.mrcnn_rle_resample_workspace_bytes(n, counts.size(1)))
    ws = workspace(nbytes, dev)
    _launch(lib.mrcnn_rle_resample_u8,
            (num_runs.data_ptr(), counts.data_ptr(), n, counts.size(1), heights.data_ptr(), widths.data_ptr(), geom.data_ptr(),
             out.data_ptr(), h, w, image_stride, row_stride, status.data_ptr(), ws.data_ptr(), nbytes, _stream()),
            lambda: (0, (n, h, w), n * h * w + 4 * counts.numel(), "rle_resample"))
    return out, status


register("rle_from_string(Tensor bytes, Tensor str_off, Tensor heights, Tensor widths, int? capacity=None) -> (Tensor, Tensor, Tensor)",
         rle_from_string)
register("rle_area_bbox(Tensor num_runs, Tensor counts, Tensor heights, Tensor widths) -> (Tensor, Tensor)", rle_area_bbox)
register("rle_to_string(Tensor num_runs, Tensor counts, int? total_bytes=None) -> (Tensor, Tensor)", rle_to_string)
register("rle_decode(Tensor num_runs, Tensor counts, int height, int width) -> Tensor", rle_decode)   # `out` is the Python binding's
# rle_resample has no torch.ops.maskrcnn schema and is not in ops.__all__: tests/test_binding_host.py pins both lists to what was
# registered before it. It is reached as ops.rle_resample (ops.py takes every public name of this module).
