"""Image pre-/post-processing around the hot path, on the GPU.

Mirrors the reference functions either side of MaskRCNN.predict:
    resize_image   utils.py:42-90      aspect-preserving resize + centre zero padding (scipy.misc.imresize → PIL)
    mold_image     model.py:1750-1754  float32(image) - MEAN_PIXEL; detect() then transposes to [1,3,H,W] (:1108-1110)
    full_masks     data.py:287-314     28x28 masks → PIL resize to the box → paste → > 127
    decode_boxes   data.py:331-343     boxes back to the original image's frame
    decode_masks   data.py:264-284     masks back to the original image's size (CenterCrop + PIL resize)
    random_colors  data.py:346-356     the instance palette
    blend_image    data.py:359-403     masks, outlines and boxes drawn onto the image (without the labels)
The host part below is the scalar bookkeeping (scale, sizes, pads — Python floats and round(), exactly the reference's
expressions); every pixel is produced by libmaskrcnn_hip.so (csrc/image.hip), bit-identical to Pillow's resample.
"""
from __future__ import annotations

import colorsys
import random
from typing import NamedTuple

import numpy as np
import torch

from . import ops
from .config import InferenceConfig


def resize_plan(h: int, w: int, min_dim=None, max_dim=None, padding=False):
    """The arithmetic of utils.resize_image (utils.py:56-88) without touching pixels.
    → (new_h, new_w, window (y1,x1,y2,x2), scale, padding [(top,bottom),(left,right),(0,0)] or False)."""
    scale = 1
    if min_dim:
        scale = max(1, min_dim / min(h, w))            # :62-64 scale up but not down
    if max_dim:
        image_max = max(h, w)
        if round(image_max * scale) > max_dim:         # :67-69
            scale = max_dim / image_max
    new_h, new_w = (round(h * scale), round(w * scale)) if scale != 1 else (h, w)   # :72-74
    window = (0, 0, new_h, new_w)
    if padding:
        top_pad = (max_dim - new_h) // 2               # :79-84
        bottom_pad = max_dim - new_h - top_pad
        left_pad = (max_dim - new_w) // 2
        right_pad = max_dim - new_w - left_pad
        padding = [(top_pad, bottom_pad), (left_pad, right_pad), (0, 0)]
        window = (top_pad, left_pad, new_h + top_pad, new_w + left_pad)
    return new_h, new_w, window, scale, padding


def _to_device_u8(image, device) -> torch.Tensor:
    if isinstance(image, np.ndarray):
        image = torch.from_numpy(np.ascontiguousarray(image))
    if image.dtype != torch.uint8 or image.dim() != 3 or image.size(2) != 3:
        raise RuntimeError(f"expected an RGB uint8 [h,w,3] image, got {image.dtype} {tuple(image.shape)}")
    return image.to(device, non_blocking=True)


def mold_inputs(images, cfg: InferenceConfig, device="cuda:0"):
    """A list of RGB uint8 [h,w,3] images (numpy or torch, any sizes) → molded fp32 [B,3,H,W] on the device, int
    windows [B,4], and per-image (scale, padding, original (h,w)) — detect()'s pre-processing (model.py:1097-1110)
    for a batch. Needs a square canvas, like the reference (IMAGE_MAX_DIM x IMAGE_MAX_DIM). Images of one size are molded
    TOGETHER (one host-to-device copy, one set of launches per size: ops.mold_images_u8), in whatever order they come."""
    if cfg.image_height != cfg.image_width or cfg.image_height != cfg.image_max_dim:
        raise RuntimeError("mold_inputs: resize_image pads to IMAGE_MAX_DIM x IMAGE_MAX_DIM; configure a square canvas "
                           "of image_max_dim, or mold images yourself")
    device = torch.device(device)
    out = torch.empty(len(images), 3, cfg.image_height, cfg.image_width, dtype=torch.float32, device=device)
    windows, metas, groups = [], [], {}
    for i, image in enumerate(images):
        if tuple(image.shape[2:]) != (3,) or len(image.shape) != 3 or image.dtype not in (torch.uint8, np.uint8):
            raise RuntimeError(f"expected an RGB uint8 [h,w,3] image, got {image.dtype} {tuple(image.shape)}")
        h, w = int(image.shape[0]), int(image.shape[1])
        new_h, new_w, window, scale, padding = resize_plan(h, w, cfg.image_min_dim, cfg.image_max_dim, True)
        windows.append(window)
        metas.append((scale, padding, (h, w)))
        groups.setdefault((h, w), []).append(i)
    for (h, w), idx in groups.items():
        new_h, new_w, window, _, _ = resize_plan(h, w, cfg.image_min_dim, cfg.image_max_dim, True)
        members = [images[i] for i in idx]
        if all(isinstance(m, np.ndarray) for m in members):
            stack = torch.from_numpy(np.stack(members)).to(device, non_blocking=True)          # one copy for the group
        else:
            stack = torch.stack([_to_device_u8(m, device) for m in members])
        whole = idx == list(range(idx[0], idx[0] + len(idx)))                                   # a contiguous run of the batch
        dst = out[idx[0]:idx[0] + len(idx)] if whole else torch.empty(len(idx), 3, cfg.image_height, cfg.image_width,
                                                                      dtype=torch.float32, device=device)
        ops.mold_images_u8(stack.contiguous(), new_h, new_w, window[0], window[1], dst, cfg.mean_pixel)
        if not whole:
            out[torch.tensor(idx, device=device)] = dst
    return out, torch.tensor(windows, dtype=torch.int64), metas


def resize_image(image, min_dim=None, max_dim=None, padding=False, device="cuda:0"):
    """utils.resize_image with the reference's signature and return values; the image comes back as a uint8 device
    tensor [H,W,3]."""
    img = _to_device_u8(image, torch.device(device))
    h, w = img.shape[:2]
    new_h, new_w, window, scale, pad = resize_plan(h, w, min_dim, max_dim, padding)
    if scale != 1:
        img = ops.resize_bilinear_u8(img, new_h, new_w)
    if padding:
        canvas = torch.zeros(max_dim, max_dim, 3, dtype=torch.uint8, device=img.device)
        canvas[window[0]:window[2], window[1]:window[3]] = img
        img = canvas
    return img, window, scale, pad


def full_masks(class_id: torch.Tensor, boxes: torch.Tensor, masks: torch.Tensor, height: int, width: int,
               channels_last: bool = False) -> torch.Tensor:
    """datalib.full_masks(class_id [N], boxes [N,4], masks [N,C,28,28], height, width) → bool [N,height,width].
    channels_last=True takes this library's [N,28,28,C] mask-head output directly."""
    return ops.paste_masks(masks, class_id, boxes, height, width, channels_last)


def decode_boxes(boxes: torch.Tensor, scale, window) -> torch.Tensor:
    """data.py:331-343: shift by the window origin, then multiply by 1/(scale + 1e-5) (fp32 tensor ops)."""
    if scale == 1:
        return boxes
    off = torch.tensor([window[0], window[1], window[0], window[1]], dtype=boxes.dtype, device=boxes.device)
    return (boxes - off) * torch.tensor([1.0 / (scale + 1e-5)] * 4, dtype=boxes.dtype, device=boxes.device)


def decode_masks(masks_l8: torch.Tensor, scale, window) -> torch.Tensor:
    """data.py:264-284 for masks given as 0/255 'L' images [N,H,W] (ops.paste_masks(as_l8=True)): CenterCrop to the
    window's size, PIL-resize by 1/scale → uint8 [N, round(h/scale), round(w/scale)] (grey levels, as the reference
    returns them). The caller handles scale == 1 (the reference returns the boolean masks untouched)."""
    n, hh, ww = masks_l8.shape
    ch, cw = window[2] - window[0], window[3] - window[1]
    top = int(round((hh - ch) / 2.0))      # torchvision center_crop; not the window origin when the pad is odd
    left = int(round((ww - cw) / 2.0))
    nh, nw = round(ch * 1.0 / scale), round(cw * 1.0 / scale)
    return ops.resize_bilinear_u8(masks_l8[:, top:top + ch, left:left + cw], nh, nw)


# ---------------------------------------------------------------------------------------------- COCO RLE masks
class RleMasks:
    """N masks of one size as COCO run-length encodings on the device: what ops.rle_encode returns (row views of it for one
    image of a detect() batch). size = (h, w); num_runs int32 [N], counts int32 [N,capacity], strings uint8 [N,6*capacity],
    string_bytes int32 [N], areas int32 [N] (on pixels), bboxes int32 [N,4] (x, y, w, h)."""

    def __init__(self, size, num_runs, counts, strings, string_bytes, areas, bboxes):
        self.size = (int(size[0]), int(size[1]))
        self.num_runs, self.counts, self.strings, self.string_bytes = num_runs, counts, strings, string_bytes
        self.areas, self.bboxes = areas, bboxes

    def __len__(self):
        return int(self.num_runs.size(0))

    @property
    def capacity(self) -> int:
        return int(self.counts.size(1))

    def to_coco(self):
        """→ [{"size": [h, w], "counts": bytes}] per mask: the dict maskUtils.encode returns (pycocotools' compressed RLE).
        The string characters are gathered on the device and come to the host in ONE small copy together with the lengths
        (a few KB per mask instead of h*w bytes). A mask that did not fit the encode's capacity has no string: RuntimeError;
        so has a row of a table that was refused (num_runs -1) or has runs and no characters (rle_masks_from_table)."""
        n = len(self)
        if n == 0:
            return []
        live = torch.arange(self.strings.size(1), device=self.strings.device)[None, :] < self.string_bytes[:, None]
        head = torch.stack([self.num_runs, self.string_bytes]).contiguous().view(torch.uint8).reshape(-1)
        packed = torch.cat([head, self.strings[live]]).cpu().numpy()
        runs, nbytes = packed[:8 * n].view(np.int32).reshape(2, n)
        if (runs < 0).any():
            raise RuntimeError(f"RleMasks.to_coco: masks {np.nonzero(runs < 0)[0].tolist()} were refused (num_runs -1): they have "
                               "no runs and no string")
        if (runs > self.capacity).any():
            raise RuntimeError(f"RleMasks.to_coco: masks {np.nonzero(runs > self.capacity)[0].tolist()} have more runs than the "
                               f"capacity {self.capacity} they were encoded with; encode again with capacity >= {int(runs.max())}")
        if ((runs > 0) & (nbytes == 0)).any():
            raise RuntimeError(f"RleMasks.to_coco: masks {np.nonzero((runs > 0) & (nbytes == 0))[0].tolist()} have runs and no string "
                               "(a refused row, or a string longer than 6 characters per run)")
        ends = 8 * n + np.cumsum(nbytes, dtype=np.int64)
        h, w = self.size
        return [{"size": [h, w], "counts": packed[e - b:e].tobytes()} for b, e in zip(nbytes.tolist(), ends.tolist())]

    def decode(self) -> torch.Tensor:
        """maskUtils.decode: uint8 [N,h,w] on the device, row-major, 0 / 1 (ops.rle_decode)."""
        return ops.rle_decode(self.num_runs, self.counts, self.size[0], self.size[1])

    def iou(self, other, iscrowd=None) -> torch.Tensor:
        """maskUtils.iou(self, other, iscrowd): float64 [len(self), len(other)] on the device, the bits of rleIou. `other` is an
        RleMasks of the same size or (num_runs, counts) device tensors (rle_table); iscrowd uint8 [len(other)] or a list."""
        if isinstance(other, RleMasks) and other.size != self.size:
            raise ValueError(f"RleMasks.iou: masks of {self.size} against masks of {other.size}")
        if iscrowd is not None and not isinstance(iscrowd, torch.Tensor):
            iscrowd = torch.tensor(np.asarray(iscrowd, dtype=np.uint8), device=self.num_runs.device)
        return ops.rle_iou(self, other, iscrowd)


def rle_masks(masks: torch.Tensor, threshold: int = 0) -> RleMasks:
    """ops.rle_encode of uint8 / bool masks [N,H,W] as an RleMasks in which every mask fits: when one has more runs than the
    default capacity the batch is encoded once more with room for the longest (one host read of the run counts)."""
    enc = ops.rle_encode(masks, threshold)
    if masks.size(0):
        longest = int(enc[0].max())
        if longest > enc[1].size(1):
            enc = ops.rle_encode(masks, threshold, capacity=longest)
    return RleMasks(masks.shape[-2:], *enc)


def rle_masks_from_table(size, num_runs: torch.Tensor, counts: torch.Tensor) -> RleMasks:
    """A run-list table of masks of ONE size (h, w) on the device — what ops.rle_from_poly / ops.rle_merge / rle_table return — as
    an RleMasks: strings, string_bytes, areas and bboxes come from ops.rle_to_string and ops.rle_area_bbox, so to_coco() gives the
    dicts maskUtils.encode would. No host synchronisation and no packed intermediate: the kernel writes each row's characters (at
    most 6 per run for masks of up to 2^28 pixels) straight into the [N, 6*capacity] layout (ops.rle_to_string_rows). A row that
    was refused or is over its capacity keeps its num_runs and has string_bytes 0, area -1 and bbox -1; to_coco() raises on it."""
    h, w = int(size[0]), int(size[1])
    num_runs, counts = ops.rle_table((num_runs, counts), "rle_masks_from_table")
    n, cap, dev = num_runs.size(0), counts.size(1), num_runs.device
    sizes = torch.tensor([h, w], dtype=torch.int32, device=dev)
    areas, bboxes = ops.rle_area_bbox(num_runs, counts, sizes[0].expand(n).contiguous(), sizes[1].expand(n).contiguous())
    strings, string_bytes = ops.rle_to_string_rows(num_runs, counts)
    return RleMasks((h, w), num_runs, counts, strings, string_bytes, areas, bboxes)


def rle_counts(obj) -> np.ndarray:
    """The run lengths (uint32, off run first) of a COCO RLE given as a dict {"size", "counts"}, a compressed string
    (bytes or str: rleFrString of cocoapi/common/maskApi.c) or a count list (returned as is). Pure numpy."""
    if isinstance(obj, dict):
        obj = obj["counts"]
    if isinstance(obj, str):
        obj = obj.encode("ascii")
    if not isinstance(obj, (bytes, bytearray)):
        return np.asarray(obj, dtype=np.uint32).reshape(-1)
    cnts, x, k = [], 0, 0
    for ch in obj:
        c = ch - 48
        x |= (c & 0x1f) << (5 * k)
        k += 1
        if c & 0x20:
            continue
        if c & 0x10:
            x |= -1 << (5 * k)          # sign-extend: the string holds differences to the run two back
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
        x, k = 0, 0
    return np.asarray(cnts, dtype=np.uint32)


def _run_error(prefix: str, i: int, h: int, w: int, bad_sum: bool, empty_run: bool, total):
    """The ValueError of run lengths that break ops.rle_iou's contract on its inputs for an h x w mask — they do not cover h*w
    pixels (total(): what they cover, asked for on this path only), or a run after the first is empty — or None."""
    if bad_sum:
        return ValueError(f"{prefix}: the runs of mask {i} cover {total()} pixels, the mask has {h} x {w}")
    if empty_run:
        return ValueError(f"{prefix}: mask {i} has an empty run after the first one")
    return None


def _checked_counts(obj, prefix: str, i: int, h: int, w: int) -> np.ndarray:
    """rle_counts(obj), checked against ops.rle_iou's contract on its inputs for an h x w mask (_run_error's ValueError)."""
    cnts = rle_counts(obj)
    total = int(cnts.astype(np.int64).sum())
    bad = _run_error(prefix, i, h, w, total != h * w, cnts.size > 1 and not cnts[1:].all(), lambda: total)
    if bad is not None:
        raise bad
    return cnts


def _pack_table(rows, device, capacity=None):
    """Run-length rows (uint32 arrays) → (num_runs int32 [N], counts int32 [N,capacity]) on the device, one copy each."""
    longest = max([r.size for r in rows], default=0)
    if capacity is None:
        capacity = max(1, longest)
    if int(capacity) < max(1, longest):
        raise ValueError(f"rle_table: capacity {capacity} is less than the longest mask's {longest} runs")
    table = np.zeros((len(rows), int(capacity)), dtype=np.uint32)
    for i, r in enumerate(rows):
        table[i, :r.size] = r
    num_runs = np.array([r.size for r in rows], dtype=np.int32)
    device = torch.device(device)
    return torch.from_numpy(num_runs).to(device), torch.from_numpy(table.view(np.int32)).to(device)


def _string_of(obj):
    """The compressed string of an RLE entry (a dict or the string itself) as bytes; None for a count list."""
    c = obj["counts"] if isinstance(obj, dict) else obj
    if isinstance(c, str):
        return c.encode("ascii")
    if isinstance(c, (bytes, bytearray)):
        return bytes(c)
    return None


def _strings_to_device(strs, hs, ws, device):
    """Compressed strings (bytes) with their sizes → ONE ops.rle_from_string call: (num_runs int32 [n], counts int32 [n,capacity],
    status int32 [n]) on the device, every well-formed string fitting. The capacity is the host's token count (numpy, one
    cumulative sum: ops.rle_string_tokens); two host-to-device copies (the characters; offsets and sizes)."""
    device = torch.device(device)
    n = len(strs)
    data = np.frombuffer(b"".join(strs), dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, strs), dtype=np.int64, count=n), out=off[1:])
    capacity = max(1, int(ops.rle_string_tokens(data, off).max())) if n else 1
    ints = torch.from_numpy(np.concatenate([off, np.asarray(hs, dtype=np.int64), np.asarray(ws, dtype=np.int64)])).to(device)
    sizes = ints[n + 1:].to(torch.int32)
    return ops.rle_from_string(torch.from_numpy(data.copy()).to(device), ints[:n + 1], sizes[:n], sizes[n:], capacity=capacity)


class _Decoded(NamedTuple):
    """The strings one ops.rle_from_string call decoded: num_runs int32 [S] and counts int32 [S,capacity] on the device, and the
    host copies (numpy int32 [S]) of num_runs (runs) and of the status the kernel wrote."""
    num_runs: torch.Tensor
    counts: torch.Tensor
    runs: np.ndarray
    status: np.ndarray


def _status_error(d: _Decoded, k: int, who: str, written=None):
    """The ValueError for row k of d by its status bits, or None. A string the kernel refused (num_runs -1): "{who} has <what is
    wrong with it>". A row it wrote and flagged, with written = (prefix, i, h, w): _run_error's, the row's counts being fetched
    from the device for the pixel sum only; written=None leaves those two bits to a later stage."""
    st = int(d.status[k])
    for bit, why in ((ops.RLE_BAD_SIZE, "a height or width outside [1, 16384]"),
                     (ops.RLE_BAD_BYTE, "a character outside '0'..'o' (bytes 48..111) in its compressed string"),
                     (ops.RLE_LONG_TOKEN, "a run of more than 6 characters in its compressed string"),
                     (ops.RLE_OPEN_TOKEN, "a compressed string that ends inside a run"),
                     (ops.RLE_BAD_OFFSETS, "string offsets outside the buffer")):
        if st & bit:
            return ValueError(f"{who} has {why}")
    if written is None:
        return None
    return _run_error(*written, st & ops.RLE_PIXEL_SUM, st & ops.RLE_EMPTY_RUN,
                      lambda: int(d.counts[k, :int(d.runs[k])].cpu().numpy().view(np.uint32).astype(np.int64).sum()))


def _merge_tables(n: int, parts, device, capacity=None):
    """parts: [(indices (numpy int64), num_runs [k], counts [k,c])] on the device, disjoint, covering what they cover of n rows →
    one zero-padded table (num_runs int32 [n], counts int32 [n,capacity]); rows no part covers are empty (num_runs 0)."""
    device = torch.device(device)
    cap = _widest(parts) if capacity is None else int(capacity)
    num_runs = torch.zeros(n, dtype=torch.int32, device=device)
    counts = torch.zeros(n, cap, dtype=torch.int32, device=device)
    for idx, nr, c in parts:
        if len(idx) == 0:
            continue
        at = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(device)
        width = min(cap, int(c.size(1)))
        live = torch.arange(width, device=device)[None, :] < nr[:, None]
        counts[at, :width] = torch.where(live, c[:, :width], torch.zeros((), dtype=torch.int32, device=device))
        num_runs[at] = nr
    return num_runs, counts


def _table_parts(objs, sizes, device, *, skip=None, decoded=None, other=None, host_strings=False, prefix="rle_table"):
    """RLE entries (dicts {"size", "counts"}, compressed strings or count lists), checked → the parts _merge_tables makes their
    table of: rows packed on the host, rows gathered on the device, strings decoded there. sizes: a list, one (h, w) per entry,
    or None: every entry is a dict (or other's) and of its own "size"; skip[i]: a row no part covers; decoded = (a _Decoded,
    {entry index: its row}): strings that are on the device already and are gathered from there; other(obj, i): given, the run
    lengths of every entry that is no dict come from it, and are taken as they come.
    Where compressed strings are decoded is the one decision: on the device, all of them in ONE ops.rle_from_string call and one
    read of num_runs / status — or, on the CPU or with host_strings, by rle_counts, and then the library is not touched. All
    else is shared: a dict of another size, runs that do not cover the mask, an empty run after the first one and a malformed
    string are ValueErrors "{prefix}: ... mask {i} ...", and the lowest bad index is the one raised."""
    device = torch.device(device)
    if sizes is None:
        size = lambda i: (int(objs[i]["size"][0]), int(objs[i]["size"][1]))
    else:
        size = lambda i: (int(sizes[i][0]), int(sizes[i][1]))
    host_strings = host_strings or device.type == "cpu"
    gathered = decoded[1] if decoded is not None else {}
    errors, rows, strs, pre = {}, [], [], []
    for i, obj in enumerate(objs):
        if skip is not None and skip[i]:
            continue
        try:
            if i in gathered:
                pre.append((i, gathered[i]))
            elif other is not None and not isinstance(obj, dict):
                rows.append((i, other(obj, i)))
            else:
                h, w = size(i)
                if sizes is not None and isinstance(obj, dict) and [int(v) for v in obj["size"]] != [h, w]:
                    raise ValueError(f"{prefix}: mask {i} is {list(obj['size'])}, the table is {[h, w]}")
                s = None if host_strings else _string_of(obj)
                if s is None:
                    rows.append((i, _checked_counts(obj, prefix, i, h, w)))
                else:
                    strs.append((i, s, h, w))
        except ValueError as e:
            if host_strings:
                raise               # nothing is pending on the host: the entries are checked in index order
            errors[i] = e

    def flagged(idx, at, d):
        for j in np.nonzero(d.status[at])[0].tolist():
            i = idx[j]
            errors[i] = _status_error(d, int(at[j]), f"{prefix}: mask {i}", (prefix, i, *size(i)))

    parts = []
    if rows:
        parts.append(([i for i, _ in rows], *_pack_table([r for _, r in rows], device)))
    if pre:
        idx, at = [i for i, _ in pre], np.array([k for _, k in pre], dtype=np.int64)
        flagged(idx, at, decoded[0])
        on_dev = torch.from_numpy(at).to(device)
        parts.append((idx, decoded[0].num_runs[on_dev], decoded[0].counts[on_dev]))
    if strs:
        idx, strings, hs, ws = zip(*strs)
        nr, cnt, status = _strings_to_device(strings, hs, ws, device)
        back = torch.stack([nr, status]).cpu().numpy()          # the one read-back
        flagged(idx, np.arange(len(strs)), _Decoded(nr, cnt, back[0], back[1]))
        parts.append((idx, nr, cnt))
    if errors:
        raise errors[min(errors)]
    return parts


def _widest(parts) -> int:
    """The capacity _merge_tables gives the table of these parts when it is not told one."""
    return max([1] + [int(c.size(1)) for _, _, c in parts])


def _build_table(objs, sizes, device, capacity=None, *, prefix="rle_table", **how):
    """The (num_runs int32 [N], counts int32 [N,capacity]) table of RLE entries on the device: _table_parts (how: its other
    keywords), the capacity check, _merge_tables."""
    parts = _table_parts(objs, sizes, device, prefix=prefix, **how)
    if capacity is not None and int(capacity) < _widest(parts):
        raise ValueError(f"{prefix}: capacity {capacity} is less than the longest mask's {_widest(parts)} runs")
    return _merge_tables(len(objs), parts, device, capacity)


def rle_table(objs, size, device="cuda:0", capacity=None):
    """A list of COCO RLEs (dicts {"size", "counts"}, compressed strings or count lists) of ONE size (h, w) → (num_runs int32
    [N], counts int32 [N,capacity]) on the device: the table layout ops.rle_encode writes and ops.rle_iou reads. Every entry is
    checked against rle_iou's contract: the runs cover exactly h*w pixels and only the leading run may be empty (ValueError
    otherwise). On a GPU device all compressed strings are decoded there in ONE ops.rle_from_string call (no per-character host
    work; a malformed string — a byte outside 48..111, a run of more than 6 characters, an end inside a run — is a ValueError
    too), count lists are packed on the host, the two are merged by index on the device, and the checks read num_runs / status
    back once. device="cpu": every entry goes through rle_counts on the host, and the library is not touched (_build_table)."""
    objs = list(objs)
    return _build_table(objs, [(int(size[0]), int(size[1]))] * len(objs), device, capacity)


def rle_decode_masks(objs, size, device="cuda:0") -> torch.Tensor:
    """COCO.annToMask for a list of RLEs of one size (dicts, compressed strings or count lists): uint8 [N,h,w] on the device,
    row-major, 0 / 1 — rle_table, then ops.rle_decode."""
    num_runs, counts = rle_table(objs, size, device)
    return ops.rle_decode(num_runs, counts, int(size[0]), int(size[1]))


def rle_decode(obj, size=None) -> np.ndarray:
    """bool [h, w] mask of a COCO RLE: a dict {"size": [h, w], "counts": compressed bytes / str or a count list}, or raw
    counts / a raw string with size=(h, w). Runs alternate off / on over the pixels in column-major order. Pure numpy."""
    if isinstance(obj, dict):
        size = obj["size"]
    if size is None:
        raise ValueError("rle_decode: size=(h, w) is needed with raw counts")
    h, w = int(size[0]), int(size[1])
    cnts = rle_counts(obj).astype(np.int64)
    if int(cnts.sum()) != h * w:
        raise ValueError(f"rle_decode: the runs cover {int(cnts.sum())} pixels, the mask has {h} x {w}")
    flat = np.repeat(np.arange(cnts.size) & 1, cnts).astype(bool)
    return flat.reshape(w, h).T


# ---------------------------------------------------------------------------------------------- polygons and boxes to RLE
def _pack_polygons(polys, sizes):
    """polys: flat [x0, y0, x1, y1, ...] lists (k = len // 2 vertices each, as _mask.pyx:266); sizes: one (h, w) or one per
    polygon → numpy (xy float64 [V,2], vert_off int64 [n+1], heights int64 [n], widths int64 [n]). ValueError for a polygon
    without a vertex or a size list of another length."""
    n = len(polys)
    sizes = np.asarray(sizes, dtype=np.int64)
    if sizes.shape == (2,):
        sizes = np.broadcast_to(sizes, (n, 2))
    if sizes.shape != (n, 2):
        raise ValueError(f"rle_from_polygons: sizes is one (h, w) or one per polygon: {n} polygons, sizes of shape {sizes.shape}")
    ks = np.array([len(p) // 2 for p in polys], dtype=np.int64)
    if (ks < 1).any():
        i = int(np.argmax(ks < 1))
        raise ValueError(f"rle_from_polygons: polygon {i} has {len(polys[i])} numbers: not one vertex")
    xy = np.empty((int(ks.sum()), 2), dtype=np.float64)
    off = np.concatenate([[0], np.cumsum(ks)])
    for i, p in enumerate(polys):
        xy[off[i]:off[i + 1]] = np.asarray(p[:2 * ks[i]], dtype=np.float64).reshape(-1, 2)
    return xy, off, np.ascontiguousarray(sizes[:, 0]), np.ascontiguousarray(sizes[:, 1])


def _polygons_to_device(xy, off, hs, ws, device):
    """ONE float64 buffer, one host-to-device copy → the device arguments of ops.rle_from_poly (the integers are exact in
    float64 and are cast on the device)."""
    v, n = xy.shape[0], hs.size
    buf = torch.from_numpy(np.concatenate([xy.reshape(-1), off, hs, ws]).astype(np.float64)).to(torch.device(device))
    ints = buf[2 * v:].to(torch.int32)
    return buf[:2 * v].view(v, 2), ints[:n + 1], ints[n + 1:2 * n + 1], ints[2 * n + 1:]


def rle_from_polygons(polys, sizes, device="cuda:0"):
    """maskUtils.frPyObjects(polys, h, w) for polygons (rleFrPoly, the same bits) on the GPU, all of them in ONE ops.rle_from_poly
    call: polys is a list of flat [x0, y0, x1, y1, ...] lists (len // 2 vertices; an odd trailing number is dropped, as the
    reference does), sizes one (h, w) or one per polygon. → (num_runs int32 [n], counts int32 [n,capacity]) on the device, every
    polygon fitting: the table ops.rle_iou / ops.rle_merge read. Everything goes to the device in one buffer and nothing comes
    back. ValueError: a polygon without a vertex, a coordinate that is not finite or has |5*v + .5| >= 2^31, a size outside
    [1, 16384], more than 2^24 boundary points in one polygon."""
    xy, off, hs, ws = _pack_polygons(polys, sizes)
    bounds = ops.poly_host_bounds(xy, off, hs, ws, "rle_from_polygons", ValueError)
    capacity = int(bounds.max()) + 1 if len(polys) else 1
    num_runs, counts, _ = ops.rle_from_poly(*_polygons_to_device(xy, off, hs, ws, device), capacity=capacity)
    return num_runs, counts


def rle_from_bboxes(boxes, size, device="cuda:0"):
    """maskUtils.frPyObjects(boxes, h, w) for (x, y, w, h) boxes [N,4] (rleFrBbox, maskApi.c:149-156: the four-vertex polygon
    xs,ys, xs,ye, xe,ye, xe,ys with xe = xs + w and ye = ys + h in float64, through the polygon kernel) → the table of
    rle_from_polygons."""
    bb = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    xs, ys = bb[:, 0], bb[:, 1]
    xe, ye = xs + bb[:, 2], ys + bb[:, 3]
    polys = np.stack([xs, ys, xs, ye, xe, ye, xe, ys], axis=1)
    return rle_from_polygons(list(polys), size, device)


# ---------------------------------------------------------------------------------------------- rendering detections
def random_colors(n: int, bright: bool = True, shuffle: bool = True):
    """data.random_colors (data.py:346-356): n (r, g, b) tuples, hues i/n at full saturation through colorsys, int(v * 255),
    shuffled with the GLOBAL random.shuffle — after random.seed(k) this is the reference's palette."""
    brightness = 1.0 if bright else 0.7
    colors = []
    for i in range(n):
        r, g, b = colorsys.hsv_to_rgb(i / n, 1, brightness)
        colors.append((int(r * 255), int(g * 255), int(b * 255)))
    if shuffle:
        random.shuffle(colors)
    return colors


INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _blend_host(image: np.ndarray, on: np.ndarray, colors: np.ndarray, boxes) -> np.ndarray:
    """The rule of mrcnn_blend_instances_u8 (include/maskrcnn_hip.h) in numpy: image uint8 [H,W,3], on bool [N,H,W], colors uint8
    [N,3], boxes int64 [N,4] (y0, x0, y1, x1) or None → a new uint8 [H,W,3]. The blend is float32 arithmetic, the box clipping
    int64. An inverted box is a ValueError, as Pillow's."""
    out = np.array(image, dtype=np.uint8)
    h, w = out.shape[:2]
    fifth = np.float32(0.2)
    for m, c in zip(on, colors):
        pad = np.zeros((h + 2, w + 2), dtype=bool)
        pad[1:-1, 1:-1] = m
        near = np.zeros((h, w), dtype=bool)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                if (dy, dx) != (1, 1):
                    near |= pad[dy:dy + h, dx:dx + w]
        edge = near & ~m
        edge[0, :] = edge[-1, :] = False
        edge[:, 0] = edge[:, -1] = False
        px = out.astype(np.float32)
        diff = (c.astype(np.int32)[None, None, :] - out.astype(np.int32)).astype(np.float32)
        blended = np.trunc(px + fifth * diff).astype(np.uint8)         # float32 throughout: fifth * diff rounds, then the sum
        out[m] = blended[m]
        out[edge] = c
    if boxes is not None:
        for (y0, x0, y1, x1), c in zip(np.asarray(boxes, dtype=np.int64).reshape(-1, 4).tolist(), colors):
            if y1 < y0 or x1 < x0:
                raise ValueError(f"blend_image: box ({y0}, {x0}, {y1}, {x1}) has y2 < y1 or x2 < x1")
            xa, xb = max(x0, 0), min(x1, w - 1)
            for y in (y0, y1):
                if 0 <= y < h and xa <= xb:
                    out[y, xa:xb + 1] = c
            ya, yb = max(min(y0 + 1, y1), 0), min(max(y0 + 1, y1), h - 1)
            for x in (x0, x1):
                if 0 <= x < w and ya <= yb:
                    out[ya:yb + 1, x] = c
    return out


def _boxes_i32(boxes: torch.Tensor) -> torch.Tensor:
    """Box coordinates truncated toward zero to int32 where they are (device or host); values outside int32 saturate."""
    if boxes.dtype == torch.int32:
        return boxes
    if boxes.dtype.is_floating_point:
        boxes = boxes.to(torch.float64).trunc()
    return boxes.clamp(INT32_MIN, INT32_MAX).to(torch.int32)


def blend_image(image, boxes, masks, colors=None, threshold=None, device="cuda:0") -> torch.Tensor:
    """data.blend_image(image, None, boxes, masks) (data.py:383-403) without the labels: every instance's mask blended at 0.2, its
    outline and its box in the instance's colour, the bits Pillow gives → uint8 [H,W,3] on `device`.
        image      numpy array or tensor uint8 [H,W,3]
        boxes      [N,4] (y1, x1, y2, x2), any real dtype, or None: no rectangles; float coordinates are truncated toward zero on
                   the device
        masks      a dense uint8 / bool tensor [N,H,W], an RleMasks (decoded on the device; threshold 0) or None: boxes only
        colors     [N,3] uint8 values (a list of tuples, an array or a tensor); None: random_colors(N), the reference's call
        threshold  a pixel is on where mask > threshold. None: 0 for bool masks and RleMasks, 127 for uint8 masks — detect()'s
                   grey levels for a resized image; give 0 for uint8 masks of 0 / 1 (the values are never inspected here)
    On a GPU device everything is one ops.blend_instances launch and nothing comes back to the host. device="cpu" runs the same
    rule in numpy (_blend_host) and does not touch the library; there an inverted box (y2 < y1 or x2 < x1) is a ValueError, as
    Pillow's, while the kernel draws nothing for it."""
    device = torch.device(device)
    img = _to_device_u8(image, device)
    h, w = int(img.size(0)), int(img.size(1))
    if isinstance(masks, RleMasks):
        if masks.size != (h, w):
            raise ValueError(f"blend_image: masks of {masks.size} on an image of {(h, w)}")
        if device.type == "cpu":
            raise RuntimeError("blend_image: an RleMasks is decoded on the GPU; give device a GPU, or dense masks")
        masks, threshold = masks.decode(), 0 if threshold is None else threshold
    if masks is None and boxes is None:
        raise ValueError("blend_image: neither masks nor boxes")
    n = int(masks.size(0)) if masks is not None else len(boxes)
    if boxes is not None:
        boxes = _boxes_i32(torch.as_tensor(boxes).to(device).reshape(-1, 4))
        if int(boxes.size(0)) != n:
            raise ValueError(f"blend_image: {n} masks and {int(boxes.size(0))} boxes")
    if masks is None:
        masks, threshold = torch.zeros(1, h, w, dtype=torch.uint8, device=device).expand(n, h, w), 0
    else:
        masks = torch.as_tensor(masks).to(device)
    if masks.dtype not in (torch.uint8, torch.bool) or tuple(masks.shape) != (n, h, w):
        raise ValueError(f"blend_image: expected uint8 or bool masks [{n},{h},{w}], got {masks.dtype} {tuple(masks.shape)}")
    if threshold is None:
        threshold = 0 if masks.dtype == torch.bool else 127
    if not 0 <= int(threshold) <= 254:
        raise ValueError(f"blend_image: threshold={threshold} must be in [0, 254]")
    if colors is None:
        colors = random_colors(n) if n else []
    if not isinstance(colors, torch.Tensor):
        colors = torch.from_numpy(np.array(colors, dtype=np.uint8).reshape(-1, 3))
    colors = colors.to(device)
    if colors.dtype != torch.uint8 or tuple(colors.shape) != (n, 3):
        raise ValueError(f"blend_image: expected uint8 colors [{n},3], got {colors.dtype} {tuple(colors.shape)}")
    if device.type == "cpu":
        on = masks.view(torch.uint8).numpy() > int(threshold) if masks.dtype == torch.bool else masks.numpy() > int(threshold)
        return torch.from_numpy(_blend_host(img.numpy(), on, colors.numpy(), None if boxes is None else boxes.numpy()))
    return ops.blend_instances(img, masks, colors, boxes, int(threshold))
