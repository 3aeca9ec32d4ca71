"""GPU tests (-m gpu) of csrc/image.hip on the case tables of tests/image_cases.py: every branch of paste_masks_kernel (tap
loops, chunks, row tiles, store widths, validity, mask sizes and strides), every launch sequence of mrcnn_resize_bilinear_u8
(asserted through ops.resize_route before the launch), and mold_kernel up to its second grid-stride trip.

Everything is called through the C ABI into guarded buffers (the output in the middle of a buffer filled with 7, both bands checked
after every call) and compared bit for bit with the references of image_cases.py, which tests/test_image_cases_host.py pins
against Pillow itself. Byte and integer work, and float(double(u8) - mean) has one correct value: no tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import image_cases as ic
from test_gpu_refine_edges import BAND, _Out, _run

pytestmark = pytest.mark.gpu
U8 = torch.uint8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import maskrcnn_amd  # noqa: F401  must load libmaskrcnn_hip.so or fail loudly
    return torch.device("cuda:0")


class _OutAt(_Out):
    """A guarded uint8 output that starts `offset` bytes past a 16-byte boundary."""

    def __init__(self, shape, dev, offset=0, fill=7):
        self.n, self.fill = int(np.prod(shape, dtype=np.int64)), fill
        self.buf = torch.full((self.n + 2 * BAND + 16,), fill, dtype=U8, device=dev)
        assert self.buf.data_ptr() % 16 == 0 and BAND % 16 == 0
        self.start = BAND + offset
        self.t = self.buf[self.start:self.start + self.n].view(*shape)
        assert self.t.data_ptr() % 16 == offset % 16

    @property
    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.buf[:self.start] == self.fill).all()) and bool((self.buf[self.start + self.n:] == self.fill).all())


# ========================================================================================================== paste_masks
def _paste(dev, case, on_value, fill=7):
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import lib
    base, ids, boxes = ic.paste_inputs(case)
    masks = ic.mask_view(case, torch.from_numpy(base.copy()).to(dev))
    if case.layout == "nchw":
        sn, sc, sy, sx = masks.stride()
    else:
        sn, sy, sx, sc = masks.stride()
    assert masks.is_contiguous() == (case.view == "contiguous")
    out = _OutAt((len(case.dets), case.H, case.W), dev, case.out_offset, fill)
    assert ops.paste_store_width(case.W, out.ptr % 16) == case.store_width
    t_ids, t_boxes = torch.from_numpy(ids).to(dev), torch.from_numpy(boxes).to(dev)
    _run(lib.mrcnn_paste_masks_u8, (masks.data_ptr(), sn, sy, sx, sc, len(case.dets), case.mh, case.mw, case.C, t_ids.data_ptr(),
                                    t_boxes.data_ptr(), case.H, case.W, on_value, out.ptr), [out])
    return out.t.cpu().numpy()


@pytest.mark.parametrize("case", ic.PASTE_CASES, ids=lambda c: c.id)
def test_paste_every_slot_against_the_reference(dev, case):
    """Bit-equal to paste_ref (== oracle.full_masks == Pillow's literal sequence, on the host) for every valid slot, all zero for
    every invalid one — compared, not skipped —, nothing outside the output, and as_l8 the same mask times 255."""
    want = ic.paste_ref(case)
    got = _paste(dev, case, 1)
    assert got.shape == want.shape
    for i, det in enumerate(case.dets):
        if not ic.det_valid(case, det):
            assert not want[i].any()
            assert not got[i].any(), f"{case.id} slot {i} ({det.note}): an invalid slot is not empty"
        else:
            bad = np.argwhere(got[i] != want[i])
            assert bad.size == 0, f"{case.id} slot {i} ({det.note}): {len(bad)} pixels differ, first at {bad[0].tolist()}"
    assert np.array_equal(_paste(dev, case, 255), want * np.uint8(255)), case.id


LARGEST_PASTE = sorted(ic.PASTE_CASES, key=lambda c: -len(c.dets) * c.H * c.W)[:3]


@pytest.mark.parametrize("case", LARGEST_PASTE, ids=lambda c: c.id)
def test_paste_clears_the_canvas_itself(dev, case):
    """A second launch into a buffer of 0xFF gives the same bytes: the callee clears the canvases, invalid slots included."""
    assert np.array_equal(_paste(dev, case, 1, fill=0xFF), ic.paste_ref(case)), case.id


# =============================================================================================================== resize
_RESIZED = {}


def _resized(dev, case):
    """The case's one launch (kept: the twins are compared with each other afterwards)."""
    if case.id in _RESIZED:
        return _RESIZED[case.id]
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import lib
    base, _ = ic.resize_inputs(case)
    tb = torch.from_numpy(base.copy()).to(dev)
    top, left, _, _ = case.crop
    base_h, base_w = base.shape[1:3]
    src = tb.data_ptr() + (top * base_w + left) * case.c
    out = _OutAt((case.n, case.out_h, case.out_w, case.c), dev, case.dst_offset)
    nbytes = int(lib.mrcnn_resize_u8_workspace_bytes(case.n, case.in_h, case.in_w, case.c, case.out_h, case.out_w))
    ws = _OutAt((nbytes,), dev)
    route = ops.resize_route(case.n, case.in_h, case.in_w, case.c, case.out_h, case.out_w, out.ptr % 16, ws.ptr % 16)
    assert route == case.route, f"{case.id}: meant for {case.route}, the launcher takes {route}"
    _run(lib.mrcnn_resize_bilinear_u8, (src, case.n, case.in_h, case.in_w, case.c, base_h * base_w * case.c, base_w * case.c, out.ptr,
                                        case.out_h, case.out_w, ws.ptr, nbytes), [out, ws])
    _RESIZED[case.id] = out.t.cpu().numpy()
    return _RESIZED[case.id]


@pytest.mark.parametrize("case", ic.RESIZE_CASES, ids=lambda c: c.id)
def test_resize_takes_its_route_and_equals_the_reference(dev, case):
    want = ic.resize_ref(case)
    got = _resized(dev, case)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{case.id} ({case.route}): {len(bad)} bytes differ, first at {bad[0].tolist()}"


def test_resize_zero_tile_twins_differ_only_where_the_planted_byte_reaches(dev, oracle):
    twins = [c for c in ic.RESIZE_CASES if c.data.endswith("_twin")]
    assert len(twins) == 3
    for twin in twins:
        case = ic.resize_case(twin.id[:-len("_twin")])
        a, b = _resized(dev, case)[0, :, :, 0], _resized(dev, twin)[0, :, :, 0]
        (py, px), _ = ic.plant_position(case)
        bv, _ = oracle.resample_coeffs(case.in_h, case.out_h)
        bh, _ = oracle.resample_coeffs(case.in_w, case.out_w)
        rows = (bv[:, 0] <= py) & (py < bv[:, 0] + bv[:, 1])
        cols = (bh[:, 0] <= px) & (px < bh[:, 0] + bh[:, 1])
        reach = rows[:, None] & cols[None, :]
        assert np.array_equal(a[~reach], b[~reach]), case.id
        assert (a != b).any(), case.id


# ================================================================================================================= mold
@pytest.mark.parametrize("case", ic.MOLD_CASES, ids=lambda c: c.id)
def test_mold_equals_the_oracles_mold_of_the_padded_resize(dev, case):
    from maskrcnn_amd._lib import lib
    src = torch.from_numpy(ic.mold_inputs(case.id).copy()).to(dev)
    out = _Out((case.n, 3, case.out_h, case.out_w), torch.float32, dev)
    outs, ws_ptr, nbytes = [out], None, 0
    if (case.new_h, case.new_w) != (case.in_h, case.in_w):
        nbytes = int(lib.mrcnn_resize_u8_workspace_bytes(case.n, case.in_h, case.in_w, 3, case.new_h, case.new_w))
        ws = _OutAt((nbytes,), dev)
        outs, ws_ptr = [out, ws], ws.ptr
    mean = (ctypes.c_double * 3)(*case.mean)
    _run(lib.mrcnn_mold_images_u8, (src.data_ptr(), case.n, case.in_h * case.in_w * 3, case.in_h, case.in_w, case.new_h, case.new_w,
                                    case.top, case.left, case.out_h, case.out_w, mean, out.ptr, ws_ptr, nbytes), outs)
    got, want = out.t.cpu().numpy(), ic.mold_ref(case)
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, f"{case.id}: {len(bad)} values differ, first at {bad[0].tolist()}"
