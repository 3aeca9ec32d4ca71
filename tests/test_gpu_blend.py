"""ops.blend_instances / image.blend_image (csrc/overlay.hip) on the GPU, bit for bit against tests/golden/blend.npz — the
reference's own blend_image under Pillow — and, where Pillow cannot go (extreme int32 boxes), against the numpy host route that
tests/test_blend_host.py holds to the same fixture. The largest input is the tile-seam case (40 x 530, 7 instances)."""
import numpy as np
import pytest
import torch

from test_blend_host import INT32_MAX, INT32_MIN, blend_cases, case, host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)


def boxes_i32(c):
    return dev(np.trunc(c["boxes"]), np.int32)


def run_op(c, **kw):
    from maskrcnn_amd import ops
    args = dict(image=dev(c["image"]), masks=dev(c["masks"]), colors=dev(c["colors"]), boxes=boxes_i32(c), threshold=0)
    args.update(kw)
    return ops.blend_instances(**args)


def same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape, what
    bad = np.argwhere((got != want).any(2))
    assert bad.size == 0, (what, len(bad), bad[:5].tolist())


def test_the_op_equals_every_golden_case():
    for c in blend_cases():
        same(run_op(c), c["want"], c["name"])
        same(torch.ops.maskrcnn.blend_instances(dev(c["image"]), dev(c["masks"]), dev(c["colors"]), boxes_i32(c), 0), c["want"],
             c["name"])


def test_blend_image_equals_every_golden_case():
    """The front end with what a caller has: a numpy image, float boxes (truncated on the device), a list of colour tuples."""
    from maskrcnn_amd import image
    for c in blend_cases():
        got = image.blend_image(np.array(c["image"]), dev(c["boxes"]), dev(c["masks"]), [tuple(v) for v in c["colors"].tolist()],
                                threshold=0, device=DEV)
        assert got.is_cuda
        same(got, c["want"], c["name"])


def test_grey_masks_with_threshold_127():
    from maskrcnn_amd import image
    rng = np.random.default_rng(11)
    for name in ("overlap3_17x23", "seams_40x530", "random_3x3", "checkerboard_17x23"):
        c = case(name)
        grey = np.where(c["masks"] > 0, rng.integers(128, 256, c["masks"].shape), rng.integers(0, 128, c["masks"].shape)).astype(np.uint8)
        grey.reshape(-1)[:4] = np.where(c["masks"].reshape(-1)[:4] > 0, (128, 255, 128, 255), (127, 0, 127, 0))   # both sides of the bar
        same(run_op(c, masks=dev(grey), threshold=127), c["want"], name)
        same(image.blend_image(dev(c["image"]), dev(c["boxes"]), dev(grey), dev(c["colors"]), device=DEV), c["want"], name)   # uint8: 127
    for t in (1, 100, 254):                                              # other thresholds: the byte compare on packed words
        c = case("seams_40x530")
        levels = np.where(c["masks"] > 0, rng.integers(t + 1, 256, c["masks"].shape), rng.integers(0, t + 1, c["masks"].shape)).astype(np.uint8)
        same(run_op(c, masks=dev(levels), threshold=t), c["want"], t)


def test_bool_masks_and_rle_masks():
    from maskrcnn_amd import image
    for name in ("overlap3_17x23", "seams_40x530", "n50_24x40"):
        c = case(name)
        same(run_op(c, masks=dev(c["masks"]).bool()), c["want"], name)
        same(image.blend_image(dev(c["image"]), dev(c["boxes"]), dev(c["masks"]).bool(), dev(c["colors"]), device=DEV), c["want"], name)
        rle = image.rle_masks(dev(c["masks"]))
        assert isinstance(rle, image.RleMasks)
        same(image.blend_image(dev(c["image"]), dev(c["boxes"]), rle, dev(c["colors"]), device=DEV), c["want"], name)


def embed(a, stride, pad_rows, offset, fill):
    """a [..., R, C] as a view cropped out of a larger `fill`-valued uint8 buffer: rows `stride` >= C bytes apart, pad_rows rows
    between the images, the first byte `offset` bytes into the allocation. → (view, whole buffer)."""
    a = torch.as_tensor(np.array(a))
    lead, (r, c) = a.shape[:-2], a.shape[-2:]
    per = (r + pad_rows) * stride
    count = int(np.prod(lead)) if lead else 1
    buf = torch.full((offset + count * per + 64,), fill, dtype=torch.uint8, device=DEV)
    view = buf[offset:offset + count * per].view(*lead, r + pad_rows, stride)[..., :r, :c]
    view.copy_(a.to(DEV))
    return view, buf


def is_aligned(t):
    return t.data_ptr() % 16 == 0 and all(s % 16 == 0 for s in t.stride()[:-1])


@pytest.mark.parametrize("masks_aligned", [True, False])
@pytest.mark.parametrize("image_aligned", [True, False])
def test_strided_operands_and_untouched_surroundings(masks_aligned, image_aligned):
    """image, masks and out as views cropped out of larger tensors: 16-byte-aligned bases and strides (the 16-byte path; the
    allocator's bases are aligned) and an odd byte offset with odd row strides (the byte path), masks and image / out each way,
    give the same expected bytes, and every byte of out's buffer outside the H x 3W region keeps its sentinel. The golden widths
    are no multiples of 16, so the waves of the last tile column go byte by byte on either path (and the seam case has two
    whole tile columns before it); the 12 x 48 crop has whole runs only, three lanes of a 16-lane tile row, and is checked
    against the host route."""
    from maskrcnn_amd import ops
    seams = case("seams_40x530")
    y0, x0 = 9, 240                                                       # 12 x 48 across the tile seam x = 256
    crop = dict(image=np.array(seams["image"][y0:y0 + 12, x0:x0 + 48]), masks=np.array(seams["masks"][:, y0:y0 + 12, x0:x0 + 48]),
                colors=seams["colors"], h=12, w=48, n=seams["n"],
                boxes=np.array([[2, 3, 9, 40], [0, 0, 11, 47], [5, 15, 5, 33], [-2, 16, 20, 31], [3, 17, 8, 32], [4, 4, 4, 4],
                                [1, 47, 10, 47]], np.float64))
    crop["want"] = host(crop, masks=torch.from_numpy(crop["masks"]))
    for c in (seams, case("blobs_9x37"), case("overlap3_17x23"), crop):
        h, w = c["h"], c["w"]
        wide = (w + 15) // 16 * 16 + 16
        m_stride, m_off = (wide, 32) if masks_aligned else (w + 5, 3)
        i_stride, i_off = (3 * wide, 16) if image_aligned else (3 * w + 7, 1)
        img, _ = embed(c["image"].reshape(h, 3 * w), i_stride, 2, i_off, 9)
        masks, _ = embed(c["masks"], m_stride, 3, m_off, 1)          # the surroundings are ON: they must never be read as pixels
        out, whole = embed(np.zeros((h, 3 * w), np.uint8), i_stride, 2, i_off, 0xA5)
        assert is_aligned(masks) == masks_aligned and is_aligned(img) == image_aligned and is_aligned(out) == image_aligned
        before = whole.clone()
        out3 = out.unflatten(1, (w, 3))
        got = ops.blend_instances(img.unflatten(1, (w, 3)), masks, dev(c["colors"]), boxes_i32(c), 0, out3)
        assert got is out3
        same(got, c["want"], (c.get("name", "crop"), masks_aligned, image_aligned))
        out.zero_()                                                   # what is left must be the buffer as it was
        assert torch.equal(whole, before), c.get("name", "crop")
    same(ops.blend_instances(dev(crop["image"]), dev(crop["masks"]), dev(crop["colors"]), boxes_i32(crop)), crop["want"], "contiguous")


def test_in_place():
    from maskrcnn_amd import ops
    for name in ("seams_40x530", "overlap3_17x23", "n50_24x40"):
        c = case(name)
        img = dev(c["image"])
        got = ops.blend_instances(img, dev(c["masks"]), dev(c["colors"]), boxes_i32(c), 0, out=img)
        assert got is img
        same(img, c["want"], name)


def test_no_instances():
    from maskrcnn_amd import image, ops
    c = case("n0_5x7")
    same(run_op(c), c["image"], "n0")
    same(image.blend_image(dev(c["image"]), None, torch.zeros(0, 5, 7, dtype=torch.bool, device=DEV), device=DEV), c["image"], "n0")
    big = case("seams_40x530")
    same(ops.blend_instances(dev(big["image"]), dev(big["masks"][:0]), dev(big["colors"][:0]), None), big["image"], "n0 big")


def test_no_boxes_equals_boxes_wholly_outside():
    from maskrcnn_amd import image
    for name in ("overlap3_reversed_17x23", "seams_40x530"):
        c = case(name)
        outside = dev(np.tile(np.array([[-9, -9, -5, -5]], np.int32), (c["n"], 1)))
        a, b = run_op(c, boxes=None), run_op(c, boxes=outside)
        assert torch.equal(a, b), name
        same(image.blend_image(dev(c["image"]), None, dev(c["masks"]), dev(c["colors"]), threshold=0, device=DEV), a.cpu().numpy(), name)
    c = case("overlap3_reversed_17x23")
    same(run_op(c, boxes=None), c["want"], "the fixture's boxes are outside too")
    # boxes only: masks=None in the front end
    c = case("box_all_17x23")
    same(image.blend_image(dev(c["image"]), dev(c["boxes"]), None, dev(c["colors"]), device=DEV), c["want"], "boxes only")


def test_extreme_int32_boxes_against_the_host_route():
    c = case("overlap3_17x23")
    boxes = np.array([[INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX], [INT32_MAX, 3, INT32_MAX, 9], [3, INT32_MAX, 9, INT32_MAX]], np.int32)
    want = host(c, boxes=torch.from_numpy(boxes))
    same(run_op(c, boxes=dev(boxes)), want, "extreme")
    boxes = np.array([[INT32_MIN, 4, 8, INT32_MAX], [INT32_MAX - 1, INT32_MIN, INT32_MAX, 5], [INT32_MIN, INT32_MIN, 6, 11]], np.int32)
    want = host(c, boxes=torch.from_numpy(boxes))
    assert not np.array_equal(want, host(c, boxes=None))                  # these do reach into the image
    same(run_op(c, boxes=dev(boxes)), want, "extreme, visible")
    # an inverted box draws nothing on the device
    inverted = np.array([[9, 3, 4, 12], [3, 12, 9, 4], [2, 2, 10, 12]], np.int32)
    visible = np.array([[-9, -9, -5, -5], [-9, -9, -5, -5], [2, 2, 10, 12]], np.int32)
    same(run_op(c, boxes=dev(inverted)), host(c, boxes=torch.from_numpy(visible)), "inverted")


def test_two_runs_give_identical_bytes():
    for name in ("seams_40x530", "n50_24x40"):
        c = case(name)
        assert torch.equal(run_op(c), run_op(c)), name


def test_bad_arguments_are_refused():
    from maskrcnn_amd import ops
    c = case("overlap3_17x23")
    with pytest.raises(RuntimeError, match="masks"):
        run_op(c, masks=dev(c["masks"][:, :, :20]))
    with pytest.raises(RuntimeError, match="colors"):
        run_op(c, colors=dev(c["colors"][:2]))
    with pytest.raises(RuntimeError, match="boxes"):
        run_op(c, boxes=dev(np.trunc(c["boxes"]), np.int64))
    with pytest.raises(RuntimeError, match="out must be"):
        run_op(c, out=torch.empty(17, 23, 4, dtype=torch.uint8, device=DEV)[:, :, :3])
    with pytest.raises(ops.MaskrcnnHipError, match="threshold=255"):
        run_op(c, threshold=255)
