"""Case builders and the independent reference for the backward of the pyramid RoIAlign (ops.roi_align_pyramid_backward,
csrc/roi_align_backward.hip), shared by tests/test_roi_align_backward_host.py, tests/test_gpu_roi_align_backward.py and
tests/golden/make_golden_roi_align_backward.py. Nothing here touches a GPU.

expected(): per image and level, the committed oracle.crop_backward (oracle/crop_ref.c: the C restatement of crop_cpu.cpp:167-265,
pinned to the reference's own output by tests/golden/crop_backward.npz) on that level's RoIs in index order, on NCHW, permuted to
NHWC. That is what the reference's roi_align backward amounts to: model.py:347-352 hands each level its boxes in original order
(`nonzero` keeps it), CropFunction.backward runs crop_backward per level, and the cat / permutation backward only moves rows.
"""
import numpy as np
import torch

F32 = np.float32
CHUNK = 64            # RoIs per chunk of the tile kernel for pool <= 16 (csrc/roi_align_backward.hip: MAX_CHUNK)
TILE = 8              # its tile side


def chunk_for(pool):
    """RoIs per chunk (csrc/roi_align_backward.hip: chunk_for): the chunk's tables hold at most 2048 samples."""
    return CHUNK if pool <= 16 else 1024 // pool


def roi_images(num_rois, batch, rois_per_image=None, roi_batch=None, roi_counts=None):
    """The image of every RoI, -1 where it contributes nothing (a slot at or past roi_counts[image], an image outside [0, batch))."""
    idx = np.arange(num_rois)
    img = np.asarray(roi_batch, np.int64) if roi_batch is not None else idx // int(rois_per_image)
    ok = (img >= 0) & (img < batch)
    if roi_counts is not None:
        counts = np.asarray(roi_counts, np.int64)
        ok &= (idx - img * int(rois_per_image)) < counts[np.clip(img, 0, len(counts) - 1)]
    return np.where(ok, img, -1)


def expected(oracle, grad_out, rois, levels, batch, map_sizes, rois_per_image=None, roi_batch=None, roi_counts=None):
    """grad_out float32 [R,pool,pool,C] (NHWC), rois float32 [R,4], levels int [R] of 2..5 (what the FORWARD kernel reported, or the
    fixture's) → the four gradients, float32 tensors [batch,H_l,W_l,C]."""
    grad_out = torch.as_tensor(np.asarray(grad_out, F32))
    rois = torch.as_tensor(np.asarray(rois, F32)).reshape(-1, 4)
    levels = np.asarray(levels, np.int64)
    r, c = grad_out.shape[0], grad_out.shape[3]
    img = roi_images(r, batch, rois_per_image, roi_batch, roi_counts)
    nchw = grad_out.permute(0, 3, 1, 2).contiguous()
    out = []
    for l, (h, w) in enumerate(map_sizes):
        g = torch.zeros(batch, h, w, c)
        for b in range(batch):
            sel = torch.as_tensor(np.nonzero((img == b) & (levels == l + 2))[0])          # ascending RoI index
            if len(sel):
                gi = oracle.crop_backward(nchw[sel], rois[sel], torch.zeros(len(sel), dtype=torch.int32), (1, c, h, w))
                g[b] = gi[0].permute(1, 2, 0)
        out.append(g)
    return out


def samples(c1, c2, size, pool):
    """crop_math.hpp's make_sample for t = 0 .. pool-1 in numpy fp32 → (lo, hi, lerp, inside). Finite coordinates only."""
    c1, c2 = F32(c1), F32(c2)
    if pool > 1:
        scale = F32(F32(F32(c2 - c1) * F32(size - 1)) / F32(pool - 1))
        pos = (F32(c1 * F32(size - 1)) + (np.arange(pool, dtype=F32) * scale).astype(F32)).astype(F32)
    else:
        pos = np.array([F32(0.5 * float(F32(c1 + c2)) * float(size - 1))], F32)
    inside = ~((pos < 0) | (pos > F32(size - 1)))
    lo = np.where(inside, np.floor(pos), 0).astype(np.int64)
    hi = np.where(inside, np.ceil(pos), 0).astype(np.int64)
    return lo, hi, (pos - lo.astype(F32)).astype(F32), inside


def rois_meeting_tile(rois, levels, level, size, pool, tile_y=0, tile_x=0):
    """How many RoIs of `level` have a footprint (the lo .. hi of their inside samples) that meets tile (tile_y, tile_x) of the
    level's map: the length of that tile's list in the kernel."""
    h, w = size
    n = 0
    for box in np.asarray(rois, F32)[np.asarray(levels) == level]:
        meets = []
        for c1, c2, extent, t0 in ((box[0], box[2], h, tile_y * TILE), (box[1], box[3], w, tile_x * TILE)):
            lo, hi, _, inside = samples(c1, c2, extent, pool)
            meets.append(bool(inside.any()) and lo[inside].min() <= min(t0 + TILE, extent) - 1 and hi[inside].max() >= t0)
        n += all(meets)
    return n


def unrounded_level(rois, image_area):
    """k = 4 + log2(sqrt(h*w) / (224 / sqrt(area))) in float64 from the fp32 coordinates (model.py:324-336 without the rounding)."""
    r = np.asarray(rois, F32).astype(np.float64)
    hw = (r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])
    with np.errstate(all="ignore"):
        return 4.0 + np.log2(np.sqrt(hw) / (224.0 / np.sqrt(float(image_area))))


def levels_of(rois, image_area):
    """The level of boxes whose unrounded level is far from a boundary (asserted): no log2 implementation can disagree there."""
    k = unrounded_level(rois, image_area)
    far = np.abs(k[:, None] - np.array([2.5, 3.5, 4.5])[None]).min(1) >= 1e-3
    assert bool((far | ~np.isfinite(k)).all()), "a box within 1e-3 of a level boundary: redraw"
    return np.where(np.isfinite(k) & (k >= 2), np.clip(np.rint(np.where(np.isfinite(k), k, 2)), 2, 5), 2).astype(np.int32)


def side_for_level(level, image_area):
    """The side of a square box (normalised) in the middle of `level`'s range (levels 2 and 5: half a level inside)."""
    return float(2.0 ** (level - 4.0) * 224.0 / np.sqrt(image_area))


def wide_grads(rng, shape):
    """Gradients over 12 binades with random signs: sums whose rounding depends on the order of the terms."""
    return (rng.standard_normal(shape) * np.exp2(rng.integers(-6, 7, shape))).astype(F32)


def order_case(oracle):
    """One 8 x 8 P5 map, C = 4, 400 near-identical RoIs over the whole map at pool 2: 400 terms on each corner pixel. Asserts that
    the reversed RoI order changes at least a quarter of the touched elements: the case can tell the orders apart."""
    area = 512.0 * 512.0
    sizes = [(64, 64), (32, 32), (16, 16), (8, 8)]
    for seed in range(20):
        rng = np.random.default_rng(1000 + seed)
        n, pool, c = 400, 2, 4
        jitter = (rng.integers(0, 64, (n, 4)) / 4096.0).astype(F32)
        rois = (np.array([0.0, 0.0, 1.0, 1.0], F32) + jitter * np.array([1, 1, -1, -1], F32)).astype(F32)
        levels = levels_of(rois, area)
        assert bool((levels == 5).all())
        grad = wide_grads(rng, (n, pool, pool, c))
        want = expected(oracle, grad, rois, levels, 1, sizes, rois_per_image=n)
        rev = expected(oracle, grad[::-1].copy(), rois[::-1].copy(), levels[::-1].copy(), 1, sizes, rois_per_image=n)
        touched = want[3] != 0
        changed = (want[3].view(torch.int32) != rev[3].view(torch.int32)) & touched
        assert int(touched.sum()) >= 4 * c
        if int(changed.sum()) * 4 >= int(touched.sum()):
            return dict(rois=rois, grad=grad, levels=levels, pool=pool, area=area, sizes=sizes, want=want, rpi=n)
    raise AssertionError("no draw whose sums depend on the RoI order: the case proves nothing")


def boxes_on(rng, n, level, area, spread=0.35):
    """n square-ish boxes of `level`, centres anywhere in the image (they may spill outside [0, 1])."""
    side = side_for_level(level, area) * np.exp2(rng.uniform(-0.3, 0.3, n))
    aspect = np.exp2(rng.uniform(-0.15, 0.15, n))
    h, w = side * aspect, side / aspect
    cy, cx = rng.uniform(0.5 - spread, 0.5 + spread, n), rng.uniform(0.5 - spread, 0.5 + spread, n)
    return np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1).astype(F32)
