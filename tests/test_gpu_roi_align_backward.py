"""GPU tests (-m gpu) of the backward of the pyramid RoIAlign: ops.roi_align_pyramid_backward (csrc/roi_align_backward.hip), the
grad_fn of ops.roi_align_pyramid and of the NCHW drop-in maskrcnn_amd.roi_align.

Every comparison is on the bits (NaNs by position). The references: tests/golden/roi_align_backward.npz (the reference's own
crop_backward behind model.roi_align's level split) and, for every other case, roi_align_backward_cases.expected — the committed
oracle.crop_backward per image and level on the RoIs in index order, with the levels the FORWARD kernel reports.
The shapes are the smallest at which the kernel can still go wrong: maps that are no multiple of the 8 x 8 tile down to one pixel,
RoIs across every tile edge, one more / one fewer / twice the RoIs a chunk (64) holds on one tile, channel counts around the
256-channel step of a wave. The file runs once more in a child pytest on the schedule-fuzz library."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import roi_align_backward_cases as rc
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ_LIB = os.path.join(ROOT, "maskrcnn_amd", "csrc", "build", "variants", "sync_fuzz", "libmaskrcnn_hip.so")
F32 = np.float32
ODD_SIZES = [(13, 9), (7, 5), (3, 2), (1, 1)]      # P2 .. P5: no multiple of the tile; a 1-pixel map has size - 1 = 0
AREA = 256.0 * 256.0


@pytest.fixture(scope="module")
def ops():
    from maskrcnn_amd import ops as o
    return o


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


def assert_same_bits(got, want, what=""):
    assert len(got) == len(want) == 4
    for l, (g, w) in enumerate(zip(got, want)):
        g, w = g.detach().cpu(), w.detach().cpu()
        assert g.shape == w.shape and g.dtype == w.dtype == torch.float32, (what, l, g.shape, w.shape)
        gn, wn = torch.isnan(g), torch.isnan(w)
        assert torch.equal(gn, wn), f"{what}: level P{l + 2}: NaNs at other elements"
        same = g.view(torch.int32)[~gn] == w.view(torch.int32)[~wn]
        assert bool(same.all()), f"{what}: level P{l + 2}: {int((~same).sum())} of {same.numel()} elements differ in their bits"


def forward_levels(ops, rois, pool, area, batch, sizes, channels=4, **kw):
    """The level the forward kernel gives every RoI (rows of skipped slots are unwritten: expected() drops those RoIs)."""
    maps = [torch.zeros(batch, h, w, channels, device=DEV) for h, w in sizes]
    kw = {k: (dev(v, np.int32) if k in ("roi_batch", "roi_counts") and v is not None else v) for k, v in kw.items()}
    _, levels = ops.roi_align_pyramid(maps, dev(rois, F32), pool, area, return_levels=True, **kw)
    return levels.cpu().numpy()


def backward(ops, grad, rois, pool, area, batch, sizes, out=None, **kw):
    kw = {k: (dev(v, np.int32) if k in ("roi_batch", "roi_counts") and v is not None else v) for k, v in kw.items()}
    got = ops.roi_align_pyramid_backward(dev(grad, F32), dev(rois, F32), pool, area, batch, sizes, out=out, **kw)
    torch.cuda.synchronize()
    return got


def check(ops, oracle, grad, rois, pool, area, batch, sizes, what, **kw):
    levels = forward_levels(ops, rois, pool, area, batch, sizes, channels=grad.shape[3], **kw)
    want = rc.expected(oracle, grad, rois, levels, batch, sizes, **kw)
    got = backward(ops, grad, rois, pool, area, batch, sizes, **kw)
    assert_same_bits(got, want, what)
    return got, want, levels


def mixed_rois(rng, per_level, area=AREA):
    """RoIs of all four levels, shuffled; the centres anywhere in the image, so they cross every tile edge and spill outside."""
    rois = np.concatenate([rc.boxes_on(rng, n, level, area, spread=0.5) for level, n in zip((2, 3, 4, 5), per_level)])
    return rois[rng.permutation(len(rois))]


# ------------------------------------------------------------------------------------------------------------------- golden
@pytest.mark.parametrize("pool", [7, 14, 1])
def test_golden_op_autograd_and_nchw_drop_in(ops, pool):
    import maskrcnn_amd
    z = load_golden("roi_align_backward")
    rois, grad = z["rois"], z[f"grad_out_p{pool}"]
    sizes = [tuple(int(v) for v in s) for s in z["map_sizes"]]
    shape = tuple(int(v) for v in z["image_shape"])
    area, n, c = float(shape[0] * shape[1]), len(rois), grad.shape[3]
    want = [torch.from_numpy(z[f"g{l}_p{pool}"]) for l in range(4)]
    assert np.array_equal(forward_levels(ops, rois, pool, area, 1, sizes, channels=c, rois_per_image=n), z["levels"])
    assert_same_bits(backward(ops, grad, rois, pool, area, 1, sizes, rois_per_image=n), want, "op")

    maps = [torch.randn(1, h, w, c, device=DEV).requires_grad_(True) for h, w in sizes]
    with torch.no_grad():
        plain = ops.roi_align_pyramid(maps, dev(rois), pool, area, rois_per_image=n)
    assert plain.grad_fn is None
    out, levels = ops.roi_align_pyramid(maps, dev(rois), pool, area, rois_per_image=n, return_levels=True)
    assert out.grad_fn is not None and not levels.requires_grad and torch.equal(out, plain)
    assert np.array_equal(levels.cpu().numpy(), z["levels"])
    out.backward(dev(grad))
    assert_same_bits([m.grad for m in maps], want, "roi_align_pyramid(...).backward")
    for flag in ("out_kblocked", "out_f16")[c % 8 != 0:]:      # the inference layouts stay without a gradient (k-blocked: C % 8 == 0)
        assert ops.roi_align_pyramid(maps, dev(rois), pool, area, rois_per_image=n, **{flag: True}).grad_fn is None

    nchw = [m.detach().permute(0, 3, 1, 2).contiguous().requires_grad_(True) for m in maps]
    pooled = maskrcnn_amd.roi_align([dev(rois).unsqueeze(0)] + nchw, pool, shape)
    assert pooled.grad_fn is not None and torch.equal(pooled, plain.permute(0, 3, 1, 2))
    pooled.backward(dev(grad).permute(0, 3, 1, 2).contiguous())
    assert_same_bits([m.grad.permute(0, 2, 3, 1).contiguous() for m in nchw], want, "roi_align(...).backward")


# -------------------------------------------------------------------------------------------------------------------- order
def test_summation_order_is_the_references_and_two_calls_agree(ops, oracle):
    """400 RoIs on one pixel of a P5 map, gradients over 12 binades: the case builder has asserted that the reversed order gives
    other bits on at least a quarter of the touched elements. 400 RoIs on one tile are seven chunks."""
    c = rc.order_case(oracle)
    assert np.array_equal(forward_levels(ops, c["rois"], c["pool"], c["area"], 1, c["sizes"], rois_per_image=c["rpi"]), c["levels"])
    got = backward(ops, c["grad"], c["rois"], c["pool"], c["area"], 1, c["sizes"], rois_per_image=c["rpi"])
    assert_same_bits(got, c["want"], "order")
    again = backward(ops, c["grad"], c["rois"], c["pool"], c["area"], 1, c["sizes"], rois_per_image=c["rpi"])
    assert_same_bits(again, [g.cpu() for g in got], "second call")


# --------------------------------------------------------------------------------------------------------- tiles and chunks
C64 = rc.CHUNK            # the chunk of every pool up to 16
C28 = rc.chunk_for(28)    # 36: a pool whose tables bound the chunk below the 64 records a wave tests at a time


@pytest.mark.parametrize("on_one_tile, depth, pool", [(C64 - 1, 4, 7), (C64, 8, 2), (C64 + 1, 8, 7), (2 * C64, 4, 7), (2 * C64 + 1, 4, 1),
                                                      (20, 256, 7), (C64 + 1, 260, 2), (3 * C28 + 2, 4, 28), (2 * C28, 4, 28)])
def test_odd_maps_tile_edges_chunk_boundaries_and_channel_tails(ops, oracle, on_one_tile, depth, pool):
    """P3 is 7 x 5: ONE tile, met by exactly `on_one_tile` RoIs (counted from the samples, asserted) — one fewer than a chunk, a
    chunk, one more, two chunks and one more; at pool 28 a chunk is 36 RoIs, so 64 records can fill it twice and the list is
    shifted by less than it holds. The other levels get RoIs across their tile edges (P2: 13 x 9 is 2 x 2 tiles)."""
    rng = np.random.default_rng(on_one_tile * 1000 + depth)
    edge = np.array([[0.55, 0.8, 0.8, 1.0], [0.6, 0.75, 0.85, 1.0]], F32)       # level 2, across P2's inner tile edges (row 8, column 8)
    rois = np.concatenate([rc.boxes_on(rng, on_one_tile, 3, AREA, spread=0.3), mixed_rois(rng, (24, 0, 6, 4)), edge])
    rois = rois[rng.permutation(len(rois))]
    grad = rc.wide_grads(rng, (len(rois), pool, pool, depth))
    _, want, levels = check(ops, oracle, grad, rois, pool, AREA, 1, ODD_SIZES, "tiles", rois_per_image=len(rois))
    assert sorted(set(levels.tolist())) == [2, 3, 4, 5]
    assert rc.rois_meeting_tile(rois, levels, 3, ODD_SIZES[1], pool) == on_one_tile == int((levels == 3).sum())
    for box in edge:                                                             # on both sides of P2's row 8 and column 8
        for c1, c2, extent in ((box[0], box[2], 13), (box[1], box[3], 9)):
            lo, hi, _, inside = rc.samples(c1, c2, extent, pool)
            assert pool == 1 or (lo[inside].min() < rc.TILE <= hi[inside].max()), (box, extent)
    assert [rc.rois_meeting_tile(rois, levels, 2, ODD_SIZES[0], pool, ty, tx) > 0 for ty in (0, 1) for tx in (0, 1)] == [True] * 4
    assert all(bool(w.any()) for w in want)


# ----------------------------------------------------------------------------------------------------------------- geometry
GEOMETRY = np.array([
    [0.0, 0.0, 1.0, 1.0],            # samples exactly on 0 and on size - 1
    [-0.5, 0.1, 0.5, 0.6],           # outside above
    [0.5, 0.1, 1.5, 0.6],            # outside below
    [0.1, -0.5, 0.6, 0.5],           # outside left
    [0.1, 0.5, 0.6, 1.5],            # outside right
    [-2.0, -2.0, -1.0, -1.0],        # wholly outside
    [0.8, 0.2, 0.3, 0.7],            # y2 < y1
    [0.2, 0.8, 0.7, 0.3],            # x2 < x1
    [0.9, 0.9, 0.2, 0.1],            # both
    [0.4, 0.3, 0.4, 0.3],            # zero area
    [0.0, 0.0, 0.0, 0.0],            # zero area on the corner
    [0.25, 0.25, 0.5, 0.5], [0.0, 0.0, 2.0, 2.0], [-1.0, -1.0, 2.0, 2.0],
], F32)


@pytest.mark.parametrize("pool", [1, 2, 7, 14])
@pytest.mark.parametrize("sizes", [ODD_SIZES, [(16, 16), (8, 8), (4, 4), (2, 2)]])
def test_sample_geometry(ops, oracle, pool, sizes):
    rng = np.random.default_rng(pool)
    rois = np.concatenate([GEOMETRY, mixed_rois(rng, (6, 6, 4, 4))])
    grad = rc.wide_grads(rng, (len(rois), pool, pool, 8))
    check(ops, oracle, grad, rois, pool, AREA, 1, sizes, f"geometry pool {pool}", rois_per_image=len(rois))


def test_a_roi_with_nan_coordinates_touches_nothing_but_pixel_0_0_of_its_level(ops, oracle):
    rng = np.random.default_rng(5)
    rois = mixed_rois(rng, (8, 8, 4, 4))
    grad = rc.wide_grads(rng, (len(rois) + 1, 7, 7, 8))
    sizes = [(16, 16), (8, 8), (4, 4), (2, 2)]
    at = 9
    with_nan = np.insert(rois, at, np.array([np.nan, 0.2, 0.6, np.nan], F32), axis=0)
    level = 2      # roi_level: h * w is NaN, so is k, and `!(k >= 2)` lands on level 2 (the forward is not asked: it would gather there)
    got = backward(ops, grad, with_nan, 7, AREA, 1, sizes, rois_per_image=len(with_nan))            # completes
    without = backward(ops, np.delete(grad, at, axis=0), rois, 7, AREA, 1, sizes, rois_per_image=len(rois))
    got, without = [g.cpu().clone() for g in got], [g.cpu().clone() for g in without]
    got[level - 2][0, 0, 0] = without[level - 2][0, 0, 0]      # the CPU's behaviour there is undefined: not compared
    assert_same_bits(got, without, "NaN RoI")


# -------------------------------------------------------------------------------------------------------------------- batch
def batch_case(seed, batch=3, per_image=20, depth=8, pool=7):
    rng = np.random.default_rng(seed)
    rois = np.concatenate([mixed_rois(rng, (8, 6, 4, 2)) for _ in range(batch)])
    assert len(rois) == batch * per_image
    return rng, rois, rc.wide_grads(rng, (len(rois), pool, pool, depth)), pool


def test_batch_by_slot_by_index_and_by_count(ops, oracle):
    rng, rois, grad, pool = batch_case(11)
    b, per = 3, 20
    got, _, _ = check(ops, oracle, grad, rois, pool, AREA, b, ODD_SIZES, "rois_per_image", rois_per_image=per)
    # the same RoIs shuffled, their images named by roi_batch, with RoIs of image -1 and image B (= nothing) in between
    extra = mixed_rois(rng, (3, 2, 2, 1))
    order = rng.permutation(len(rois) + len(extra))
    all_rois = np.concatenate([rois, extra])[order]
    all_grad = np.concatenate([grad, np.full((len(extra), pool, pool, grad.shape[3]), np.nan, F32)])[order]
    image = np.concatenate([np.repeat(np.arange(b), per), np.array([-1, b] * 4)])[order].astype(np.int32)
    _, want, _ = check(ops, oracle, all_grad, all_rois, pool, AREA, b, ODD_SIZES, "roi_batch", roi_batch=image)
    assert all(bool(torch.isfinite(w).all()) for w in want)
    # roi_counts: the slots past the count hold NaN gradients (the forward leaves their rows unwritten) and are never read
    counts = np.array([20, 7, 0], np.int32)
    nan_grad = grad.copy()
    for i, n in enumerate(counts):
        nan_grad[i * per + n:(i + 1) * per] = np.nan
    counted, want, _ = check(ops, oracle, nan_grad, rois, pool, AREA, b, ODD_SIZES, "roi_counts", rois_per_image=per, roi_counts=counts)
    assert all(bool(torch.isfinite(g).all()) for g in counted) and not any(bool(g[2].any()) for g in counted)
    assert_same_bits([g[:1] for g in counted], [g[:1] for g in got], "image 0 with all its slots")


def test_an_images_gradients_do_not_depend_on_the_rest_of_the_batch(ops):
    _, rois, grad, pool = batch_case(12)
    per = 20
    whole = backward(ops, grad, rois, pool, AREA, 3, ODD_SIZES, rois_per_image=per)
    for i in range(3):
        alone = backward(ops, grad[i * per:(i + 1) * per], rois[i * per:(i + 1) * per], pool, AREA, 1, ODD_SIZES, rois_per_image=per)
        assert_same_bits(alone, [g[i:i + 1] for g in whole], f"image {i} alone")
    perm = [2, 0, 1]
    rows = np.concatenate([np.arange(i * per, (i + 1) * per) for i in perm])
    moved = backward(ops, grad[rows], rois[rows], pool, AREA, 3, ODD_SIZES, rois_per_image=per)
    assert_same_bits([g[[perm.index(i) for i in range(3)]] for g in moved], whole, "images in another order")


# -------------------------------------------------------------------------------------------------------- every byte written
def nan_filled(batch, sizes, depth):
    return [torch.full((batch, h, w, depth), -1, dtype=torch.int32, device=DEV).view(torch.float32) for h, w in sizes]


def test_every_byte_is_written_and_untouched_pixels_are_plus_zero(ops, oracle):
    rng = np.random.default_rng(21)
    sizes = [(21, 19), (9, 10), (3, 2), (1, 1)]
    rois = np.array([[0.1, 0.1, 0.2, 0.25], [0.7, 0.6, 0.8, 0.75], [0.1, 0.2, 0.5, 0.7]], F32)      # two on P2, one on P3: most pixels untouched
    grad = -np.abs(rc.wide_grads(rng, (3, 2, 2, 8)))          # negative terms: a sum that starts from -0 would stay -0
    levels = forward_levels(ops, rois, 2, AREA, 2, sizes, channels=8, roi_batch=np.array([0, 0, 1]))
    want = rc.expected(oracle, grad, rois, levels, 2, sizes, roi_batch=np.array([0, 0, 1]))
    out = nan_filled(2, sizes, 8)
    assert all(bool(torch.isnan(o).all()) for o in out)
    got = backward(ops, grad, rois, 2, AREA, 2, sizes, out=out, roi_batch=np.array([0, 0, 1]))
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    assert_same_bits(got, want, "out=")
    for g, w in zip(got, want):
        untouched = w == 0
        assert bool(untouched.any()) and bool((g.cpu().view(torch.int32)[untouched] == 0).all()), "an untouched pixel is not +0"
    # no RoI at all
    out = nan_filled(2, sizes, 8)
    got = ops.roi_align_pyramid_backward(torch.empty(0, 7, 7, 8, device=DEV), torch.empty(0, 4, device=DEV), 7, AREA, 2, sizes,
                                         rois_per_image=5, out=out)
    torch.cuda.synchronize()
    assert all(bool((g.view(torch.int32) == 0).all()) for g in got)


def test_out_tensors_and_arguments_are_checked(ops):
    g, rois, sizes = torch.zeros(2, 7, 7, 8, device=DEV), torch.zeros(2, 4, device=DEV), [(8, 8), (4, 4), (2, 2), (1, 1)]
    with pytest.raises(RuntimeError, match=r"roi_align_pyramid_backward: out tensor grad_P3 must be float32 \[1,4,4,8\] contiguous on cuda:0, got"):
        ops.roi_align_pyramid_backward(g, rois, 7, AREA, 1, sizes, rois_per_image=2,
                                       out=[torch.empty(1, h, w, 8 if h != 4 else 4, device=DEV) for h, w in sizes])
    with pytest.raises(RuntimeError, match="roi_align_pyramid_backward: out must hold 4 tensors"):
        ops.roi_align_pyramid_backward(g, rois, 7, AREA, 1, sizes, rois_per_image=2, out=[torch.empty(1, 8, 8, 8, device=DEV)])
    with pytest.raises(RuntimeError, match=r"roi_align_pyramid_backward: grad_out must be float32 \[R,7,7,C\], got float32 \[2, 7, 6, 8\]"):
        ops.roi_align_pyramid_backward(g[:, :, :6], rois, 7, AREA, 1, sizes, rois_per_image=2)
    with pytest.raises(RuntimeError, match=r"roi_align_pyramid_backward: grad_out must be float32 \[R,7,7,C\] with C a multiple of 4"):
        ops.roi_align_pyramid_backward(g[..., :6], rois, 7, AREA, 1, sizes, rois_per_image=2)
    with pytest.raises(RuntimeError, match=r"roi_align_pyramid_backward: rois must be float32 \[2,4\], got float32 \[3, 4\]"):
        ops.roi_align_pyramid_backward(g, torch.zeros(3, 4, device=DEV), 7, AREA, 1, sizes, rois_per_image=2)
    with pytest.raises(RuntimeError, match=r"roi_align_pyramid_backward: roi_batch must be int32 \[2\] or None, got int64"):
        ops.roi_align_pyramid_backward(g, rois, 7, AREA, 1, sizes, roi_batch=torch.zeros(2, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="roi_align_pyramid_backward: rois_per_image must be >= 1 without roi_batch, got None"):
        ops.roi_align_pyramid_backward(g, rois, 7, AREA, 1, sizes)
    with pytest.raises(RuntimeError, match="roi_align_pyramid_backward: roi_counts must be None with roi_batch"):
        ops.roi_align_pyramid_backward(g, rois, 7, AREA, 1, sizes, roi_batch=torch.zeros(2, dtype=torch.int32, device=DEV),
                                       roi_counts=torch.zeros(1, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------------------------------------------ non-finite gradients
def test_infinite_gradients_on_grid_line_samples_give_the_references_nans(ops, oracle):
    """[0,0,1,1] (level 4 of a 256 x 256 image) on a 16 x 16 map at pool 7 samples 0, 2.5, 5, ..: on every other sample lo == hi and lerp == 0, and the replayed
    zero-weight taps turn an infinite gradient into NaN (0 * inf), as in crop_cpu.cpp:254-260."""
    rng = np.random.default_rng(31)
    sizes = [(31, 31), (8, 8), (16, 16), (2, 2)]
    rois = np.concatenate([np.array([[0.0, 0.0, 1.0, 1.0]], F32), rc.boxes_on(rng, 10, 4, AREA)])
    lo, hi, lerp, inside = rc.samples(0.0, 1.0, 16, 7)
    assert bool((inside & (lo == hi) & (lerp == 0)).sum() >= 3) and bool((lerp != 0).any())
    grad = rc.wide_grads(rng, (len(rois), 7, 7, 4))
    grad[0, 0, 0, :2] = np.inf          # on a grid line in both axes
    grad[0, 2, 1, 2:] = -np.inf         # on a grid line in y only
    grad[0, 3, 3, 0] = np.inf           # between grid lines: no NaN, infinities on four pixels
    _, want, levels = check(ops, oracle, grad, rois, 7, AREA, 1, sizes, "infinite gradients", rois_per_image=len(rois))
    assert levels[0] == 4 and bool(torch.isnan(want[2]).any()) and bool(torch.isinf(want[2]).any())


# ------------------------------------------------------------------------------------------------------------------ adjoint
def test_backward_is_the_adjoint_of_the_forward(ops):
    """<forward(x), g> and <x, backward(g)>, both inner products in float64 on the host, are the same sum over (bin, tap) of
    w_tap * x_tap * g in exact arithmetic. The bound on their difference, with u = 2^-24 and S = the sum over inside bins, their four
    taps and the channels of |x_tap| * |g| (the weights are at most 1):
      forward: bilerp is 8 operations on values bounded by 2 * (sum of the bin's |taps|): at most 16 u * (sum of |taps|) per bin;
      backward: a term is three roundings (1 - lerp, two products), a pixel's sum of m terms m - 1 more: (m + 2) u * sum |g|;
    so |difference| <= (m_max + 18) * u * S, m_max the largest number of terms behind one map element."""
    rng = np.random.default_rng(41)
    sizes, pool, c = [(16, 16), (8, 8), (4, 4), (2, 2)], 3, 4
    rois = np.concatenate([mixed_rois(rng, (10, 8, 6, 4)), GEOMETRY[:5]])
    n = len(rois)
    x = [rng.standard_normal((1, h, w, c)).astype(F32) for h, w in sizes]
    g = rng.standard_normal((n, pool, pool, c)).astype(F32)
    out, levels = ops.roi_align_pyramid([dev(v) for v in x], dev(rois), pool, AREA, rois_per_image=n, return_levels=True)
    gx = backward(ops, g, rois, pool, AREA, 1, sizes, rois_per_image=n)
    lhs = float((out.cpu().numpy().astype(np.float64) * g).sum())
    rhs = float(sum((a.astype(np.float64) * b.cpu().numpy()).sum() for a, b in zip(x, gx)))
    s, terms = 0.0, [np.zeros((h, w), np.int64) for h, w in sizes]
    for r, lv in enumerate(levels.cpu().numpy()):
        h, w = sizes[lv - 2]
        ylo, yhi, _, yin = rc.samples(rois[r, 0], rois[r, 2], h, pool)
        xlo, xhi, _, xin = rc.samples(rois[r, 1], rois[r, 3], w, pool)
        for i in np.nonzero(yin)[0]:
            for j in np.nonzero(xin)[0]:
                for yy in (ylo[i], yhi[i]):
                    for xx in (xlo[j], xhi[j]):
                        s += float((np.abs(x[lv - 2][0, yy, xx].astype(np.float64)) * np.abs(g[r, i, j])).sum())
                        terms[lv - 2][yy, xx] += 1
    m_max = max(int(t.max()) for t in terms)
    bound = (m_max + 18) * 2.0 ** -24 * s
    print(f"adjoint: <Fx,g> = {lhs:.9g}, <x,Bg> = {rhs:.9g}, |difference| {abs(lhs - rhs):.3e}, bound {bound:.3e} "
          f"(m_max {m_max}, S {s:.4g}): {abs(lhs - rhs) / bound:.4f} of the bound")
    assert s > 0 and m_max >= 4 and abs(lhs - rhs) <= bound


# ----------------------------------------------------------------------------------------------------------------- the link
def test_head_losses_backward_reaches_the_four_maps(ops):
    """targets.detection_targets -> roi_align_pyramid on maps that require grad -> one linear layer per head output ->
    losses.head_losses -> .backward(): the gradients arrive on P2 .. P4 and P5, which no RoI chose, gets exact zeros."""
    from maskrcnn_amd import losses, targets
    rng = np.random.default_rng(51)
    side, count, classes, c, pool, mh = 256, 12, 3, 8, 7, 4
    sizes = [(64, 64), (32, 32), (16, 16), (8, 8)]
    gt = np.array([[20, 30, 70, 82], [100, 90, 228, 220], [10, 12, 238, 244],          # image 0: levels 2, 3, 4
                   [150, 40, 204, 96], [30, 100, 160, 226]], F32)                       # image 1: levels 2, 3
    ids, off = np.array([1, 2, 1, 2, 1], np.int32), np.array([0, 3, 5], np.int32)
    masks = np.zeros((5, side, side), np.uint8)
    for i, (y1, x1, y2, x2) in enumerate(gt.astype(int)):
        masks[i, y1:y2, x1:x2] = 1
    rois = np.zeros((2, 24, 4), F32)
    for b in range(2):
        mine = gt[off[b]:off[b + 1]]
        near = np.repeat(mine, 4, axis=0) + rng.integers(-4, 5, (4 * len(mine), 4))
        small = rng.integers(0, 200, (24 - len(near), 2))
        rois[b] = np.clip(np.concatenate([near, np.concatenate([small, small + rng.integers(20, 50, small.shape)], 1)]), 0, side)
    # the positives are taken by ascending key: the first jittered copy of every ground-truth box comes first
    j = np.arange(24)
    keys = np.stack([np.where(j < 4 * n, (j % 4) * 10 + j // 4, 100 + j) for n in (3, 2)]).astype(np.int32)
    t = targets.detection_targets(dev(rois / side), dev(gt / side), dev(ids), dev(masks), count=count, mask_shape=(mh, mh), keys=dev(keys),
                                  device=DEV, gt_off=dev(off))
    maps = [dev(rng.standard_normal((2, h, w, c)).astype(F32)).requires_grad_(True) for h, w in sizes]
    pooled, levels = ops.roi_align_pyramid(maps, t.rois.reshape(-1, 4), pool, float(side * side), rois_per_image=count, return_levels=True)
    flat = pooled.reshape(2 * count, -1)
    heads = [dev((rng.standard_normal((flat.size(1), n)) * 0.05).astype(F32)) for n in (classes, classes * 4, classes * mh * mh)]
    logits, pbox = flat @ heads[0], (flat @ heads[1]).reshape(-1, classes, 4)
    pmask = torch.sigmoid(flat @ heads[2]).reshape(-1, classes, mh, mh)
    head = losses.head_losses(t, logits, pbox, pmask)
    (head.class_loss + head.bbox_loss + head.mask_loss).backward()
    torch.cuda.synchronize()
    grads = [m.grad.cpu() for m in maps]
    levels, num_pos, boxes = levels.cpu().numpy().reshape(2, count), t.num_pos.cpu().numpy(), t.rois.cpu().numpy()
    assert int(num_pos.min()) > 0 and all(bool(torch.isfinite(g).all()) for g in grads)
    assert 5 not in levels and not bool(grads[3].any()) and {2, 3, 4} <= set(levels.reshape(-1).tolist())
    for b in range(2):
        for s in range(int(num_pos[b])):
            h, w = sizes[levels[b, s] - 2]
            y1, x1, y2, x2 = boxes[b, s]
            ys = slice(int(np.floor(y1 * (h - 1))), int(np.ceil(y2 * (h - 1))) + 1)
            xs = slice(int(np.floor(x1 * (w - 1))), int(np.ceil(x2 * (w - 1))) + 1)
            assert bool(grads[levels[b, s] - 2][b, ys, xs].any()), f"no gradient under positive RoI {s} of image {b}"


# --------------------------------------------------------------------------------------------------------- schedule fuzzing
# The child's time limit: four times the wall time measured on the fuzzed library, rounded up to 30 s: 5.6 s (29 tests; 3.6 s of
# it inside pytest, the rest start-up), so 22.4 s -> 30 s.
FUZZ_TIMEOUT = 30


@pytest.mark.skipif(os.environ.get("MRCNN_SYNC_FUZZ_CHILD") == "1", reason="this IS the fuzzed child run")
def test_this_file_passes_under_schedule_fuzzing():
    """Every barrier of roi_backward_tiles — the list before a chunk's tables are built, the tables before the waves read them, the
    readers before the list is shifted and the next chunk's tables overwrite them — is followed by a random sleep per wave on that
    build; a hand-off that a barrier does not order fails its comparison there."""
    assert os.path.exists(FUZZ_LIB), f"{FUZZ_LIB} is missing: run __graft_entry__.build()"
    env = dict(os.environ, MRCNN_LIB=FUZZ_LIB, MRCNN_SYNC_FUZZ_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_roi_align_backward.py", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=FUZZ_TIMEOUT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
