"""RPN training targets on the GPU (csrc/targets.hip) against the reference's own outputs (tests/golden/targets.npz): every case
through ops.anchor_match / sample_by_key / rpn_deltas, through targets.rpn_targets and through torch.ops.maskrcnn.*.

Bounds: all integer outputs, iou_max, dy and dx are bit-equal to the fixture. dh and dw go through the device's fp64 log, which
is within one ulp of the host's, and are then narrowed to fp32: they may differ from the fixture by at most ONE fp32 ulp, and at
most 1 % of a case's finite dh / dw values may differ at all (none is expected: about 2^-29 per value)."""
import functools

import numpy as np
import pytest
import torch

from targets_cases import case, images, names, shared_geometry, ulp_distance

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = names()


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def inputs(c):
    return dev(c["anchors"]), dev(c["boxes"]), dev(c["ids"]), dev(c["off"]), dev(c["keys"])


def check_deltas(got, want, what):
    """→ the number of dh / dw values that differ (by one ulp); asserts the bounds of the module docstring."""
    got, want = np.asarray(got, np.float32).reshape(-1, 4), np.asarray(want, np.float32).reshape(-1, 4)
    assert got.shape == want.shape, what
    assert np.array_equal(got[:, :2].view(np.int32), want[:, :2].view(np.int32)), f"{what}: dy / dx"
    g, w = got[:, 2:], want[:, 2:]
    finite = np.isfinite(w)
    assert np.array_equal(np.isfinite(g), finite) and np.array_equal(g[~finite], w[~finite], equal_nan=True), f"{what}: infinities"
    d = ulp_distance(g[finite], w[finite])
    differ = int((d != 0).sum())
    print(f"{what}: {differ} of {int(finite.sum())} finite dh / dw values differ, largest distance {int(d.max()) if d.size else 0} ulp")
    assert d.size == 0 or d.max() <= 1, f"{what}: dh / dw off by {int(d.max())} ulp"
    assert differ <= 0.01 * finite.sum(), f"{what}: {differ} of {int(finite.sum())} dh / dw values differ"
    return differ


def check_sampled(c, bbox, what):
    """rpn_bbox [B,count,4] of a case: the positives' rows within the bounds, every other row zero (an image without a kept row
    has no positives). Only the positives' values count towards the 1 % bound, not the padding."""
    got = bbox.cpu().numpy()
    rows = np.arange(c["count"])[None, :] < (c["match"] == 1).sum(1)[:, None]
    assert not got[~rows].any() and not c["bbox"][~rows].any(), what
    return check_deltas(got[rows], c["bbox"][rows], what)


@functools.lru_cache(maxsize=None)
def dense_reference(name):
    """(iou_argmax [B,A], iou_max [B,A]) of a sparse case from the numpy route, which test_targets_host.py holds to the fixture."""
    from maskrcnn_amd import targets
    c = case(name)
    r = [targets.match_numpy(c["anchors"], b, i) for b, i in images(c)]
    return np.stack([x[1] for x in r]), np.stack([x[2] for x in r])


def check_case(c, anchor_match, sample_by_key, rpn_deltas):
    a, boxes, ids, off, keys = inputs(c)
    match_u, arg, iou, gt_arg, status = anchor_match(a, boxes, ids, off)
    torch.cuda.synchronize()
    n, name = c["anchors"].shape[0], c["name"]
    assert match_u.dtype == arg.dtype == gt_arg.dtype == status.dtype == torch.int32 and iou.dtype == torch.float32
    assert tuple(match_u.shape) == tuple(arg.shape) == tuple(iou.shape) == (c["batch"], n)
    assert np.array_equal(status.cpu().numpy(), c["status"]), name
    assert np.array_equal(match_u.cpu().numpy(), c["match_u"]), name
    assert np.array_equal(gt_arg.cpu().numpy(), c["gt_argmax"]), name
    if c["sparse"]:
        flat_arg, flat_iou = arg.cpu().numpy().ravel(), iou.cpu().numpy().ravel()
        assert np.array_equal(flat_arg[c["u_idx"]], c["u_argmax"]) and np.array_equal(bits(flat_iou[c["u_idx"]]), bits(c["u_iou"])), name
        want_arg, want_iou = dense_reference(name)
    else:
        want_arg, want_iou = c["argmax"], c["iou_max"]
    assert np.array_equal(arg.cpu().numpy(), want_arg), name
    assert np.array_equal(bits(iou), bits(want_iou)), name

    sampled = sample_by_key(match_u, keys, c["count"])
    assert sampled.data_ptr() != match_u.data_ptr() and np.array_equal(match_u.cpu().numpy(), c["match_u"])   # the input is not touched
    assert np.array_equal(sampled.cpu().numpy(), c["match"]), name
    # the ends of the 256-bin scan of the radix select, which takes the digits (key << 24 | anchor) >> 48, >> 40, ... & 255: every
    # key in bin 0 of the first pass (key >> 24 == 0), then every key in bin 255 of the second ((key >> 16) & 255 == 255; the
    # first pass's digit is a 31-bit key's top 7 bits and never passes 127), where only the scan's last thread holds a count.
    # Against the numpy route, which test_targets_host.py holds to the fixture
    from maskrcnn_amd import targets
    for what, ends in (("bin 0", c["keys"] >> 8), ("bin 255", (c["keys"] & 0xffff) | 0x00ff0000)):
        ends = np.ascontiguousarray(ends.astype(np.int32))
        assert (ends >> 24 == 0).all() and (what == "bin 0" or ((ends >> 16) & 255 == 255).all())
        want = np.stack([targets.sample_numpy(c["match_u"][i], ends[i], c["count"]) for i in range(c["batch"])])
        assert np.array_equal(sample_by_key(match_u, dev(ends), c["count"]).cpu().numpy(), want), (name, what)

    differ = 0
    bbox, num_pos = rpn_deltas(a, boxes, off, sampled, arg, c["count"])
    assert tuple(bbox.shape) == (c["batch"], c["count"], 4) and bbox.dtype == torch.float32
    assert np.array_equal(num_pos.cpu().numpy(), (c["match"] == 1).sum(1)), name
    differ += check_sampled(c, bbox, f"{name} sampled")
    # every positive's deltas: the unsampled match, `count` = the largest number of positives of an image
    most = max(int(c["npos_all"].max()), 1)
    every, num_all = rpn_deltas(a, boxes, off, match_u, arg, most)
    assert np.array_equal(num_all.cpu().numpy(), c["npos_all"]), name
    every = every.cpu().numpy()
    assert all(not every[i, k:].any() for i, k in enumerate(c["npos_all"]))
    got = np.concatenate([every[i, :k] for i, k in enumerate(c["npos_all"])])
    differ += check_deltas(got, c["bbox_all"], f"{name} unsampled")
    return differ


@pytest.mark.parametrize("name", NAMES)
def test_ops_equal_the_reference(name):
    from maskrcnn_amd import ops
    check_case(case(name), ops.anchor_match, ops.sample_by_key, ops.rpn_deltas)


@pytest.mark.parametrize("name", NAMES)
def test_dispatcher_ops_equal_the_reference(name):
    import maskrcnn_amd  # noqa: F401
    t = torch.ops.maskrcnn
    check_case(case(name), t.anchor_match, t.sample_by_key,
               lambda a, boxes, off, match, arg, count: t.rpn_deltas(a, boxes, off, match, arg, count, [0.1, 0.1, 0.2, 0.2]))


@pytest.mark.parametrize("name", names(usable_only=True))
def test_rpn_targets_equals_the_reference(name):
    from maskrcnn_amd import targets
    c = case(name)
    bs, cs = zip(*images(c))
    a, boxes, ids, off, keys = inputs(c)
    for form in ("lists", "packed host", "packed device"):
        if form == "lists":
            m, b = targets.rpn_targets(c["anchors"], list(bs), list(cs), c["count"], keys=c["keys"], device=DEV)
        elif form == "packed host":
            m, b = targets.rpn_targets(torch.from_numpy(c["anchors"].copy()), c["boxes"], c["ids"], c["count"], keys=keys, device=DEV, gt_off=c["off"])
        else:
            m, b = targets.rpn_targets(a, boxes, ids, c["count"], keys=keys, device=DEV, gt_off=off)
        assert m.is_cuda and m.dtype == torch.int32 and tuple(m.shape) == (c["batch"], c["anchors"].shape[0], 1), form
        assert np.array_equal(m.cpu().numpy()[..., 0], c["match"]), (name, form)
        check_sampled(c, b, f"{name} rpn_targets {form}")


def test_rpn_targets_refuses_an_image_without_usable_ground_truth_and_draws_keys():
    from maskrcnn_amd import targets
    c = case("pyr64_all_crowd")
    bs, cs = zip(*images(c))
    with pytest.raises(ValueError, match="image 0 has no usable ground truth"):
        targets.rpn_targets(c["anchors"], list(bs), list(cs), device=DEV)
    c = case("pyr128_b3_count8")
    bs, cs = zip(*images(c))
    run = lambda seed: targets.rpn_targets(c["anchors"], list(bs), list(cs), 8, device=DEV,
                                           generator=torch.Generator(device=DEV).manual_seed(seed))
    (m1, b1), (m2, b2), (m3, _) = run(5), run(5), run(6)
    assert torch.equal(m1, m2) and torch.equal(bits_t(b1), bits_t(b2)) and not torch.equal(m1, m3)
    m = m1.cpu().numpy()[..., 0]
    assert ((m == 1).sum(1) <= 4).all() and ((m != 0).sum(1) == 8).all()
    assert ((m == 1) <= (c["match_u"] == 1)).all() and ((m == -1) <= (c["match_u"] == -1)).all()


def bits_t(t):
    return t.view(torch.int32)


def test_anchor_match_and_detection_targets_match_one_geometry_alike():
    """The two kernels share their matching rule (csrc/target_match.hpp): on the same 100 boxes (a partial wave) the RoIs
    detection_targets keeps as positives — pos_iou 0.7, positive_ratio 1 and count 100: every one that reaches the threshold, no
    negatives — are the anchors whose iou_max reaches it, each matched to the same row. test_targets_host.py holds the numpy
    routes to the same on this input."""
    from maskrcnn_amd import ops
    g = shared_geometry()
    boxes, ids, off = dev(g["gt"]), dev(g["ids"]), dev(g["off"])
    _, arg, iou, _, status = ops.anchor_match(dev(g["boxes"]), boxes, ids, off)
    rois = dev(np.stack([g["boxes"]] * 2), np.float32)
    _, _, _, roi_index, gt_index, num_pos, num_neg, roi_status = ops.detection_targets(rois, boxes, ids, off, dev(g["keys"]), 100, 1.0,
                                                                                         pos_iou=0.7)
    arg, iou, roi_index, gt_index = arg.cpu().numpy(), iou.cpu().numpy(), roi_index.cpu().numpy(), gt_index.cpu().numpy()
    assert status.tolist() == roi_status.tolist() == [0, 0] and num_neg.tolist() == [0, 0]
    for i, p in enumerate(num_pos.tolist()):
        want = np.where((arg[i] >= 0) & (iou[i] >= np.float32(0.7)))[0]
        assert len(want) >= 1 and sorted(roi_index[i, :p].tolist()) == want.tolist(), i
        assert np.array_equal(gt_index[i, :p], arg[i][roi_index[i, :p]]), i


@pytest.mark.parametrize("name", ["pyr128_b3_count8_mod4_keys", "full_b2"])
def test_two_runs_other_stream_and_out_give_the_same_bits(name):
    from maskrcnn_amd import ops
    c = case(name)
    a, boxes, ids, off, keys = inputs(c)

    def run(out=None):
        r = ops.anchor_match(a, boxes, ids, off)
        s = ops.sample_by_key(r[0], keys, c["count"], out=out)
        return (*r, s, *ops.rpn_deltas(a, boxes, off, s, r[1], c["count"]))

    first, second = run(), run()
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    given = torch.full((c["batch"], c["anchors"].shape[0]), 77, dtype=torch.int32, device=DEV)
    with torch.cuda.stream(stream):
        third = run(out=given)
    stream.synchronize()
    assert third[5] is given
    for x, y, z in zip(first, second, third):
        assert x.dtype == y.dtype == z.dtype
        v = bits_t if x.dtype == torch.float32 else (lambda t: t)
        assert torch.equal(v(x), v(y)) and torch.equal(v(x), v(z))
    # in place: out is the match itself
    m = first[0].clone()
    assert ops.sample_by_key(m, keys, c["count"], out=m) is m and torch.equal(m, first[5])


def test_positives_beyond_count_are_counted_not_written():
    from maskrcnn_amd import ops
    c = case("rows1024")                                    # 64 positives in image 0, 2 in image 1
    a, boxes, ids, off, _ = inputs(c)
    match_u, arg = dev(c["match_u"]), dev(c["argmax"])
    full, n_full = ops.rpn_deltas(a, boxes, off, match_u, arg, 64)
    part, n_part = ops.rpn_deltas(a, boxes, off, match_u, arg, 5)
    assert n_full.tolist() == n_part.tolist() == [64, 2]
    assert torch.equal(bits_t(part[0]), bits_t(full[0, :5])) and torch.equal(bits_t(part[1, :2]), bits_t(full[1, :2])) and not part[1, 2:].any()


def test_indices_out_of_range_are_clamped_not_followed():
    """The ops stay memory-safe on anything: a row index outside the image gives a row of zeros, row offsets beyond the packed
    rows are clamped to them."""
    from maskrcnn_amd import ops
    c = case("pyr64_b3")
    a, boxes, ids, off, _ = inputs(c)
    match, want_arg = dev(c["match_u"]), c["argmax"]
    pos = np.argwhere(c["match_u"] == 1)
    arg = want_arg.copy()
    arg[pos[0][0], pos[0][1]] = 2 ** 31 - 1
    arg[pos[1][0], pos[1][1]] = -7
    arg[pos[2][0], pos[2][1]] = 6                           # image 0 has rows 0..5
    bbox, num = ops.rpn_deltas(a, boxes, off, match, dev(arg), 16)
    good, _ = ops.rpn_deltas(a, boxes, off, match, dev(want_arg), 16)
    assert num.tolist() == c["npos_all"].tolist()
    assert not bbox[0, :3].any() and torch.equal(bits_t(bbox[0, 3:]), bits_t(good[0, 3:])) and torch.equal(bits_t(bbox[1:]), bits_t(good[1:]))
    wild = dev(np.array([0, 6, 10 ** 6, 2 ** 31 - 1], np.int32))      # image 1 and 2 reach past the 10 rows
    m, ar, _, gt_arg, status = ops.anchor_match(a, boxes, ids, wild)
    torch.cuda.synchronize()
    assert np.array_equal(m[0].cpu().numpy(), c["match_u"][0]) and np.array_equal(ar[0].cpu().numpy(), c["argmax"][0])
    assert status.tolist() == [0, 0, 1] and gt_arg.tolist()[:6] == c["gt_argmax"].tolist()[:6]
    assert int(ar[1].max()) < 4 and (ar[2] == -1).all() and not m[2].any()
