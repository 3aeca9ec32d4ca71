"""Detection training targets on the GPU (csrc/detection_targets.hip) against the reference's own model.mrn_samples outputs
(tests/golden/detection_targets.npz): every case through ops.detection_targets / ops.mask_targets, through
torch.ops.maskrcnn.* and through targets.detection_targets.

Bars (detection_targets_cases.compare): every integer output, rois_out, dy, dx and every mask target are bit-equal to the fixture
(so the device equals the numpy route bit for bit there: test_detection_targets_host.py holds that route to the same bits). dh
and dw: torch's fp32 CPU log may differ from a correctly rounded one by one ulp and one correctly rounded division by std_dev can
carry that to two, so 2 fp32 ulps against the fixture."""
import functools

import numpy as np
import pytest
import torch

from detection_targets_cases import STD_DEV, case, case_masks, compare, images, names

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = names()
OUT_NAMES = ("rois_out", "class_ids", "deltas", "roi_index", "gt_index", "num_pos", "num_neg", "status")


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)


def bits_t(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@functools.lru_cache(maxsize=None)
def masks_of(name):
    m = case_masks(case(name))
    m.setflags(write=False)
    return m


def inputs(c):
    return dev(c["rois"]), dev(c["boxes"]), dev(c["ids"]), dev(c["off"]), dev(c["keys"])


def run_ops(c, detection_targets, mask_targets, masks=None):
    rois, boxes, ids, off, keys = inputs(c)
    masks = dev(masks_of(c["name"])) if masks is None else masks
    outs = detection_targets(rois, boxes, ids, off, keys, c["count"], c["ratio"], list(STD_DEV))
    tm = mask_targets(masks, off, outs[0], outs[4], outs[5], list(c["mask_shape"]))
    torch.cuda.synchronize()
    assert [t.dtype for t in outs] == [torch.float32, torch.int32, torch.float32] + [torch.int32] * 5 and tm.dtype == torch.float32
    assert tuple(tm.shape) == (c["batch"], c["count"], *c["mask_shape"])
    got = {k: t.cpu().numpy() for k, t in zip(OUT_NAMES, outs)}
    got["target_mask"] = tm.cpu().numpy()
    return got


@pytest.mark.parametrize("name", NAMES)
def test_ops_equal_the_reference(name):
    from maskrcnn_amd import ops
    c = case(name)
    compare(c, run_ops(c, ops.detection_targets, ops.mask_targets))


@pytest.mark.parametrize("name", NAMES)
def test_dispatcher_ops_equal_the_reference(name):
    import maskrcnn_amd  # noqa: F401
    c = case(name)
    compare(c, run_ops(c, torch.ops.maskrcnn.detection_targets, torch.ops.maskrcnn.mask_targets))


def front_end_dict(t):
    v = {k: getattr(t, k).cpu().numpy() for k in t._fields}
    v["rois_out"], v["class_ids"], v["deltas"] = v.pop("rois"), v.pop("target_class_ids"), v.pop("target_deltas")
    return v


@pytest.mark.parametrize("name", names(usable_only=True))
def test_detection_targets_equals_the_reference(name):
    from maskrcnn_amd import targets
    c = case(name)
    masks = masks_of(name)
    bs, cs = zip(*images(c))
    ms = [masks[s:e] for s, e in zip(c["off"][:-1], c["off"][1:])]
    kw = dict(count=c["count"], positive_ratio=c["ratio"], mask_shape=c["mask_shape"], device=DEV)
    rois, boxes, ids, off, keys = inputs(c)
    for form in ("lists", "packed host", "packed device"):
        if form == "lists":
            t = targets.detection_targets(list(c["rois"]), list(bs), list(cs), ms, keys=c["keys"], **kw)
        elif form == "packed host":
            t = targets.detection_targets(c["rois"], c["boxes"], c["ids"], masks, keys=keys, gt_off=c["off"], **kw)
        else:
            t = targets.detection_targets(rois, boxes, ids, dev(masks), keys=keys, gt_off=off, **kw)
        assert all(v.is_cuda for v in t), form
        compare(c, front_end_dict(t))
    for i in range(c["batch"]):
        n = int(c["num_pos"][i] + c["num_neg"][i])
        r, k, d, m = t.unpad(i)
        if n == 0:
            assert [tuple(x.shape) for x in (r, k, d, m)] == [(0,)] * 4
        else:
            assert tuple(m.shape) == (n, *c["mask_shape"]) and np.array_equal(r.cpu().numpy(), c["rois_out"][i, :n])
            assert np.array_equal(k.cpu().numpy(), c["class_ids"][i, :n]) and tuple(d.shape) == (n, 4)


def test_front_end_refuses_an_unusable_image_and_draws_keys():
    from maskrcnn_amd import targets
    c = case("all_crowd_between")
    with pytest.raises(ValueError, match="image 1 has no usable ground truth"):
        targets.detection_targets(c["rois"], c["boxes"], c["ids"], masks_of(c["name"]), gt_off=c["off"], device=DEV)
    # drawn keys: reproducible from the generator, and valid: num_pos <= pos_limit, num_neg <= neg_limit, every index of its class
    c = case("both_limits_ratio0.33")
    run = lambda seed, count: targets.detection_targets(c["rois"], c["boxes"], c["ids"], masks_of(c["name"]), count=count, gt_off=c["off"],
                                                        device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    a, b, d = run(5, 100), run(5, 100), run(6, 100)
    assert all(torch.equal(bits_t(x), bits_t(y)) for x, y in zip(a, b)) and not torch.equal(a.roi_index, d.roi_index)
    cls = targets.roi_match_numpy(c["rois"][0], c["boxes"], c["ids"])[0]
    for t, count in ((a, 100), (d, 100), (run(7, 8), 8), (run(8, 31), 31)):
        p, q = int(t.num_pos[0]), int(t.num_neg[0])
        pos_limit = int(count * 0.33)
        assert p == min(pos_limit, int((cls == 0).sum())) and q == min(int(1.0 / 0.33 * p - p), int((cls == 1).sum()))
        idx = t.roi_index[0].cpu().numpy()
        assert (cls[idx[:p]] == 0).all() and (cls[idx[p:p + q]] == 1).all() and (idx[p + q:] == -1).all()
        assert len(set(idx[:p + q].tolist())) == p + q
        got = targets.mask_targets_numpy(masks_of(c["name"]), t.gt_index[0, :p].cpu().numpy(), c["rois"][0][idx[:p]])
        assert np.array_equal(t.target_mask[0, :p].cpu().numpy(), got) and not t.target_mask[0, p:].any()


@pytest.mark.parametrize("name", ["basic_b3_count8_mod4_keys", "n4096_rows50"])
def test_two_runs_other_stream_and_out_give_the_same_bits(name):
    from maskrcnn_amd import ops
    c = case(name)
    rois, boxes, ids, off, keys = inputs(c)
    masks = dev(masks_of(name))

    def run(out=None, mask_out=None):
        r = ops.detection_targets(rois, boxes, ids, off, keys, c["count"], c["ratio"], out=out)
        return (*r, ops.mask_targets(masks, off, r[0], r[4], r[5], c["mask_shape"], out=mask_out))

    first, second = run(), run()
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    given = tuple(torch.full_like(t, 77) for t in first[:8])
    given_mask = torch.full_like(first[8], 77.0)
    with torch.cuda.stream(stream):
        third = run(out=given, mask_out=given_mask)
    stream.synchronize()
    assert all(x is y for x, y in zip(third[:8], given)) and third[8] is given_mask
    for x, y, z in zip(first, second, third):
        assert x.dtype == y.dtype == z.dtype
        assert torch.equal(bits_t(x), bits_t(y)) and torch.equal(bits_t(x), bits_t(z))
    with pytest.raises(RuntimeError, match="out tensor num_pos"):
        ops.detection_targets(rois, boxes, ids, off, keys, c["count"], c["ratio"], out=(*given[:5], given[5].long(), *given[6:]))


def test_uint8_bool_and_float32_masks_give_the_same_targets():
    from maskrcnn_amd import ops
    c = case("basic_b3")
    base = masks_of("basic_b3")
    assert base.dtype == np.uint8 and set(np.unique(base).tolist()) == {0, 1}
    want = run_ops(c, ops.detection_targets, ops.mask_targets)["target_mask"]
    for m in (dev(base).bool(), dev(base).float(), dev(base.astype(bool))):
        got = run_ops(c, ops.detection_targets, ops.mask_targets, masks=m)["target_mask"]
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), m.dtype
    assert np.array_equal(want, c["target_mask"])


def with_canary(shape, dtype, fill):
    """(a contiguous tensor of `shape` at the front of a larger buffer, the 4096 elements behind it)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 4096,), fill, dtype=dtype, device=DEV)
    return buf[:n].view(shape), buf[n:]


def test_indices_out_of_range_are_clamped_not_followed():
    """The ops stay memory-safe on anything: row offsets beyond the packed rows are clamped to them, a row index outside the image
    or a num_pos outside [0, count] gives slots of zeros; outputs stay within their shapes (a canary region behind each)."""
    from maskrcnn_amd import ops
    c = case("basic_b3")
    rois, boxes, ids, off, keys = inputs(c)
    masks = dev(masks_of("basic_b3"))
    b, count, (mh, mw) = c["batch"], c["count"], c["mask_shape"]
    spec = ((torch.float32, (b, count, 4)), (torch.int32, (b, count)), (torch.float32, (b, count, 4)), (torch.int32, (b, count)),
            (torch.int32, (b, count)), (torch.int32, (b,)), (torch.int32, (b,)), (torch.int32, (b,)))
    outs, canaries = zip(*[with_canary(s, d, 77) for d, s in spec])
    wild = dev(np.array([0, 4, 10 ** 6, 2 ** 31 - 1], np.int32))          # images 1 and 2 reach past the 8 rows
    got = ops.detection_targets(rois, boxes, ids, wild, keys, count, c["ratio"], out=outs)
    torch.cuda.synchronize()
    assert all((cn == 77).all() for cn in canaries)
    good = ops.detection_targets(rois, boxes, ids, off, keys, count, c["ratio"])
    for g, w, k in zip(got, good, OUT_NAMES):
        assert torch.equal(bits_t(g[0]), bits_t(w[0])), k                                # image 0 is untouched by its neighbours
    assert got[7].tolist() == [0, 0, 1] and got[5].tolist()[2] == 0 and (got[3][2] == -1).all() and not got[0][2].any()
    assert int(got[4][1].max()) < 4 and int(got[4][1, :int(got[5][1])].min()) >= 0       # image 1: rows 4 .. 7, clamped to the 8
    negative = dev(np.array([-5, -1, 3, 2], np.int32))                                    # a start below 0, an end below the start
    got = ops.detection_targets(rois, boxes, ids, negative, keys, count, c["ratio"])
    assert got[7].tolist() == [1, 0, 1] and int(got[4][1].max()) < 3                      # rows [0,0), [0,3), [3,3)

    # mask_targets: wild gt_index and num_pos
    rois_out, _, _, _, gt_index, num_pos, _, _ = good
    want = ops.mask_targets(masks, off, rois_out, gt_index, num_pos, (mh, mw))
    assert np.array_equal(want.cpu().numpy(), c["target_mask"])
    bad = gt_index.clone()
    bad[0, 0], bad[0, 1], bad[0, 2], bad[1, 0] = 2 ** 31 - 1, -7, 4, 3                    # image 0 has rows 0..3, image 1 rows 0..2
    out, canary = with_canary((b, count, mh, mw), torch.float32, 77.0)
    got = ops.mask_targets(masks, off, rois_out, bad, num_pos, (mh, mw), out=out)
    torch.cuda.synchronize()
    assert got is out and (canary == 77).all()
    assert not got[0, :3].any() and not got[1, 0].any()
    assert torch.equal(got[0, 3:], want[0, 3:]) and torch.equal(got[1, 1:], want[1, 1:]) and torch.equal(got[2], want[2])
    out, canary = with_canary((b, count, mh, mw), torch.float32, 77.0)
    got = ops.mask_targets(masks, off, rois_out, gt_index, dev(np.array([10 ** 6, -5, 2 ** 31 - 1], np.int32)), (mh, mw), out=out)
    torch.cuda.synchronize()
    assert (canary == 77).all() and not got[1].any()
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])                 # slots past the positives hold gt_index -1
    out, canary = with_canary((b, count, mh, mw), torch.float32, 77.0)
    got = ops.mask_targets(masks, wild, rois_out, gt_index, num_pos, (mh, mw), out=out)   # mask rows past the 8: clamped
    torch.cuda.synchronize()
    assert (canary == 77).all() and torch.equal(got[0], want[0]) and not got[2].any()
    # a NaN box passes the crop's inside test: its taps are clamped into the mask
    nan_rois = rois_out.clone()
    nan_rois[0, 0] = float("nan")
    got = ops.mask_targets(masks, off, nan_rois, gt_index, num_pos, (mh, mw))
    torch.cuda.synchronize()
    assert torch.equal(got[0, 1:], want[0, 1:])


def test_mask_offsets_above_2_to_31():
    """33 byte masks of 8192 x 8192 are 2.2 GB: the last row starts at byte 2^31, one past what an int32 offset can hold."""
    from maskrcnn_amd import ops, targets
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    if free < 4 * 2 ** 30:
        pytest.skip(f"needs 4 GB of free device memory, {free / 2 ** 30:.1f} GB are free")
    rows, side = 33, 8192
    assert (rows - 1) * side * side > 2 ** 31 - 1
    masks = torch.zeros(rows, side, side, dtype=torch.uint8, device=DEV)
    masks[rows - 1, 3000:5001, 1000:7001] = 1
    last = np.zeros((1, side, side), np.uint8)
    last[0, 3000:5001, 1000:7001] = 1
    rois = np.array([[0.30, 0.10, 0.70, 0.90], [0.36, 0.12, 0.62, 0.86], [0.0, 0.0, 1.0, 1.0], [0.5, 0.5, 0.5001, 0.5001],
                     [0.6, 0.8, 0.7, 0.9]], np.float32)
    count = 8
    rois_out = np.zeros((1, count, 4), np.float32)
    rois_out[0, :5] = rois
    gt_index = np.full((1, count), -1, np.int32)
    gt_index[0, :5] = rows - 1
    got = ops.mask_targets(masks, dev(np.array([0, rows], np.int32)), dev(rois_out), dev(gt_index), dev(np.array([5], np.int32)))
    torch.cuda.synchronize()
    want = targets.mask_targets_numpy(last, np.zeros(5, np.int64), rois)
    assert want[:4].any() and 0 < want[4].sum() < want[4].size
    assert np.array_equal(got[0, :5].cpu().numpy(), want) and not got[0, 5:].any()
