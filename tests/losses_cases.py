"""The cases of tests/golden/losses.npz, shared by its generator (tests/golden/make_golden_losses.py, which calls the reference's five
loss functions on them) and by test_losses_host.py / test_gpu_losses.py. The INPUTS are not stored: they are rebuilt here from the
case table and a seed (PCG64's raw doubles only); the fixture holds what the reference returned. Loaded once; nothing here is
modified by a test.

The shapes are the smallest at which the kernels can go wrong: anchors on both sides of a wave (63 / 65), of the 1024-anchor chunk
of the RPN kernels (4095 / 4097) and of several chunks (12293), positives on the chunk edges, 1 / 8 / 100 slots, 2 / 81 classes,
1x1 / 28x28 / 64x64 masks (a slot's C*mh*mw floats are written as a scalar head, 16-byte vectors and a scalar tail)."""
import functools

import numpy as np

from conftest import load_golden

RPN_CASES = (
    # name, anchors, count, [(positives, negatives) per image], kind
    ("a1", 1, 8, [(1, 0)], ""),
    ("a63", 63, 8, [(5, 20)], ""),
    ("a65", 65, 8, [(5, 20)], ""),
    ("a4095", 4095, 16, [(9, 30)], ""),
    ("a4097", 4097, 16, [(9, 30)], ""),
    ("a12293", 12293, 128, [(60, 68)], ""),
    ("b3_a65", 65, 8, [(5, 20), (0, 10), (0, 0)], ""),                 # an image with no positive, one with no anchor at all
    ("b3_a4097", 4097, 16, [(0, 0), (9, 30), (0, 12)], ""),
    ("b3_a12293", 12293, 128, [(60, 68), (33, 95), (64, 64)], ""),
    ("exact_count", 4097, 8, [(8, 24)], ""),
    ("over_count", 4097, 8, [(11, 24)], ""),                            # status bit 0: the reference on the first 8
    ("b3_over_count", 65, 8, [(11, 5), (8, 5), (3, 0)], ""),
    ("all_positive_a65", 65, 128, [(65, 0)], ""),
    ("nonfinite_neutral", 4097, 16, [(9, 30)], "nonfinite"),
    ("saturating", 65, 32, [(24, 24)], "saturating"),                   # |d| exactly 1 (and one ulp either side), logits +-80
)

HEAD_CASES = (
    # name, count, classes, (mh, mw), [(num_rois, positives) per image], kind
    ("count1_c2_1x1", 1, 2, (1, 1), [(1, 1)], ""),
    ("count8_c81_28", 8, 81, (28, 28), [(6, 2)], ""),
    ("count100_c81_28", 100, 81, (28, 28), [(80, 5)], ""),
    ("count8_c2_64", 8, 2, (64, 64), [(8, 2)], ""),
    ("count8_c81_1x1", 8, 81, (1, 1), [(8, 3)], ""),
    ("b3_count8_c81_28", 8, 81, (28, 28), [(6, 2), (0, 0), (5, 0)], "padding_nan"),   # num_rois < count, num_rois = 0, negatives only
    ("b3_count100_c2_1x1", 100, 2, (1, 1), [(100, 33), (67, 20), (1, 1)], ""),
    ("negatives_only", 8, 81, (28, 28), [(8, 0)], ""),
    ("empty", 8, 2, (28, 28), [(0, 0)], "padding_nan"),
    ("bad_class", 8, 81, (28, 28), [(6, 3)], "bad_class"),                             # a class id of C: status bit 1
    ("prob01_matching", 8, 2, (28, 28), [(8, 2)], "prob01_matching"),                  # p == y in {0, 1}
    ("prob01_opposing", 8, 2, (28, 28), [(8, 2)], "prob01_opposing"),                  # p == 1 - y: the -100 clamp, the 1e-12 denominator
    ("targets_half", 8, 81, (28, 28), [(8, 2)], "half"),                               # y = 0.5
)


def _uniform(rng, lo, hi, shape):
    return (lo + (hi - lo) * rng.random(shape)).astype(np.float32)


def _order(rng, n):
    return np.argsort(rng.random(n), kind="stable")


def rpn_inputs(index: int):
    """→ dict(name, batch, anchors, count, match int32 [B,A], logits [B,A,2], pred [B,A,4], target [B,count,4])."""
    name, a, count, images, kind = RPN_CASES[index]
    rng = np.random.default_rng(7100 + index)
    b = len(images)
    match = np.zeros((b, a), np.int32)
    logits, pred = _uniform(rng, -8, 8, (b, a, 2)), _uniform(rng, -8, 8, (b, a, 4))
    target = _uniform(rng, -8, 8, (b, count, 4))
    edges = [e for e in dict.fromkeys([0, a - 1, 1023, 1024, 2047, 2048, 63, 64]) if 0 <= e < a]
    for i, (npos, nneg) in enumerate(images):
        rest = _order(rng, a)
        order = np.array(edges + [r for r in rest.tolist() if r not in edges], np.int64)
        match[i, order[:npos]] = 1
        match[i, order[npos:npos + nneg]] = -1
        target[i, min(npos, count):] = 0                       # as rpn_deltas pads
    if kind == "nonfinite":
        neutral, negative = np.where(match[0] == 0)[0], np.where(match[0] == -1)[0]
        logits[0, neutral[0]] = np.nan
        logits[0, neutral[1], 1] = np.inf
        logits[0, neutral[2], 0] = -np.inf
        pred[0, neutral[3]] = np.nan
        pred[0, neutral[4], 2] = np.inf
        pred[0, negative[0]] = np.nan                          # a negative is in the class loss, not in the box loss
        pred[0, negative[1], 0] = -np.inf
    if kind == "saturating":
        target[0] = np.round(target[0] * 4) / 4
        one = np.float32(1)
        pos = np.where(match[0] == 1)[0]
        for k, anchor in enumerate(pos[:count]):
            t = target[0, k]
            sign = np.where((np.arange(4) + k) % 2 == 0, one, -one)
            d = (one, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)))[k % 3]      # where t's ulp allows it
            pred[0, anchor] = t + sign * d
        for k, anchor in enumerate(np.where(match[0] != 0)[0]):
            logits[0, anchor] = (80, -80) if k % 2 else (-80, 80)
    return dict(name=name, batch=b, anchors=a, count=count, match=match, logits=logits, pred=pred, target=target)


def head_inputs(index: int):
    """→ dict(name, batch, count, classes, mask_shape, ids int32 [B,count], num_rois int32 [B], deltas [B,count,4], mask
    [B,count,mh,mw], logits [B,count,C], pred_bbox [B,count,C,4], pred_masks [B,count,C,mh,mw])."""
    name, count, classes, (mh, mw), images, kind = HEAD_CASES[index]
    rng = np.random.default_rng(8200 + index)
    b = len(images)
    ids, num_rois = np.zeros((b, count), np.int32), np.array([n for n, _ in images], np.int32)
    deltas = _uniform(rng, -8, 8, (b, count, 4))
    mask = (rng.random((b, count, mh, mw)) < 0.5).astype(np.float32)
    logits, pred_bbox = _uniform(rng, -8, 8, (b, count, classes)), _uniform(rng, -8, 8, (b, count, classes, 4))
    pred_masks = _uniform(rng, 1e-6, 1 - 1e-6, (b, count, classes, mh, mw))
    pred_masks = np.clip(pred_masks, np.float32(1e-6), np.float32(1 - 1e-6))
    for i, (n, npos) in enumerate(images):
        slots = _order(rng, n)[:npos]
        ids[i, slots] = 1 + np.floor(rng.random(npos) * (classes - 1)).astype(np.int32)
        deltas[i, n:], mask[i, n:] = 0, 0
    if kind == "padding_nan":
        for i, (n, _) in enumerate(images):
            logits[i, n:], pred_bbox[i, n:], pred_masks[i, n:] = np.nan, np.inf, np.nan
            ids[i, n:n + 1] = 1                                # whatever a padding slot holds
            for s in np.where(ids[i, :n] > 0)[0]:              # another class's row and plane of a positive slot
                other = (ids[i, s] + 1) % classes
                pred_bbox[i, s, other], pred_masks[i, s, other] = np.nan, np.nan
    if kind == "bad_class":
        ids[0, np.where(ids[0, :images[0][0]] == 0)[0][0]] = classes
        ids[0, np.where(ids[0, :images[0][0]] > 0)[0][0]] = -2
    for s in np.where(ids[0] > 0)[0] if kind.startswith("prob01") or kind == "half" else ():
        if kind == "half":
            mask[0, s] = 0.5
        else:
            pred_masks[0, s, ids[0, s]] = mask[0, s] if kind == "prob01_matching" else 1 - mask[0, s]
    return dict(name=name, batch=b, count=count, classes=classes, mask_shape=(mh, mw), ids=ids, num_rois=num_rois, deltas=deltas, mask=mask,
                logits=logits, pred_bbox=pred_bbox, pred_masks=pred_masks)


def head_slots(c, image: int):
    """(slots in the class loss, slots in the box and mask losses) of an image, from the case's own definition."""
    ids = c["ids"][image].astype(np.int64)
    valid = np.arange(c["count"]) < c["num_rois"][image]
    use = np.where(valid & (ids >= 0) & (ids < c["classes"]))[0]
    return use, use[ids[use] > 0]


def rpn_used(c, image: int):
    """(anchors in the class loss, positives that have a target row) of an image."""
    m = c["match"][image]
    return np.where(m != 0)[0], np.where(m == 1)[0][:c["count"]]


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _dense(shape, where, values):
    out = np.zeros(shape, np.float32)
    out[where] = values
    return out


@functools.lru_cache(maxsize=None)
def rpn_cases():
    """The inputs plus what the fixture holds. Per reduction r in ("mean", "per_image"): ref64_r / ref32_r (losses: the reference in
    float64 / float32), grad_logits_r / grad_bbox_r (the float64 reference's gradients narrowed to float32, dense)."""
    z = load_golden("losses")
    out = []
    for i in range(len(RPN_CASES)):
        c, p = rpn_inputs(i), f"r{i}_"
        assert str(z["rpn_names"][i]) == c["name"]
        c.update(counts=z[p + "counts"], status=z[p + "status"])
        nz = np.concatenate([k * c["anchors"] + rpn_used(c, k)[0] for k in range(c["batch"])])
        used = np.concatenate([k * c["anchors"] + rpn_used(c, k)[1] for k in range(c["batch"])])
        for r in ("mean", "per_image"):
            c["ref64_" + r], c["ref32_" + r] = z[p + "ref64_" + r], z[p + "ref32_" + r]
            c["grad_logits_" + r] = _dense((c["batch"] * c["anchors"], 2), nz, z[p + "g_logits_" + r]).reshape(c["logits"].shape)
            c["grad_bbox_" + r] = _dense((c["batch"] * c["anchors"], 4), used, z[p + "g_bbox_" + r]).reshape(c["pred"].shape)
        out.append(_freeze(c))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def head_cases():
    z = load_golden("losses")
    out = []
    for i in range(len(HEAD_CASES)):
        c, p = head_inputs(i), f"h{i}_"
        assert str(z["head_names"][i]) == c["name"]
        c.update(counts=z[p + "counts"], status=z[p + "status"])
        rows = [(k, s, int(c["ids"][k, s])) for k in range(c["batch"]) for s in head_slots(c, k)[1]]
        where = tuple(np.array([r[j] for r in rows], np.int64) for j in range(3))
        for r in ("mean", "per_image"):
            c["ref64_" + r], c["ref32_" + r] = z[p + "ref64_" + r], z[p + "ref32_" + r]
            c["grad_logits_" + r] = z[p + "g_logits_" + r].reshape(c["logits"].shape)
            c["grad_bbox_" + r] = _dense(c["pred_bbox"].shape, where, z[p + "g_bbox_" + r])
            c["grad_masks_" + r] = _dense(c["pred_masks"].shape, where, z[p + "g_masks_" + r])
        out.append(_freeze(c))
    return tuple(out)


def rpn_case(name):
    return next(c for c in rpn_cases() if c["name"] == name)


def head_case(name):
    return next(c for c in head_cases() if c["name"] == name)


RPN_NAMES = tuple(c[0] for c in RPN_CASES)
HEAD_NAMES = tuple(c[0] for c in HEAD_CASES)


# ----------------------------------------------------------------------------------------------------------------------
# The bars. Derived, not measured: the rule is evaluated in float64 and narrowed once; the float64 reference does the same with
# another libm and another order of summation — a few float64 roundings (<= 1e-14 absolute on terms of magnitude <= 100) and one
# double rounding at the narrowing.
# ----------------------------------------------------------------------------------------------------------------------
def ulp32(v):
    """The float32 unit in the last place at |v| (v float32 or float64)."""
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def assert_within_one_ulp(got, want, what: str):
    """|got - want| <= 1 float32 ulp of the fixture value + 1e-14, element by element; exact zeros wherever the fixture's are."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bar = ulp32(want) + 1e-14
    worst = float((err / bar).max()) if err.size else 0.0
    print(f"{what}: largest error {worst:.3f} of the bar over {err.size} values")
    assert (err <= bar).all(), f"{what}: {int((err > bar).sum())} of {err.size} values beyond 1 ulp + 1e-14, worst {worst:.3f} x the bar"
    if want.dtype == np.float32:
        zero = want == 0
        assert not got[zero].any(), f"{what}: {int((got[zero] != 0).sum())} non-zero values where the fixture has exact zeros"


def assert_losses(got, c, reduction: str, what: str):
    """got float32 [k] or [B,k] against the case's float64 reference: within 1 ulp + 1e-14, and at least as close as the reference's
    own float32 result plus one ulp."""
    got = np.asarray(got)
    assert got.dtype == np.float32
    ref64, ref32 = c["ref64_" + reduction], c["ref32_" + reduction]
    assert_within_one_ulp(got.astype(np.float64), ref64, f"{what} {c['name']} {reduction} losses")
    err, own = np.abs(got.astype(np.float64) - ref64), np.abs(ref32.astype(np.float64) - ref64)
    assert (err <= own + ulp32(ref64)).all(), f"{what} {c['name']} {reduction}: errors {err} against the reference's own {own}"
