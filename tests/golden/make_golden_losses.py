#!/usr/bin/env python3
"""Regenerates tests/golden/losses.npz from the reference's own five loss functions.

    python tests/golden/make_golden_losses.py      (reference tree: $MASKRCNN_REFERENCE, as for make_golden.py)

Loads the reference through make_golden.load_reference() and calls RPN.class_loss, RPN.boxes_loss, Classifier.class_loss,
Classifier.boxes_loss and Mask.mask_loss (model.py:652-718, 802-845, 922-953) with self=None — none of them uses it — on the cases
of tests/losses_cases.py, twice each: on float32 tensors (ref32) and on the same values as float64 with requires_grad (ref64 and
torch.autograd.grad of each loss, stored narrowed to float32).

"mean": for B > 1 the functions are given the concatenation of the images. RPN.class_loss takes [B,A,...] natively; RPN.boxes_loss
reads target_bbox[0], so the images are concatenated along the anchor axis into one [1, B*A, ...] call with the positives' target
rows concatenated; the head functions take the images' slots below num_rois, concatenated. "per_image": one call per image.
What the reference is NOT asked:
  * a loss without a contributing element. The reference's stock losses return NaN there (the mean of nothing; its head functions
    return 0 for an empty input only); the library defines 0 with zero gradients, and that is what the fixture holds.
  * elements the rule leaves out: a positive anchor whose rank is >= count (the reference would pair pred rows with fewer target rows
    and fail; it is given the first `count` positives), a slot whose class id is outside 0 .. C-1 (F.cross_entropy raises).
counts and status come from the case's own definition (losses_cases.rpn_used / head_slots), not from the code under test. The
generator ends by checking the numpy route of maskrcnn_amd.losses against what it stored, under the tests' bars.

DATA only. Inputs are NOT stored (losses_cases rebuilds them from seeds). Per RPN case i: r<i>_counts int32 [B,2], r<i>_status int32
[B], and per reduction r: r<i>_ref64_<r> float64 [2] / [B,2], r<i>_ref32_<r> float32, r<i>_g_logits_<r> float32 [n,2] (the anchors
with match != 0, image after image in ascending index), r<i>_g_bbox_<r> float32 [p,4] (the positives that have a target row). Per
head case i: h<i>_counts int32 [B,3], h<i>_status, h<i>_ref64_<r> / _ref32_<r> [3] / [B,3], h<i>_g_logits_<r> float32 [B,count,C],
h<i>_g_bbox_<r> float32 [p,4] and h<i>_g_masks_<r> float32 [p,mh,mw] (the positive slots' class row and plane). Every other gradient
element is an exact zero (asserted here).
"""
import importlib.util
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import losses_cases as lc  # noqa: E402


def call(fn, floats, others, dtype):
    """fn(*args) with the float arrays as tensors of `dtype` (requiring grad when float64) → (loss as float, gradients or None)."""
    tensors = [torch.from_numpy(np.array(v)).to(dtype) for v in floats]
    if dtype == torch.float64:
        for t in tensors:
            t.requires_grad_(True)
    loss = fn(*tensors, *others).reshape(())
    assert torch.isfinite(loss), "the reference returned a non-finite loss: fix the case"
    grads = None
    if dtype == torch.float64:
        grads = [np.zeros(t.shape) if g is None else g.numpy() for t, g in
                 zip(tensors, torch.autograd.grad(loss, tensors, allow_unused=True) if loss.requires_grad else [None] * len(tensors))]
    return (loss.item() if dtype == torch.float64 else np.float32(loss.item())), grads


def both(fn, floats, others):
    """(ref64, ref32, float64 gradients of the float arrays)."""
    ref64, grads = call(fn, floats, others, torch.float64)
    ref32, _ = call(fn, floats, others, torch.float32)
    return ref64, ref32, grads


def rpn_reference(rmodel, c, images):
    """The two RPN losses over these images as ONE reference call each → (ref64 [2], ref32 [2], g_logits [n,2], g_bbox [p,4])."""
    match = c["match"][images]                                            # [b,A]
    logits, pred = c["logits"][images], c["pred"][images]
    sel = [lc.rpn_used(c, k) for k in images]
    ref64, ref32 = np.zeros(2), np.zeros(2, np.float32)
    g_logits, g_bbox = np.zeros((sum(len(nz) for nz, _ in sel), 2)), np.zeros((sum(len(u) for _, u in sel), 4))
    if len(g_logits):
        m = torch.from_numpy(match.astype(np.int64))[:, :, None]
        ref64[0], ref32[0], (g,) = both(lambda x, mm: rmodel.RPN.class_loss(None, mm, x), [logits], [m])
        g_logits = np.concatenate([g[j][nz] for j, (nz, _) in enumerate(sel)])
        assert np.count_nonzero(g) == np.count_nonzero(g_logits)
    if len(g_bbox):
        # one [1, b*A] call: the positives beyond `count` rows are not positives for this function
        flat = np.zeros(match.shape, np.int64)
        for j, (_, used) in enumerate(sel):
            flat[j, used] = 1
        m = torch.from_numpy(flat.reshape(1, -1, 1))
        rows = np.concatenate([c["target"][k][:len(used)] for k, (_, used) in zip(images, sel)])
        fn = lambda p, t, mm: rmodel.RPN.boxes_loss(None, t, mm, p)
        ref64[1], ref32[1], (g, _) = both(fn, [pred.reshape(1, -1, 4), rows[None]], [m])
        g = g.reshape(pred.shape)
        g_bbox = np.concatenate([g[j][used] for j, (_, used) in enumerate(sel)])
        assert np.count_nonzero(g) == np.count_nonzero(g_bbox)
    return ref64, ref32, g_logits, g_bbox


def head_reference(rmodel, c, images):
    """The three head losses over these images → (ref64 [3], ref32 [3], g_logits [b,count,C], g_bbox [p,4], g_masks [p,mh,mw])."""
    sel = [lc.head_slots(c, k) for k in images]
    mh, mw = c["mask_shape"]
    ref64, ref32 = np.zeros(3), np.zeros(3, np.float32)
    g_logits = np.zeros((len(images), c["count"], c["classes"]))
    npos = sum(len(p) for _, p in sel)
    g_bbox, g_masks = np.zeros((npos, 4)), np.zeros((npos, mh, mw))
    cat = lambda name, which: np.concatenate([c[name][k][s[which]] for k, s in zip(images, sel)])
    ids = torch.from_numpy(cat("ids", 0).astype(np.int32))
    if len(ids):
        ref64[0], ref32[0], (g,) = both(lambda x, i: rmodel.Classifier.class_loss(None, i, x), [cat("logits", 0)], [ids])
        at = 0
        for j, (use, _) in enumerate(sel):
            g_logits[j, use] = g[at:at + len(use)]
            at += len(use)
    if npos:
        # the slots in the class loss, as the reference gets them from mrn_samples: its own nonzero(ids > 0) picks the positives
        fn = lambda p, t, i: rmodel.Classifier.boxes_loss(None, i, t, p)
        ref64[1], ref32[1], (g, _) = both(fn, [cat("pred_bbox", 0), cat("deltas", 0)], [ids])
        rows = np.where(ids.numpy() > 0)[0]
        g_bbox = g[rows, ids.numpy()[rows]]
        assert np.count_nonzero(g) == np.count_nonzero(g_bbox)
        fn = lambda p, t, i: rmodel.Mask.mask_loss(None, i, t, p)
        ref64[2], ref32[2], (g, _) = both(fn, [cat("pred_masks", 0), cat("mask", 0)], [ids])
        g_masks = g[rows, ids.numpy()[rows]]
        assert np.count_nonzero(g) == np.count_nonzero(g_masks)
    return ref64, ref32, g_logits, g_bbox, g_masks


def family(rmodel, prefix, cases, reference, arrays):
    for i, c in enumerate(cases):
        p = f"{prefix}{i}_"
        every = list(range(c["batch"]))
        mean = reference(rmodel, c, every)
        per = [reference(rmodel, c, [k]) for k in every]
        arrays[p + "ref64_mean"], arrays[p + "ref32_mean"] = mean[0], mean[1]
        arrays[p + "ref64_per_image"], arrays[p + "ref32_per_image"] = np.stack([r[0] for r in per]), np.stack([r[1] for r in per])
        for j, name in enumerate(("g_logits", "g_bbox", "g_masks")[:len(mean) - 2]):
            arrays[p + name + "_mean"] = mean[2 + j].astype(np.float32)
            arrays[p + name + "_per_image"] = np.concatenate([r[2 + j] for r in per]).astype(np.float32)
        print(f"{c['name']}: mean {mean[0]}  |ref32 - ref64| {np.abs(mean[1].astype(np.float64) - mean[0])}")


def main():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    _, _, _, _, rmodel = mg.load_reference()
    rpn, head = [lc.rpn_inputs(i) for i in range(len(lc.RPN_CASES))], [lc.head_inputs(i) for i in range(len(lc.HEAD_CASES))]
    arrays = dict(rpn_names=np.array(lc.RPN_NAMES), head_names=np.array(lc.HEAD_NAMES))
    for i, c in enumerate(rpn):
        sel = [lc.rpn_used(c, k) for k in range(c["batch"])]
        arrays[f"r{i}_counts"] = np.array([[len(nz), 4 * len(u)] for nz, u in sel], np.int32)
        arrays[f"r{i}_status"] = np.array([int((c["match"][k] == 1).sum() > c["count"]) for k in range(c["batch"])], np.int32)
    for i, c in enumerate(head):
        sel = [lc.head_slots(c, k) for k in range(c["batch"])]
        hw = c["mask_shape"][0] * c["mask_shape"][1]
        arrays[f"h{i}_counts"] = np.array([[len(u), 4 * len(p), hw * len(p)] for u, p in sel], np.int32)
        valid = [c["ids"][k][:c["num_rois"][k]] for k in range(c["batch"])]
        arrays[f"h{i}_status"] = np.array([2 * int(((v < 0) | (v >= c["classes"])).any()) for v in valid], np.int32)
    family(rmodel, "r", rpn, rpn_reference, arrays)
    family(rmodel, "h", head, head_reference, arrays)
    arrays.update(numpy_version=np.array(np.__version__), torch_version=np.array(torch.__version__))
    mg.save("losses", **arrays)

    # the numpy route against what was just stored, under the tests' bars
    lc.rpn_cases.cache_clear()
    lc.head_cases.cache_clear()
    from maskrcnn_amd import losses
    for c in lc.rpn_cases():
        for r in ("mean", "per_image"):
            got = losses.rpn_losses_numpy(c["match"], c["logits"], c["pred"], c["target"], r)
            lc.assert_losses(got[0], c, r, "numpy")
            assert np.array_equal(got[1], c["counts"]) and np.array_equal(got[2], c["status"])
            lc.assert_within_one_ulp(got[3], c["grad_logits_" + r], f"{c['name']} {r} grad_logits")
            lc.assert_within_one_ulp(got[4], c["grad_bbox_" + r], f"{c['name']} {r} grad_bbox")
    for c in lc.head_cases():
        for r in ("mean", "per_image"):
            got = losses.head_losses_numpy(c["ids"], c["num_rois"], c["deltas"], c["mask"], c["logits"], c["pred_bbox"], c["pred_masks"], r)
            lc.assert_losses(got[0], c, r, "numpy")
            assert np.array_equal(got[1], c["counts"]) and np.array_equal(got[2], c["status"])
            for k, name in enumerate(("grad_logits", "grad_bbox", "grad_masks")):
                lc.assert_within_one_ulp(got[3 + k], c[name + "_" + r], f"{c['name']} {r} {name}")


if __name__ == "__main__":
    main()
