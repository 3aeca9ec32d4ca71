"""The training losses without a GPU: the numpy route of maskrcnn_amd.losses against what the reference's own five loss functions
returned (tests/golden/losses.npz, made by tests/golden/make_golden_losses.py) under the bars of losses_cases — every loss and
every gradient element within 1 fp32 ulp of the fixture value + 1e-14, exact zeros where the fixture has them, every loss at least
as close to the float64 reference as the reference's own float32 result plus one ulp — which checks the fixture and the bars here;
plus the header's declarations, the library's exports and argument checks, and the ops' refusal of CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import ROOT
from losses_cases import (HEAD_NAMES, RPN_NAMES, assert_losses, assert_within_one_ulp, head_case, head_cases, head_slots, rpn_case,
                          rpn_cases, rpn_used)

ENTRY_POINTS = ("mrcnn_rpn_loss_forward", "mrcnn_rpn_loss_backward", "mrcnn_head_loss_forward", "mrcnn_head_loss_backward")
REDUCTIONS = ("mean", "per_image")
HEAD_GRADS = ("grad_logits", "grad_bbox", "grad_masks")


def head_args(c):
    return c["ids"], c["num_rois"], c["deltas"], c["mask"], c["logits"], c["pred_bbox"], c["pred_masks"]


def test_fixture_covers_the_cases():
    assert {c["anchors"] for c in rpn_cases()} >= {1, 63, 65, 4095, 4097, 12293} and {c["batch"] for c in rpn_cases()} == {1, 3}
    b3 = rpn_case("b3_a65")
    assert b3["counts"].tolist() == [[25, 20], [10, 0], [0, 0]]                        # no positive; no contributing anchor at all
    assert rpn_case("exact_count")["counts"][0, 1] == 4 * 8 and rpn_case("exact_count")["status"].tolist() == [0]
    over = rpn_case("over_count")
    assert (over["match"] == 1).sum() == over["count"] + 3 and over["status"].tolist() == [1] and over["counts"].tolist() == [[35, 32]]
    assert rpn_case("b3_over_count")["status"].tolist() == [1, 0, 0]
    assert (rpn_case("all_positive_a65")["match"] == 1).all()
    for c in rpn_cases():                                                            # positives on the chunk and wave edges
        if c["anchors"] > 2048 and (c["match"][0] == 1).sum() >= 8:
            assert (c["match"][0, [0, 1023, 1024, 2047, 2048, c["anchors"] - 1]] == 1).all()
    n = rpn_case("nonfinite_neutral")
    neutral = n["match"][0] == 0
    assert np.isnan(n["logits"][0][neutral]).any() and np.isinf(n["logits"][0][neutral]).any()
    assert np.isnan(n["pred"][0][neutral]).any() and np.isinf(n["pred"][0][neutral]).any() and np.isnan(n["pred"][0][n["match"][0] == -1]).any()
    assert np.isfinite(n["logits"][0][~neutral]).all() and np.isfinite(n["pred"][0][n["match"][0] == 1]).all()
    s = rpn_case("saturating")
    d = np.abs(s["pred"][0][rpn_used(s, 0)[1]] - s["target"][0][:len(rpn_used(s, 0)[1])])
    assert (d == 1).any() and (np.abs(s["logits"][0][s["match"][0] != 0]) == 80).all()
    assert {c["count"] for c in head_cases()} == {1, 8, 100} and {c["classes"] for c in head_cases()} == {2, 81}
    assert {c["mask_shape"] for c in head_cases()} == {(1, 1), (28, 28), (64, 64)} and {c["batch"] for c in head_cases()} == {1, 3}
    b3 = head_case("b3_count8_c81_28")
    assert b3["num_rois"].tolist() == [6, 0, 5] and b3["counts"][:, 0].tolist() == [6, 0, 5] and b3["counts"][2].tolist() == [5, 0, 0]
    assert np.isnan(b3["logits"][0, 6:]).all() and np.isnan(b3["pred_masks"][1]).all() and b3["ids"][1, 0] == 1
    bad = head_case("bad_class")
    assert (bad["ids"][0, :6] == 81).sum() == 1 and (bad["ids"][0, :6] < 0).sum() == 1 and bad["status"].tolist() == [2]
    assert bad["counts"].tolist() == [[4, 8, 2 * 784]]
    for name, same in (("prob01_matching", True), ("prob01_opposing", False)):
        c = head_case(name)
        for s in head_slots(c, 0)[1]:
            p, y = c["pred_masks"][0, s, c["ids"][0, s]], c["mask"][0, s]
            assert set(np.unique(p).tolist()) == {0.0, 1.0} and ((p == y) == same).all()
    assert head_case("prob01_opposing")["ref64_mean"][2] == 100.0 and head_case("prob01_matching")["ref64_mean"][2] == 0.0
    g = head_case("prob01_opposing")["grad_masks_mean"]
    assert np.abs(g[g != 0]).min() > 1e12 / (2 * 784) * 0.999                          # +-1e12 / n by definition
    half = head_case("targets_half")
    assert (half["mask"][0, head_slots(half, 0)[1]] == 0.5).all()


@pytest.mark.parametrize("name", RPN_NAMES)
def test_rpn_numpy_route_equals_the_fixture(name):
    from maskrcnn_amd import losses
    c = rpn_case(name)
    for r in REDUCTIONS:
        got = losses.rpn_losses_numpy(c["match"], c["logits"], c["pred"], c["target"], r)
        assert_losses(got[0], c, r, "numpy")
        assert got[1].dtype == np.int32 and np.array_equal(got[1], c["counts"]) and np.array_equal(got[2], c["status"])
        assert_within_one_ulp(got[3], c["grad_logits_" + r], f"{name} {r} grad_logits")
        assert_within_one_ulp(got[4], c["grad_bbox_" + r], f"{name} {r} grad_bbox")


@pytest.mark.parametrize("name", HEAD_NAMES)
def test_head_numpy_route_equals_the_fixture(name):
    from maskrcnn_amd import losses
    c = head_case(name)
    for r in REDUCTIONS:
        got = losses.head_losses_numpy(*head_args(c), r)
        assert_losses(got[0], c, r, "numpy")
        assert got[1].dtype == np.int32 and np.array_equal(got[1], c["counts"]) and np.array_equal(got[2], c["status"])
        for k, g in enumerate(HEAD_GRADS):
            assert_within_one_ulp(got[3 + k], c[f"{g}_{r}"], f"{name} {r} {g}")


def leaf(a):
    return torch.from_numpy(np.array(a)).requires_grad_(True)


@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_front_end_on_the_cpu_route_with_backward(reduction):
    """losses.rpn_losses / head_losses with device="cpu": named tuples, the accepted forms of the inputs, and gradients through
    autograd; upstream gradients of 2, 4 and 8 scale the fixture's gradients exactly."""
    from maskrcnn_amd import losses, targets
    c = rpn_case("b3_over_count")
    logits, pred = leaf(c["logits"]), leaf(c["pred"])
    got = losses.rpn_losses(torch.from_numpy(c["match"].astype(np.int64))[:, :, None], logits, pred, c["target"], reduction=reduction,
                            device="cpu")
    assert got._fields == ("rpn_class_loss", "rpn_bbox_loss", "status") and got.status.dtype == torch.int32
    assert tuple(got.rpn_class_loss.shape) == (() if reduction == "mean" else (3,)) and got.rpn_class_loss.dtype == torch.float32
    assert_losses(torch.stack(got[:2], -1).detach().numpy(), c, reduction, "front end")
    assert got.status.tolist() == c["status"].tolist()
    (2 * got.rpn_class_loss.sum() + 4 * got.rpn_bbox_loss.sum()).backward()
    assert_within_one_ulp(logits.grad.numpy(), 2 * c["grad_logits_" + reduction], "front end grad_logits x 2")
    assert_within_one_ulp(pred.grad.numpy(), 4 * c["grad_bbox_" + reduction], "front end grad_bbox x 4")

    c = head_case("b3_count8_c81_28")
    flat = lambda a: a.reshape(-1, *a.shape[2:])
    logits, pbox, pmask = leaf(flat(c["logits"])), leaf(c["pred_bbox"]), leaf(flat(c["pred_masks"]))        # flat and [B,count,...] forms
    got = losses.head_losses(c["ids"].astype(np.int64), c["num_rois"], c["deltas"], c["mask"], logits, pbox, pmask, reduction, "cpu")
    assert got._fields == ("class_loss", "bbox_loss", "mask_loss", "status")
    assert_losses(torch.stack(got[:3], -1).detach().numpy(), c, reduction, "front end")
    (2 * got.class_loss.sum() + 4 * got.bbox_loss.sum() + 8 * got.mask_loss.sum()).backward()
    assert tuple(logits.grad.shape) == tuple(logits.shape) and tuple(pmask.grad.shape) == tuple(pmask.shape)
    assert_within_one_ulp(logits.grad.numpy().reshape(c["logits"].shape), 2 * c["grad_logits_" + reduction], "front end grad_logits x 2")
    assert_within_one_ulp(pbox.grad.numpy(), 4 * c["grad_bbox_" + reduction], "front end grad_bbox x 4")
    assert_within_one_ulp(pmask.grad.numpy().reshape(c["pred_masks"].shape), 8 * c["grad_masks_" + reduction], "front end grad_masks x 8")
    # a DetectionTargets in place of the four target arguments
    t = lambda a: torch.from_numpy(np.array(a))
    npos = t(np.array([len(head_slots(c, k)[1]) for k in range(3)], np.int32))
    dt = targets.DetectionTargets(torch.zeros(3, 8, 4), t(c["ids"]), t(c["deltas"]), t(c["mask"]), t(c["ids"]), t(c["ids"]), npos,
                                  t(c["num_rois"]) - npos, torch.zeros(3, dtype=torch.int32))
    again = losses.head_losses(dt, t(c["logits"]), t(c["pred_bbox"]), t(c["pred_masks"]), reduction=reduction, device="cpu")
    assert all(torch.equal(a, b.detach()) for a, b in zip(again, got))


def test_front_end_value_errors():
    from maskrcnn_amd import losses
    c, h = rpn_case("a65"), head_case("count8_c81_28")
    rpn = lambda **kw: losses.rpn_losses(**{**dict(rpn_match=c["match"], rpn_class_logits=c["logits"], rpn_pred_bbox=c["pred"],
                                                   target_bbox=c["target"], device="cpu"), **kw})
    with pytest.raises(ValueError, match="reduction='sum'"):
        rpn(reduction="sum")
    with pytest.raises(ValueError, match="rpn_match must be int32 or int64"):
        rpn(rpn_match=c["match"].astype(np.float32))
    with pytest.raises(ValueError, match=r"rpn_class_logits must be \[1,65,2\]"):
        rpn(rpn_class_logits=c["logits"][:, :64])
    with pytest.raises(ValueError, match="count in \\[1, 1024\\]"):
        rpn(target_bbox=np.zeros((1, 1025, 4), np.float32))
    head = lambda *a, **kw: losses.head_losses(*a, device="cpu", **kw)
    with pytest.raises(ValueError, match="class_logits, pred_bbox and pred_masks are required"):
        head(*head_args(h)[:4])
    with pytest.raises(ValueError, match="pred_bbox must be"):
        head(*head_args(h)[:5], h["pred_bbox"][:, :, :80], h["pred_masks"])
    with pytest.raises(ValueError, match="mh, mw in \\[1, 64\\]"):
        head(h["ids"], h["num_rois"], h["deltas"], np.zeros((1, 8, 65, 28), np.float32), *head_args(h)[4:])
    with pytest.raises(ValueError, match="C in \\[2, 4096\\]"):
        head(*head_args(h)[:4], h["logits"][:, :, :1], h["pred_bbox"][:, :, :1], h["pred_masks"][:, :, :1])


def test_header_version_and_exports():
    import maskrcnn_amd
    from maskrcnn_amd import _lib, losses, ops
    assert _lib.header_abi_version() >= 26 and int(_lib.lib.mrcnn_abi_version()) == _lib.header_abi_version()
    declared, protos = _lib.declared_symbols(), _lib.header_prototypes()
    for name in ENTRY_POINTS:
        assert name in declared and name in protos
        fn = getattr(_lib.lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == protos[name][1] and fn.argtypes[-1] is ctypes.c_void_p
    assert [len(protos[n][1]) for n in ENTRY_POINTS] == [14, 14, 18, 19]
    assert protos["mrcnn_rpn_loss_forward"][1][12] is ctypes.c_size_t and protos["mrcnn_head_loss_forward"][1][16] is ctypes.c_size_t
    for name, res in (("mrcnn_rpn_loss_workspace_bytes", ctypes.c_size_t), ("mrcnn_head_loss_workspace_bytes", ctypes.c_size_t),
                      ("mrcnn_rpn_loss_chunks", ctypes.c_int32)):
        assert name in declared and getattr(_lib.lib, name).restype is res
    lib = _lib.lib
    assert [lib.mrcnn_rpn_loss_chunks(a) for a in (0, 1, 1024, 1025, 261888, 1 << 24, (1 << 24) + 1)] == [0, 1, 1, 2, 256, 16384, 0]
    assert lib.mrcnn_rpn_loss_workspace_bytes(2, 1025, 128) == 2 * 2 * (8 + 4 * 129) and lib.mrcnn_rpn_loss_workspace_bytes(0, 8, 8) == 0
    assert lib.mrcnn_head_loss_workspace_bytes(3, 100) == 3 * 100 * 28 and lib.mrcnn_head_loss_workspace_bytes(1, 1025) == 0
    for name in ("rpn_loss", "rpn_loss_backward", "head_loss", "head_loss_backward"):
        assert name in ops.__all__ and callable(getattr(ops, name)) and hasattr(torch.ops.maskrcnn, name)
    assert maskrcnn_amd.losses is losses and "losses" in maskrcnn_amd.__all__
    for name in ("rpn_losses", "head_losses", "RpnLosses", "HeadLosses", "rpn_losses_numpy", "head_losses_numpy", "rpn_terms_numpy",
                 "head_terms_numpy"):
        assert name in losses.__all__ and hasattr(losses, name)
    header = open(_lib.HEADER).read()
    block = header[header.index("Training losses"):]
    for phrase in ("model.py:652-718", "in fp64 from the fp32 inputs", "FIXED order", "no floating-point atomic", "DEVIATION", "1e-12",
                   "max(log p, -100)", "a select, not a multiply by zero", "bit 0 of status", "bit 1 and the slot is skipped", "B * A < 2^31"):
        assert phrase in block, phrase
    build = open(f"{ROOT}/maskrcnn_amd/build.py").read()
    assert '"losses.hip": ["-ffp-contract=off"]' in build
    src = open(f"{ROOT}/maskrcnn_amd/csrc/losses.hip").read()
    assert '#include "workgroup.hpp"' in src and "atomic" not in src.split("namespace {", 1)[1]


def test_the_ops_refuse_cpu_tensors():
    from maskrcnn_amd import ops
    c, h = rpn_case("a65"), head_case("count1_c2_1x1")
    t = lambda *arrays: [torch.from_numpy(np.array(a)) for a in arrays]
    rpn = t(c["match"], c["logits"], c["pred"], c["target"])
    back = t(np.zeros((1, 1), np.int32), np.zeros((1, 2), np.int32), np.ones(2, np.float32))
    head = t(*head_args(h))
    head_back = t(np.zeros((1, 3), np.int32), np.ones(3, np.float32))
    for fn, args in ((ops.rpn_loss, rpn), (torch.ops.maskrcnn.rpn_loss, rpn), (ops.rpn_loss_backward, rpn + back),
                     (torch.ops.maskrcnn.rpn_loss_backward, rpn + back), (ops.head_loss, head), (torch.ops.maskrcnn.head_loss, head),
                     (ops.head_loss_backward, head + head_back), (torch.ops.maskrcnn.head_loss_backward, head + head_back)):
        with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
            fn(*args)


def test_the_library_validates_its_arguments():
    """Host-side checks of the C entry points, reachable without a GPU: they fail before any launch."""
    from maskrcnn_amd import _lib
    lib = _lib.lib
    p = ctypes.c_void_p(16)           # never dereferenced: every call below is refused first
    big = 1 << 40

    def rpn_forward(batch=1, a=8, count=8, first=p, ws=p):
        return lib.mrcnn_rpn_loss_forward(first, p, p, p, batch, a, count, p, p, p, p, ws, big, None)

    def rpn_backward(batch=1, a=8, count=8, first=p, ws=p):
        return lib.mrcnn_rpn_loss_backward(first, p, p, p, p, p, p, 0, batch, a, count, p, ws, None)

    def head_forward(batch=1, count=8, c=81, mh=28, mw=28, first=p, ws=p):
        return lib.mrcnn_head_loss_forward(first, p, p, p, p, p, p, batch, count, c, mh, mw, p, p, p, ws, big, None)

    def head_backward(batch=1, count=8, c=81, mh=28, mw=28, first=p, ws=p):
        return lib.mrcnn_head_loss_backward(first, p, p, p, p, p, p, p, p, 0, batch, count, c, mh, mw, p, p, ws, None)

    shared = ((dict(batch=0), "batch=0"), (dict(batch=65536), "batch=65536"), (dict(count=0), "count=0"), (dict(count=1025), "count=1025"),
              (dict(first=None), "null pointer"), (dict(ws=None), "null pointer"))
    for fn in (rpn_forward, rpn_backward):
        for kw, msg in shared + ((dict(a=0), "num_anchors=0"), (dict(a=(1 << 24) + 1), f"num_anchors={(1 << 24) + 1}"),
                                 (dict(a=1 << 24, batch=128), f"batch * num_anchors = {1 << 31}")):
            assert fn(**kw) != 0 and msg in lib.mrcnn_last_error().decode(), (fn.__name__, kw, lib.mrcnn_last_error().decode())
    for fn in (head_forward, head_backward):
        for kw, msg in shared + ((dict(c=1), "num_classes=1"), (dict(c=4097), "num_classes=4097"), (dict(mh=0), "mask_height=0"),
                                 (dict(mh=65), "mask_height=65"), (dict(mw=0), "mask_width=0"), (dict(mw=65), "mask_width=65")):
            assert fn(**kw) != 0 and msg in lib.mrcnn_last_error().decode(), (fn.__name__, kw, lib.mrcnn_last_error().decode())
    # the largest accepted values pass the range checks: the refusal that follows is the workspace's size
    assert lib.mrcnn_rpn_loss_forward(p, p, p, p, 127, 1 << 24, 1024, p, p, p, p, p, 8, None) != 0
    assert "workspace of 8 bytes" in lib.mrcnn_last_error().decode()
    assert lib.mrcnn_head_loss_forward(p, p, p, p, p, p, p, 65535, 1024, 4096, 64, 64, p, p, p, p, 8, None) != 0
    assert "workspace of 8 bytes" in lib.mrcnn_last_error().decode()
