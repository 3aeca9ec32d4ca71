"""Host tests (no GPU) of the heads' training mode: the numpy restatements of the class-plane rules (maskrcnn_amd.head_train) against
float64 stock-torch autograd of the DENSE graph (F.conv2d to C planes, index the class plane, F.binary_cross_entropy), the conditions that
make the GPU tests' bit-for-bit comparisons theorems, the argument refusals that need no launch, the C ABI, losses.classifier_losses on
the CPU route against losses.head_losses, and the CPU front end from the pooled crops."""
import numpy as np
import pytest
import torch

import head_train_cases as hc
import losses_cases as lc
from maskrcnn_amd import _lib, head_train, losses
from maskrcnn_amd.head_train import (TrainableClassifier, TrainableMask, class_plane_backward_numpy, class_plane_conv_numpy,
                                     mask_plane_terms_numpy)

F32, F64, I32 = torch.float32, torch.float64, torch.int32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32 if a.itemsize == 4 else np.int64),
                                                                         b.view(np.int32 if b.itemsize == 4 else np.int64))


def test_the_case_tables_hold_what_they_say():
    for c in hc.CASES:
        ids, num = hc.ids_of(c)
        assert ids.shape == (hc.BATCH, hc.COUNT) and len(c.num) == hc.BATCH and c.cin % 4 == 0
        assert head_train.plane_status_numpy(ids, num, hc.SLOTS, c.classes).tolist() == list(c.status)
    on = {c.id: hc.active(c)[0] for c in hc.CASES}
    assert not on["empty_and_full"][0].any() and on["empty_and_full"][1].all()                 # num = 0; all P slots
    assert 4 in hc.active(hc.case("empty_and_full"))[1][1]                                      # class C - 1
    k = hc.active(hc.case("shared_class"))[1]
    assert k[0, 0] == k[0, 1] == k[1, 0] == 2 and not on["shared_class"][1, 1]                # one class in and across images; a negative
    assert on["bad_and_no_room"].tolist() == [[False, False, True], [True, True, False]]
    assert hc.case("bad_and_no_room").ids[0][hc.SLOTS] > 0 and hc.case("bad_and_no_room").num[0] > hc.SLOTS


def test_the_header_declares_the_entry_points_and_the_library_exports_them():
    names = _lib.declared_symbols()
    for name in ("mrcnn_class_plane_conv_f32", "mrcnn_class_plane_conv_backward_f32", "mrcnn_class_plane_conv_backward_workspace_bytes",
                 "mrcnn_mask_plane_loss_forward", "mrcnn_mask_plane_loss_backward", "mrcnn_mask_plane_loss_workspace_bytes"):
        assert name in names and hasattr(_lib.lib, name)
    assert _lib.header_abi_version() >= 34 and int(_lib.lib.mrcnn_abi_version()) == _lib.header_abi_version()
    protos = _lib.header_prototypes()
    assert len(protos["mrcnn_class_plane_conv_f32"][1]) == 16 and len(protos["mrcnn_class_plane_conv_backward_f32"][1]) == 20
    assert len(protos["mrcnn_mask_plane_loss_forward"][1]) == 16 and len(protos["mrcnn_mask_plane_loss_backward"][1]) == 15
    # 8 bytes per (slot, chunk of 64 pixels, channel) and per (slot, chunk); nothing for arguments the entry points refuse
    assert _lib.lib.mrcnn_class_plane_conv_backward_workspace_bytes(2, 3, 28, 28, 256) == 2 * 3 * 13 * 257 * 8
    assert _lib.lib.mrcnn_class_plane_conv_backward_workspace_bytes(2, 3, 65, 28, 256) == 0
    assert _lib.lib.mrcnn_mask_plane_loss_workspace_bytes(2, 3) == 2 * 3 * 12


def test_the_bindings_are_reached_through_ops_without_a_schema():
    from maskrcnn_amd import ops
    for name in ("class_plane_conv", "class_plane_conv_backward", "mask_plane_loss", "mask_plane_loss_backward"):
        assert callable(getattr(ops, name)) and name not in ops.__all__ and not hasattr(torch.ops.maskrcnn, name)
    import maskrcnn_amd
    assert maskrcnn_amd.head_train is head_train and "head_train" in maskrcnn_amd.__all__


def test_the_build_compiles_the_file_without_contraction():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("_b", os.path.join(os.path.dirname(_lib.PKG), "maskrcnn_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.SOURCES["mask_train.hip"] == ["-ffp-contract=off"] and "-fno-fast-math" in b.COMMON


@pytest.mark.parametrize("name", hc.NAMES)
def test_the_integer_case_is_exact_and_numpy_equals_the_dense_float64_graph(name):
    """Every product and partial sum of the act = 0 case on integer data stays below 2^24 in absolute value, so fp32 and fp64 compute it
    exactly in any order and the zero terms of the dense graph change nothing: the class-plane rule and the dense graph agree bit for bit."""
    c = hc.case(name)
    o = hc.operands(c, integer=True)
    for v in (o.x, o.w, o.bias, o.dy):
        assert torch.equal(v, v.round())
    bound = hc.conv_exactness_bound(c, o)
    assert bound < 2 ** 24, bound
    ids, num = hc.ids_of(c)
    y64, dx64, dw64, db64 = hc.dense_conv_reference(c, o, 0)
    y, z, status = class_plane_conv_numpy(o.x.numpy(), o.w.numpy(), o.bias.numpy(), ids, num, 0)
    assert y.dtype == np.float32 and status.tolist() == list(c.status)
    assert np.array_equal(y.astype(np.float64), y64.numpy()) and same_bits(y, z)
    dx, dw, db = class_plane_backward_numpy(o.dy.numpy(), None, o.x.numpy(), o.w.numpy(), ids, num, 0)
    for got, want in ((dx, dx64), (dw, dw64), (db, db64)):
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want.numpy())


@pytest.mark.parametrize("name", hc.NAMES)
@pytest.mark.parametrize("act", [0, 2])
def test_numpy_on_rounded_data_is_the_dense_float64_graph_to_rounding(name, act):
    c = hc.case(name)
    o = hc.operands(c, integer=False)
    ids, num = hc.ids_of(c)
    y64, dx64, dw64, db64 = hc.dense_conv_reference(c, o, act)
    y, z, _ = class_plane_conv_numpy(o.x.numpy(), o.w.numpy(), o.bias.numpy(), ids, num, act)
    # z: the only fp32 rounding is the last; the fp64 sum of Cin exact products is within Cin 2^-53 sum|x w| of the exact one
    if act == 0:
        absdot = torch.einsum("sijc,kc->skij", o.x.to(F64).abs(), o.w.to(F64).abs()).amax(1).numpy()
        bar = 0.5 * np.spacing(np.abs(y64.numpy()).astype(np.float32)).astype(np.float64) + c.cin * 2.0 ** -53 * absdot
        assert (np.abs(z.astype(np.float64) - y64.numpy()) <= bar).all()
    assert np.abs(y.astype(np.float64) - y64.numpy()).max() <= 4 * hc.U * max(1.0, float(y64.abs().max()))
    dx, dw, db = class_plane_backward_numpy(o.dy.numpy(), y, o.x.numpy(), o.w.numpy(), ids, num, act)
    for got, want, what in ((dx, dx64, "dx"), (dw, dw64, "dw"), (db, db64, "dbias")):
        assert np.abs(got.astype(np.float64) - want.numpy()).max() <= 8 * hc.U * max(1.0, float(want.abs().max())), what
    # the slots that are not active: +0 everywhere, and what they hold is never read
    on, _ = hc.active(c)
    off = ~on.reshape(-1)
    assert not y.view(np.int32)[off].any() and not dx.view(np.int32)[off].any()
    py, pz, _ = class_plane_conv_numpy(hc.poisoned(c, o.x).numpy(), o.w.numpy(), o.bias.numpy(), ids, num, act)
    assert same_bits(py, y)
    got = class_plane_backward_numpy(hc.poisoned(c, o.dy).numpy(), hc.poisoned(c, torch.from_numpy(y)).numpy(), hc.poisoned(c, o.x).numpy(),
                                     o.w.numpy(), ids, num, act)
    assert all(same_bits(a, b) for a, b in zip(got, (dx, dw, db)))


@pytest.mark.parametrize("name", hc.NAMES)
@pytest.mark.parametrize("reduction", ["mean", "per_image"])
def test_mask_plane_terms_numpy_is_binary_cross_entropy_on_the_class_planes(name, reduction):
    c = hc.case(name)
    ids, num = hc.ids_of(c)
    p, target = hc.probabilities(c), hc.operands(c, integer=False).target
    want, want_grad = hc.dense_bce_reference(c, p, target, reduction)
    sums, counts, status, deriv = mask_plane_terms_numpy(hc.poisoned(c, p).numpy(), hc.poisoned(c, target, per_count=True).numpy(), ids, num,
                                                         c.classes)
    on, _ = hc.active(c)
    assert counts.tolist() == [int(on[b].sum()) * c.side * c.side for b in range(hc.BATCH)] and status.tolist() == list(c.status)
    got, denominators = losses.reduce_numpy(sums[:, None], counts[:, None], reduction)
    n = max(int(counts.sum()), 1)
    assert np.abs(got[..., 0].astype(np.float64) - want.numpy()).max() <= 2 * hc.U * max(1.0, float(want.abs().max())) + n * 2.0 ** -53 * 100
    grad = losses._scaled([deriv], denominators, np.ones(1))[0]
    assert np.isfinite(grad).all() and np.abs(grad.astype(np.float64) - want_grad.numpy()).max() <= 2 * hc.U * max(1.0, float(want_grad.abs().max()))


def test_the_cpu_functions_carry_gradients_and_equal_the_numpy_rules():
    c = hc.case("shared_class")
    o = hc.operands(c, integer=False)
    ids, num = (torch.from_numpy(v) for v in hc.ids_of(c))
    x, w, bias = (v.clone().requires_grad_(True) for v in (o.x, o.w, o.bias))
    y, status = head_train.class_plane_conv(x, w, bias, ids, num, act=2)
    assert y.grad_fn is not None and not status.requires_grad and status.tolist() == list(c.status)
    loss, status = head_train.mask_plane_loss(y.view(hc.BATCH, hc.SLOTS, c.side, c.side), o.target, ids, num, "mean", c.classes)
    loss.backward()
    x64, w64, b64 = (v.detach().to(F64).requires_grad_(True) for v in (o.x, o.w, o.bias))
    on, k = hc.active(c)
    z = torch.nn.functional.conv2d(x64.permute(0, 3, 1, 2), w64[:, :, None, None], b64)
    rows = [i for i in range(hc.BATCH * hc.SLOTS) if on.reshape(-1)[i]]
    pred = torch.stack([torch.sigmoid(z[i, int(k.reshape(-1)[i])]) for i in rows])
    want = torch.nn.functional.binary_cross_entropy(pred, torch.stack([o.target[i // hc.SLOTS, i % hc.SLOTS].to(F64) for i in rows]))
    want.backward()
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-6 * max(1.0, float(want.detach()))
    for got, ref, what in ((x, x64, "x"), (w, w64, "w"), (bias, b64, "bias")):
        assert float((got.grad.to(F64) - ref.grad).abs().max()) <= 1e-6 * max(1.0, float(ref.grad.abs().max())), what
    with pytest.raises(ValueError, match=r"mask_plane_loss: reduction='sum' must be one of"):
        head_train.mask_plane_loss(y.detach().view(hc.BATCH, hc.SLOTS, c.side, c.side), o.target, ids, num, "sum")
    with pytest.raises(ValueError, match=r"class_plane_conv: ids must be int32 or int64 \[B,count\] and num \[B\]"):
        head_train.class_plane_conv(o.x, o.w, o.bias, ids.to(F32), num)


def test_cpu_tensors_are_refused_by_the_bindings_in_the_house_words():
    from maskrcnn_amd import ops
    c = hc.case("shared_class")
    o = hc.operands(c, integer=False)
    ids, num = (torch.from_numpy(v) for v in hc.ids_of(c))
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.class_plane_conv(o.x, o.w, o.bias, ids, num)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.mask_plane_loss(hc.probabilities(c), o.target, ids, num, c.classes)
    with pytest.raises(RuntimeError, match=r"class_plane_conv: act must be 0 \(none\) or 2 \(sigmoid\), got 1"):
        ops.class_plane_conv(o.x, o.w, o.bias, ids, num, 1)
    with pytest.raises(RuntimeError, match=r"class_plane_conv_backward: needs must hold 3 flags \(dx, dw, dbias\), got 2"):
        ops.class_plane_conv_backward(o.dy, None, o.x, o.w, ids, num, 0, needs=(True, True))


@pytest.mark.parametrize("name", lc.HEAD_NAMES)
@pytest.mark.parametrize("reduction", ["mean", "per_image"])
def test_classifier_losses_on_the_cpu_are_head_losses_first_two_bit_for_bit(name, reduction):
    c = lc.head_case(name)
    t = lambda k: torch.from_numpy(np.array(c[k]))
    args = (t("ids"), t("num_rois"), t("deltas"))
    logits, pbox = t("logits").requires_grad_(True), t("pred_bbox").requires_grad_(True)
    want = losses.head_losses(*args, t("mask"), logits, pbox, t("pred_masks"), reduction=reduction, device="cpu")
    (want.class_loss.sum() + 3 * want.bbox_loss.sum()).backward()
    logits2, pbox2 = t("logits").requires_grad_(True), t("pred_bbox").requires_grad_(True)
    cls, box, status = losses.classifier_losses(*args, logits2, pbox2, reduction=reduction, device="cpu")
    (cls.sum() + 3 * box.sum()).backward()
    assert same_bits(cls.detach().numpy(), want.class_loss.detach().numpy()) and same_bits(box.detach().numpy(), want.bbox_loss.detach().numpy())
    assert torch.equal(status, want.status)
    assert same_bits(logits2.grad.numpy(), logits.grad.numpy()) and same_bits(pbox2.grad.numpy(), pbox.grad.numpy())


def test_classifier_losses_refuses_what_head_losses_refuses():
    c = lc.head_case("count8_c81_28")
    t = lambda k: torch.from_numpy(np.array(c[k]))
    with pytest.raises(ValueError, match=r"classifier_losses: reduction='sum' must be one of"):
        losses.classifier_losses(t("ids"), t("num_rois"), t("deltas"), t("logits"), t("pred_bbox"), reduction="sum", device="cpu")
    with pytest.raises(ValueError, match=r"classifier_losses: pred_bbox must be \[1, 8, 81, 4\] or \[8, 81, 4\]"):
        losses.classifier_losses(t("ids"), t("num_rois"), t("deltas"), t("logits"), t("pred_bbox")[..., :3], device="cpu")
    with pytest.raises(ValueError, match="classifier_losses: target_deltas, class_logits and pred_bbox are required"):
        losses.classifier_losses(t("ids"), t("num_rois"), t("deltas"), t("logits"))
    with pytest.raises(ValueError, match="head_losses: class_logits, pred_bbox and pred_masks are required"):      # unchanged
        losses.head_losses(t("ids"), t("num_rois"), t("deltas"), t("mask"), t("logits"), t("pred_bbox"))


# ------------------------------------------------------------------------------------------------------------------ whole head
@pytest.mark.parametrize("name", hc.HEAD_NAMES)
def test_the_separated_parameters_keep_every_relu_and_probability_off_its_edge(name):
    h = hc.head_case(name)
    maps, t = hc.head_maps(), hc.head_targets(h)
    relu, prob = hc.margins(maps, t, hc.separated_params(maps, t))
    assert relu > 1e-3 and prob > 1e-3, (relu, prob)
    levels = hc.head_levels(t["rois"])
    assert sorted(set(levels.tolist())) == [2, 3, 4, 5]
    for b in range(hc.BATCH):
        assert h.num_pos[b] <= hc.SLOTS and all(k > 0 for k in h.ids[b][:h.num_pos[b]]) and not any(h.ids[b][h.num_pos[b]:])


def test_from_state_dict_keeps_the_reference_names_and_layouts_and_freezes_batchnorm():
    sd = hc.head_params()
    cls = TrainableClassifier.from_state_dict(sd, image_area=hc.AREA)
    mask = TrainableMask.from_state_dict(sd, image_area=hc.AREA, mask_slots=hc.SLOTS)
    assert (cls.depth, cls.pool, cls.hidden, cls.num_classes) == (hc.DEPTH, hc.POOL, hc.HIDDEN, hc.CLASSES)
    assert (mask.depth, mask.num_classes, mask.slots(hc.COUNT)) == (hc.DEPTH, hc.CLASSES, hc.SLOTS)
    assert TrainableMask().slots(100) == 33 and TrainableMask().pool == 14
    names = {"classifier." + n for n, _ in cls.named_parameters()} | {"mask." + n for n, _ in mask.named_parameters()}
    buffers = {"classifier." + n for n, _ in cls.named_buffers()} | {"mask." + n for n, _ in mask.named_buffers()}
    assert names | buffers == set(sd)
    trained = {"classifier." + n for n, p in cls.named_parameters() if p.requires_grad} | {"mask." + n for n, p in mask.named_parameters() if p.requires_grad}
    assert trained == set(hc.TRAINED)
    assert tuple(mask.deconv.weight.shape) == (hc.DEPTH, hc.DEPTH, 2, 2) and tuple(mask.conv5.weight.shape) == (hc.CLASSES, hc.DEPTH, 1, 1)
    with pytest.raises(ValueError, match=r"TrainableMask: mask_slots=9 must be in 1 \.\. count = 8"):
        TrainableMask(mask_slots=9).slots(8)
    with pytest.raises(RuntimeError, match="RoIAlign has no CPU form"):
        mask.planes(hc.head_maps(), hc.detection_targets_of(hc.head_targets(hc.head_case("full_and_one"))))


@pytest.mark.parametrize("name", hc.HEAD_NAMES)
def test_the_cpu_heads_from_the_pooled_crops_agree_with_the_float64_stock_graph(name):
    h = hc.head_case(name)
    maps, t = hc.head_maps(), hc.head_targets(h)
    sd = hc.separated_params(maps, t)
    want_cls, want_box, want_mask, m64, sd64 = hc.stock_losses(h, maps, t, sd)
    cls = TrainableClassifier.from_state_dict(sd, image_area=hc.AREA)
    mask = TrainableMask.from_state_dict(sd, image_area=hc.AREA, mask_slots=hc.SLOTS)
    fms = [m.clone().requires_grad_(True) for m in maps]
    num_rois = t["num_pos"] + t["num_neg"]
    logits, bbox = cls.head(hc.pooled64(fms, t["rois"], hc.POOL))
    got_cls, got_box, status = losses.classifier_losses(t["ids"], num_rois, t["deltas"], logits, bbox, device="cpu")
    planes, mask_status = mask.planes_from_pooled(hc.pooled64(fms, t["rois"][:, :hc.SLOTS], hc.POOL), t["ids"], num_rois)
    got_mask, _ = head_train.mask_plane_loss(planes.view(hc.BATCH, hc.SLOTS, 2 * hc.POOL, 2 * hc.POOL), t["mask"], t["ids"], num_rois, "mean", hc.CLASSES)
    (got_cls + got_box + got_mask).backward()
    assert status.tolist() == [0, 0] and mask_status.tolist() == [0, 0]
    tol = lambda w: 1e-4 * max(1.0, float(w.abs().max()))
    for got, want, what in ((got_cls, want_cls, "class"), (got_box, want_box, "box"), (got_mask, want_mask, "mask")):
        assert abs(float(got.detach()) - float(want)) <= tol(want), what
    for l, (f, m) in enumerate(zip(fms, m64)):
        assert float((f.grad.to(F64) - m.grad).abs().max()) <= tol(m.grad), f"map {l}"
    params = {**{"classifier." + n: p for n, p in cls.named_parameters()}, **{"mask." + n: p for n, p in mask.named_parameters()}}
    for n in hc.TRAINED:
        assert float((params[n].grad.to(F64) - sd64[n].grad).abs().max()) <= tol(sd64[n].grad), n
    assert all(params[n].grad is None for n in params if n not in hc.TRAINED)
