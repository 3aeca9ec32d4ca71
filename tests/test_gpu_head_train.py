"""GPU tests (-m gpu) of the heads' training mode: ops.class_plane_conv, ops.class_plane_conv_backward, ops.mask_plane_loss and
ops.mask_plane_loss_backward (csrc/mask_train.hip), losses.classifier_losses, and the front end maskrcnn_amd.head_train.

The four ops are compared bit for bit with their rules restated in numpy (head_train.class_plane_conv_numpy / class_plane_backward_numpy /
mask_plane_terms_numpy, which tests/test_head_train_host.py ties to the dense stock-torch graph), on exact data with the float64 autograd of
that dense graph, and with the ops they replace: the sigmoid with ops.conv_bn_act's, the mask loss with ops.head_loss on a dense tensor
whose other planes are NaN, and with the mask cases of tests/golden/losses.npz. On rounded data TrainableHeads.losses(...).backward() is
held to twice the error of this project's own dense route against the float64 stock graph. The shapes are the smallest at which each
mechanism can go wrong (head_train_cases). The file runs once more in a child pytest on the schedule-fuzz library."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import head_train_cases as hc
import losses_cases as lc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ_LIB = os.path.join(ROOT, "maskrcnn_amd", "csrc", "build", "variants", "sync_fuzz", "libmaskrcnn_hip.so")
F32, F64, I32 = torch.float32, torch.float64, torch.int32
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from maskrcnn_amd import ops as o
    return o


@pytest.fixture(scope="module")
def ht():
    from maskrcnn_amd import head_train as m
    return m


def dev(t):
    return (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).contiguous().to(DEV)


def bits(t):
    t = t.detach().cpu().contiguous() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def nan_like(*shape):
    return torch.full(shape, float("nan"), dtype=F32, device=DEV)


def targets(c):
    return tuple(dev(v) for v in hc.ids_of(c))


def assert_same_bits(got, want64, what):
    """got (fp32, GPU) against a float64 expectation that fp32 holds exactly; -0 and +0 are the same number here."""
    got, want = got.detach().cpu(), want64.to(F32)
    assert torch.equal(want.to(F64), want64.to(F64)), f"{what}: the expectation is not an fp32 number"
    assert got.shape == want.shape and got.dtype == F32, (what, got.shape, want.shape)
    same = bits(got + 0.0) == bits(want + 0.0)
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} elements differ in their bits"


# -------------------------------------------------------------------------------------------------------- the class-plane conv
def backward(ops, c, o, y, act, **kw):
    ids, num = targets(c)
    s, q = hc.BATCH * hc.SLOTS, c.side
    out = (nan_like(s, q, q, c.cin), nan_like(c.classes, c.cin), nan_like(c.classes))
    got = ops.class_plane_conv_backward(dev(o.dy), None if y is None else dev(y), dev(o.x), dev(o.w), ids, num, act, out=out, **kw)
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("name", hc.NAMES)
def test_exact_data_equals_the_dense_float64_graph_bit_for_bit(ops, name):
    c = hc.case(name)
    o = hc.operands(c, integer=True)
    ids, num = targets(c)
    y64, dx64, dw64, db64 = hc.dense_conv_reference(c, o, 0)
    out = nan_like(hc.BATCH * hc.SLOTS, c.side, c.side)
    y, status = ops.class_plane_conv(dev(hc.poisoned(c, o.x)), dev(o.w), dev(o.bias), ids, num, 0, out=out)
    assert y is out and status.dtype == I32 and status.tolist() == list(c.status)
    assert_same_bits(y, y64, "y")
    poisoned = o._replace(x=hc.poisoned(c, o.x), dy=hc.poisoned(c, o.dy))
    dx, dw, db = backward(ops, c, poisoned, None, 0)
    assert_same_bits(dx, dx64, "dx")
    assert_same_bits(dw, dw64, "dw")
    assert_same_bits(db, db64, "dbias")


@pytest.mark.parametrize("name", hc.NAMES)
def test_rounded_data_equals_the_numpy_rule_bit_for_bit(ops, ht, name):
    c = hc.case(name)
    o = hc.operands(c, integer=False)
    ids, num = targets(c)
    np_ids, np_num = hc.ids_of(c)
    xp = hc.poisoned(c, o.x)
    _, z_np, status_np = ht.class_plane_conv_numpy(o.x.numpy(), o.w.numpy(), o.bias.numpy(), np_ids, np_num, 0)
    z, status = ops.class_plane_conv(dev(xp), dev(o.w), dev(o.bias), ids, num, 0, out=nan_like(hc.BATCH * hc.SLOTS, c.side, c.side))
    assert torch.equal(bits(z), bits(z_np)) and np.array_equal(status.cpu().numpy(), status_np)      # +0 for the slots that are not active
    # without a bias: the same sum, not bias 0 added
    _, z0_np, _ = ht.class_plane_conv_numpy(o.x.numpy(), o.w.numpy(), None, np_ids, np_num, 0)
    assert torch.equal(bits(ops.class_plane_conv(dev(xp), dev(o.w), None, ids, num, 0)[0]), bits(z0_np))
    # z is within half an fp32 ulp and the fp64 sum's own error of the float64 dot: the only fp32 rounding is the last
    y64, *_ = hc.dense_conv_reference(c, o, 0)
    absdot = torch.einsum("sijc,kc->skij", o.x.to(F64).abs(), o.w.to(F64).abs()).amax(1).numpy()
    bar = 0.5 * np.spacing(np.abs(y64.numpy()).astype(np.float32)).astype(np.float64) + c.cin * 2.0 ** -53 * absdot
    assert (np.abs(z.cpu().numpy().astype(np.float64) - y64.numpy()) <= bar).all()
    # the sigmoid is the conv forward's: the same z through a 4 x 4 identity 1x1 weight with act = 2
    p, _ = ops.class_plane_conv(dev(xp), dev(o.w), dev(o.bias), ids, num, 2, out=nan_like(hc.BATCH * hc.SLOTS, c.side, c.side))
    on = torch.from_numpy(hc.active(c)[0].reshape(-1))
    flat = z.reshape(-1)
    rows = torch.cat([flat, flat.new_zeros(-flat.numel() % 4)]).view(-1, 1, 1, 4)
    want = ops.conv_bn_act(rows, torch.eye(4, device=DEV).view(4, 1, 1, 4).contiguous(), None, None, relu=2).reshape(-1)[:flat.numel()]
    assert torch.equal(bits(p[on]), bits(want.view_as(p)[on])) and not bool(bits(p[~on]).any())
    # the backward from the device's own p, NaN in every row of a slot that is not active
    for act, y in ((0, None), (2, p.cpu())):
        want = ht.class_plane_backward_numpy(o.dy.numpy(), None if y is None else y.numpy(), o.x.numpy(), o.w.numpy(), np_ids, np_num, act)
        poisoned = o._replace(x=xp, dy=hc.poisoned(c, o.dy))
        got = backward(ops, c, poisoned, None if y is None else hc.poisoned(c, y), act)
        again = backward(ops, c, poisoned, None if y is None else hc.poisoned(c, y), act)
        for g, a, w, what in zip(got, again, want, ("dx", "dw", "dbias")):
            assert torch.equal(bits(g), bits(w)), f"act {act}: {what}"
            assert torch.equal(bits(g), bits(a)), f"act {act}: {what}: two calls differ"


def test_the_backward_computes_what_is_needed_and_an_image_alone_gives_the_same_bits(ops):
    c = hc.case("shared_class")
    o = hc.operands(c, integer=False)
    ids, num = targets(c)
    whole = backward(ops, c, o, None, 0)
    for needs in ((True, False, False), (False, True, False), (False, False, True), (False, True, True), (False, False, False)):
        some = backward(ops, c, o, None, 0, needs=needs)
        for g, w, need in zip(some, whole, needs):
            assert (g is not None) == need and (g is None or torch.equal(bits(g), bits(w))), needs
    for i in range(hc.BATCH):
        rows = slice(i * hc.SLOTS, (i + 1) * hc.SLOTS)
        dx, _, _ = ops.class_plane_conv_backward(dev(o.dy[rows]), None, dev(o.x[rows]), dev(o.w), ids[i:i + 1], num[i:i + 1], 0)
        assert torch.equal(bits(dx), bits(whole[0][rows])), f"image {i}"


# -------------------------------------------------------------------------------------------------------------- the mask loss
def dense_of(c, p, ids):
    """p [B,P,q,q] scattered into [B,count,C,q,q] whose other planes are NaN, and ids without the positives at or past P."""
    on, k = hc.active(c)
    dense = torch.full((hc.BATCH, hc.COUNT, c.classes, c.side, c.side), float("nan"))
    for b in range(hc.BATCH):
        for s in range(hc.SLOTS):
            if on[b, s]:
                dense[b, s, k[b, s]] = p[b, s]
    kept = torch.from_numpy(ids.copy())
    kept[:, hc.SLOTS:] = 0
    return dense, kept


@pytest.mark.parametrize("name", hc.NAMES)
def test_the_plane_loss_is_head_loss_on_the_dense_tensor(ops, ht, name):
    c = hc.case(name)
    np_ids, np_num = hc.ids_of(c)
    ids, num = targets(c)
    p, target = hc.probabilities(c), hc.operands(c, integer=False).target
    pp, tp = dev(hc.poisoned(c, p)), dev(hc.poisoned(c, target, per_count=True))
    sums, counts, status = ops.mask_plane_loss(pp, tp, ids, num, c.classes)
    again = ops.mask_plane_loss(pp, tp, ids, num, c.classes)
    assert sums.dtype == F64 and counts.dtype == I32 and status.tolist() == list(c.status)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((sums, counts, status), again))
    dense, kept = dense_of(c, p, np_ids)
    g = hc.rng(9)
    logits, pbox = torch.randn(hc.BATCH, hc.COUNT, c.classes, generator=g), torch.randn(hc.BATCH, hc.COUNT, c.classes, 4, generator=g)
    deltas = torch.randn(hc.BATCH, hc.COUNT, 4, generator=g)
    head = (dev(kept), num, dev(deltas), dev(target), dev(logits), dev(pbox), dev(dense))
    h_sums, h_counts, _ = ops.head_loss(*head)
    assert torch.equal(counts, h_counts[:, 2])
    assert torch.equal(bits(sums), bits(h_sums[:, 2].contiguous())), "the slot sum's code is shared: the sums are the dense op's bits"
    # the numpy rule: counts, status and the gradient bit for bit (the gradient is arithmetic alone)
    n_sums, n_counts, n_status, deriv = ht.mask_plane_terms_numpy(p.numpy(), target.numpy(), np_ids, np_num, c.classes)
    assert np.array_equal(counts.cpu().numpy(), n_counts) and np.array_equal(status.cpu().numpy(), n_status)
    from maskrcnn_amd import losses
    for per_image in (False, True):
        up = torch.tensor([0.75, 1.5] if per_image else [0.75], dtype=F32)
        out = nan_like(hc.BATCH, hc.SLOTS, c.side, c.side)
        grad = ops.mask_plane_loss_backward(pp, tp, ids, num, c.classes, counts, dev(up), per_image, out=out)
        assert grad is out
        up3 = torch.zeros((hc.BATCH, 3) if per_image else (3,))
        up3[..., 2] = up
        h_grad = ops.head_loss_backward(*head, h_counts, dev(up3))[2]
        on, k = hc.active(c)
        for b in range(hc.BATCH):
            for s in range(hc.SLOTS):
                want = h_grad[b, s, k[b, s]] if on[b, s] else torch.zeros(c.side, c.side)
                assert torch.equal(bits(grad[b, s]), bits(want)), (per_image, b, s)
        _, denominators = losses.reduce_numpy(n_sums[:, None], n_counts[:, None], "per_image" if per_image else "mean")
        want = losses._scaled([deriv], denominators, up.numpy().astype(np.float64).reshape(-1, 1) if per_image else up.numpy().astype(np.float64))[0]
        assert torch.equal(bits(grad), bits(want)), f"per_image {per_image}: the gradient against numpy"


@pytest.mark.parametrize("name", hc.NAMES)
def test_the_plane_loss_sums_equal_the_numpy_rule(ops, ht, name):
    """The order of the sum is the kernel's in numpy; the logarithms are each side's own libm."""
    c = hc.case(name)
    np_ids, np_num = hc.ids_of(c)
    p, target = hc.probabilities(c), hc.operands(c, integer=False).target
    sums, _, _ = ops.mask_plane_loss(dev(p), dev(target), *targets(c), c.classes)
    want, *_ = ht.mask_plane_terms_numpy(p.numpy(), target.numpy(), np_ids, np_num, c.classes)
    got = sums.cpu().numpy()
    print(f"{name}: sums {got.tolist()} numpy {want.tolist()} difference {(got - want).tolist()}")
    assert np.array_equal(got.view(np.int64), want.view(np.int64))


@pytest.mark.parametrize("name", lc.HEAD_NAMES)
def test_the_plane_loss_on_the_golden_mask_cases(ops, name):
    """The mask column of tests/golden/losses.npz with P = count, held to test_gpu_losses.py's bar for mask_loss."""
    from maskrcnn_amd import losses
    c = lc.head_case(name)
    b, count, classes = c["batch"], c["count"], c["classes"]
    mh, mw = c["mask_shape"]
    p = np.full((b, count, mh, mw), np.nan, np.float32)
    for i in range(b):
        for s in lc.head_slots(c, i)[1]:
            p[i, s] = c["pred_masks"][i, s, c["ids"][i, s]]
    args = (dev(p), dev(np.array(c["mask"])), dev(np.array(c["ids"])), dev(np.array(c["num_rois"])), classes)
    sums, counts, status = ops.mask_plane_loss(*args)
    assert np.array_equal(counts.cpu().numpy(), c["counts"][:, 2]) and np.array_equal(status.cpu().numpy(), c["status"])
    for r in ("mean", "per_image"):
        got = losses.reduce_numpy(sums.cpu().numpy()[:, None], counts.cpu().numpy()[:, None], r)[0][..., 0]
        lc.assert_within_one_ulp(got.astype(np.float64), c["ref64_" + r][..., 2], f"{name} {r} mask loss")
        up = torch.ones(b if r == "per_image" else 1, dtype=F32, device=DEV)
        grad = ops.mask_plane_loss_backward(*args, counts, up, r == "per_image").cpu().numpy()
        want = np.zeros_like(grad)
        for i in range(b):
            for s in lc.head_slots(c, i)[1]:
                want[i, s] = c["grad_masks_" + r][i, s, c["ids"][i, s]]
        lc.assert_within_one_ulp(grad, want, f"{name} {r} grad_p")


@pytest.mark.parametrize("name", ["count8_c81_28", "b3_count8_c81_28", "b3_count100_c2_1x1", "bad_class", "empty"])
def test_classifier_losses_are_head_losses_class_and_box_bit_for_bit(ops, name):
    from maskrcnn_amd import losses
    c = lc.head_case(name)
    t = lambda k: dev(np.array(c[k]))
    for r in ("mean", "per_image"):
        logits, pbox = t("logits").requires_grad_(True), t("pred_bbox").requires_grad_(True)
        pm = torch.where(torch.isnan(t("pred_masks")), torch.full_like(t("pred_masks"), 0.5), t("pred_masks"))
        want = losses.head_losses(t("ids"), t("num_rois"), t("deltas"), t("mask"), logits, pbox, pm, reduction=r)
        (2 * want.class_loss.sum() + 4 * want.bbox_loss.sum()).backward()
        logits2, pbox2 = t("logits").requires_grad_(True), t("pred_bbox").requires_grad_(True)
        cls, box, status = losses.classifier_losses(t("ids"), t("num_rois"), t("deltas"), logits2, pbox2, reduction=r)
        (2 * cls.sum() + 4 * box.sum()).backward()
        assert torch.equal(bits(cls), bits(want.class_loss)) and torch.equal(bits(box), bits(want.bbox_loss)) and torch.equal(status, want.status)
        assert torch.equal(bits(logits2.grad), bits(logits.grad)) and torch.equal(bits(pbox2.grad), bits(pbox.grad))
    sums, counts, _ = ops.head_loss(t("ids"), t("num_rois"), t("deltas"), None, t("logits"), t("pred_bbox"), None)
    assert not bool(sums[:, 2].any()) and not bool(counts[:, 2].any())


# ---------------------------------------------------------------------------------------------------------------- whole head
def gpu_heads(ht, sd):
    return ht.TrainableHeads(ht.TrainableClassifier.from_state_dict(sd, image_area=hc.AREA),
                             ht.TrainableMask.from_state_dict(sd, image_area=hc.AREA, pool=hc.POOL, mask_slots=hc.SLOTS)).to(DEV)


def parameter_grads(heads):
    params = {**{"classifier." + n: p for n, p in heads.classifier.named_parameters()}, **{"mask." + n: p for n, p in heads.mask.named_parameters()}}
    return {n: params[n].grad for n in hc.TRAINED}


def run_heads(ht, sd, maps, t, reduction="mean"):
    heads = gpu_heads(ht, sd)
    fms = [dev(m).requires_grad_(True) for m in maps]
    out = heads.losses(fms, hc.detection_targets_of(t, DEV), reduction)
    (out.class_loss.sum() + out.bbox_loss.sum() + out.mask_loss.sum()).backward()
    torch.cuda.synchronize()
    return out, [f.grad for f in fms], parameter_grads(heads)


def dense_route(sd, maps, t):
    """This project's own dense route: RoIAlign and the layers composition over all count slots, conv5 to all C planes,
    losses.head_losses → (the three losses, [map gradients], {parameter: gradient})."""
    from maskrcnn_amd import layers, losses, modules, ops
    fms = [dev(m).requires_grad_(True) for m in maps]
    q = {k: dev(v).requires_grad_(k in hc.TRAINED) for k, v in sd.items() if v.is_floating_point()}
    ohwi = lambda w: w.permute(0, 2, 3, 1).contiguous()
    c, r = hc.CLASSES, hc.BATCH * hc.COUNT
    pooled = ops.roi_align_pyramid(fms, dev(t["rois"]).reshape(r, 4), hc.POOL, hc.AREA, rois_per_image=hc.COUNT)
    s1, t1 = modules.fold_bn(q, "classifier.conv1", "classifier.bn1", DEV)
    s2, t2 = modules.fold_bn(q, "classifier.conv2", "classifier.bn2", DEV)
    h = layers.conv_bn_act(pooled.reshape(r, 1, 1, -1), ohwi(q["classifier.conv1.weight"]).reshape(hc.HIDDEN, 1, 1, -1), s1, t1, act=1)
    h = layers.conv_bn_act(h, ohwi(q["classifier.conv2.weight"]), s2, t2, act=1)
    w_fc = torch.cat([q["classifier.linear_class.weight"], q["classifier.linear_bbox.weight"]], 0).view(5 * c, 1, 1, hc.HIDDEN)
    y = layers.conv_bn_act(h, w_fc, None, torch.cat([q["classifier.linear_class.bias"], q["classifier.linear_bbox.bias"]])).view(r, 5 * c)
    x = pooled
    for i in (1, 2, 3, 4):
        s, sh = modules.fold_bn(q, f"mask.conv{i}", f"mask.bn{i}", DEV)
        x = layers.conv_bn_act(x, ohwi(q[f"mask.conv{i}.weight"]), s, sh, (1, 1, 1, 1), 1)
    w4 = q["mask.deconv.weight"].permute(2, 3, 1, 0).reshape(4 * hc.DEPTH, 1, 1, hc.DEPTH).contiguous()
    x = layers.deconv2x2(x, w4, q["mask.deconv.bias"].repeat(4), 1)
    m = layers.conv_bn_act(x, ohwi(q["mask.conv5.weight"]), None, q["mask.conv5.bias"], act=2)
    masks = m.permute(0, 3, 1, 2).reshape(hc.BATCH, hc.COUNT, c, 2 * hc.POOL, 2 * hc.POOL)
    out = losses.head_losses(hc.detection_targets_of(t, DEV), y[:, :c].reshape(hc.BATCH, hc.COUNT, c),
                             y[:, c:].reshape(hc.BATCH, hc.COUNT, c, 4), masks)
    (out.class_loss + out.bbox_loss + out.mask_loss).backward()
    return out, [f.grad for f in fms], {n: q[n].grad for n in hc.TRAINED}


@pytest.mark.parametrize("name", hc.HEAD_NAMES)
def test_losses_and_gradients_on_rounded_data_within_twice_the_dense_routes_error(ht, name):
    """For each loss and each gradient tensor: max|ours - f64| <= 2 max|dense - f64| + 4u max|f64|. The class-plane route does the dense
    route's arithmetic minus exact zero terms, with the conv5 dot product and its weight gradient in fp64 (margin 2); the floor covers the
    fp32 narrowing. Observed on the MI355X over the two cases' 54 rows, in units of u max|f64| (printed below): ours at most 23.34 (the
    gradient of classifier.linear_bbox.weight, the dense route's own figure), the dense route at most 23.34, ours / dense at most 1.76
    (3.90 against 2.21, the gradient of mask.conv3.bias: the trunk's shift gradient is summed over B P slots here and over B count
    there); the six losses agree with the dense route's to the printed digits (0.04 .. 3.80)."""
    h = hc.head_case(name)
    maps, t = hc.head_maps(), hc.head_targets(h)
    sd = hc.separated_params(maps, t)
    want_cls, want_box, want_mask, m64, sd64 = hc.stock_losses(h, maps, t, sd)
    d_out, d_maps, d_p = dense_route(sd, maps, t)
    out, g_maps, g_p = run_heads(ht, sd, maps, t)
    assert out.status.tolist() == [0, 0] and d_out.status.tolist() == [0, 0]
    rows = [("class loss", out.class_loss.detach(), d_out.class_loss.detach(), want_cls),
            ("box loss", out.bbox_loss.detach(), d_out.bbox_loss.detach(), want_box),
            ("mask loss", out.mask_loss.detach(), d_out.mask_loss.detach(), want_mask)]
    rows += [(f"gradient of map {l}", g, d, m.grad) for l, (g, d, m) in enumerate(zip(g_maps, d_maps, m64))]
    rows += [(f"gradient of {n}", g_p[n], d_p[n], sd64[n].grad) for n in hc.TRAINED]
    failed = []
    for what, ours, dense, want in rows:
        want = want.to(F64)
        e_ours = float((ours.cpu().to(F64) - want).abs().max())
        e_dense = float((dense.cpu().to(F64) - want).abs().max())
        scale = float(want.abs().max())
        unit = U * scale if scale > 0 else 1.0
        print(f"{name}: {what}: ours {e_ours / unit:.2f} u, dense {e_dense / unit:.2f} u (u = 2^-24 max|f64| = {unit:.3e})")
        if not e_ours <= 2 * e_dense + 4 * U * scale:
            failed.append((what, e_ours, e_dense, scale))
    assert not failed, failed
    again, a_maps, a_p = run_heads(ht, sd, maps, t)
    for a, b in zip([*out[:3], *g_maps, *g_p.values()], [*again[:3], *a_maps, *a_p.values()]):
        assert torch.equal(bits(a), bits(b)), "two calls differ"


def test_an_images_losses_and_map_gradients_do_not_depend_on_the_rest_of_the_batch(ht):
    """Per image ("per_image": each image's own sums and counts) against the image run alone. The class-plane ops give the same bits
    (asserted above, op by op); the layers in front of them may take another K route of the conv kernels at another batch size, so the
    whole head is held to 8 u of the largest value."""
    h = hc.head_case("full_and_one")
    maps, t = hc.head_maps(), hc.head_targets(h)
    sd = hc.separated_params(maps, t)
    out, g_maps, _ = run_heads(ht, sd, maps, t, "per_image")
    assert tuple(out.mask_loss.shape) == (hc.BATCH,)
    for i in range(hc.BATCH):
        alone, a_maps, _ = run_heads(ht, sd, [m[i:i + 1] for m in maps], {k: v[i:i + 1] for k, v in t.items()}, "per_image")
        for got, want in zip(alone[:3], out[:3]):
            assert abs(float(got[0].detach()) - float(want[i].detach())) <= 8 * U * max(1.0, abs(float(want[i].detach())))
        for l, (g, w) in enumerate(zip(a_maps, g_maps)):
            assert float((g[0] - w[i]).abs().max()) <= 8 * U * max(1.0, float(w[i].abs().max())), f"image {i}, map {l}"


def test_a_positive_past_the_mask_slots_sets_the_status_bit(ht):
    h = hc.head_case("full_and_one")
    maps, t = hc.head_maps(), hc.head_targets(h)
    heads = gpu_heads(ht, hc.head_params())
    heads.mask.mask_slots = 2                                                        # image 0 has three positives
    out = heads.losses([dev(m) for m in maps], hc.detection_targets_of(t, DEV))
    assert out.status.tolist() == [ht.STATUS_NO_ROOM, 0] and bool(torch.isfinite(out.mask_loss))


# ----------------------------------------------------------------------------------------------------------------- arguments
def test_bad_arguments_are_refused_with_the_house_message_before_any_launch(ops):
    c = hc.case("shared_class")
    o = hc.operands(c, integer=False)
    ids, num = targets(c)
    x, w, bias, dy, p, target = dev(o.x), dev(o.w), dev(o.bias), dev(o.dy), dev(hc.probabilities(c)), dev(o.target)
    prof = ops.CONV_PROFILE
    ops.CONV_PROFILE = []                  # every launch of a binding is booked here: it must stay empty
    try:
        with pytest.raises(RuntimeError, match=r"class_plane_conv: act must be 0 \(none\) or 2 \(sigmoid\), got 1"):
            ops.class_plane_conv(x, w, bias, ids, num, 1)
        with pytest.raises(RuntimeError, match=r"class_plane_conv: x must be float32 \[S,mh,mw,Cin\] with mh, mw in 1 \.\. 64 and Cin a multiple of 4"):
            ops.class_plane_conv(torch.zeros(6, 4, 4, 6, device=DEV), torch.zeros(5, 6, device=DEV), None, ids, num)
        with pytest.raises(RuntimeError, match=r"class_plane_conv: x must be float32 \[S,mh,mw,Cin\] with mh, mw in 1 \.\. 64"):
            ops.class_plane_conv(torch.zeros(6, 65, 4, 8, device=DEV), w, None, ids, num)
        with pytest.raises(RuntimeError, match=r"class_plane_conv: w must be float32 \[C>=2,8\], got float32 \[5, 4\]"):
            ops.class_plane_conv(x, w[:, :4], bias, ids, num)
        with pytest.raises(RuntimeError, match=r"class_plane_conv: w must be float32 \[C>=2,8\], got float32 \[1, 8\]"):
            ops.class_plane_conv(x, w[:1], None, ids, num)
        with pytest.raises(RuntimeError, match=r"class_plane_conv: bias must be float32 \[5\] or None, got float32 \[4\]"):
            ops.class_plane_conv(x, w, bias[:4], ids, num)
        with pytest.raises(RuntimeError, match=r"class_plane_conv: plane slots P must be in 1 \.\. count = 8, got 0"):
            ops.class_plane_conv(x[:5], w, bias, ids, num)                                   # 5 slots for 2 images
        with pytest.raises(RuntimeError, match=r"class_plane_conv: plane slots P must be in 1 \.\. count = 8, got 9"):
            ops.class_plane_conv(torch.zeros(18, 4, 4, 8, device=DEV), w, bias, ids, num)
        with pytest.raises(RuntimeError, match=r"class_plane_conv: num must be int32 \[2\], got int32 \[3\]"):
            ops.class_plane_conv(x, w, bias, ids, torch.zeros(3, dtype=I32, device=DEV))
        with pytest.raises(RuntimeError, match=r"class_plane_conv: ids must be int32 \[B>=1,count>=1\], got int64 \[2, 8\]"):
            ops.class_plane_conv(x, w, bias, ids.to(torch.int64), num)
        with pytest.raises(RuntimeError, match=r"class_plane_conv: ids must be int32 \[B,count\] with B in 1 \.\. 65535 and count in 1 \.\. 1024"):
            ops.class_plane_conv(x[:2], w, bias, torch.zeros(2, 1025, dtype=I32, device=DEV), num)
        with pytest.raises(RuntimeError, match=r"class_plane_conv: out tensor out must be float32 \[6,4,4\] contiguous"):
            ops.class_plane_conv(x, w, bias, ids, num, out=torch.zeros(6, 4, 5, device=DEV))
        with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
            ops.class_plane_conv(x.cpu(), w, bias, ids, num)
        with pytest.raises(RuntimeError, match=r"class_plane_conv_backward: dy must be float32 \[6,4,4\], got float32 \[6, 4, 3\]"):
            ops.class_plane_conv_backward(dy[..., :3], None, x, w, ids, num)
        with pytest.raises(RuntimeError, match=r"class_plane_conv_backward: y must be float32 \[6,4,4\], got None"):
            ops.class_plane_conv_backward(dy, None, x, w, ids, num, 2)
        with pytest.raises(RuntimeError, match=r"class_plane_conv_backward: needs must hold 3 flags \(dx, dw, dbias\), got 4"):
            ops.class_plane_conv_backward(dy, None, x, w, ids, num, 0, needs=(True,) * 4)
        with pytest.raises(RuntimeError, match=r"class_plane_conv_backward: out tensor dw must be float32 \[5,8\] contiguous"):
            ops.class_plane_conv_backward(dy, None, x, w, ids, num, 0, out=(None, torch.zeros(8, 5, device=DEV), None))
        with pytest.raises(RuntimeError, match=r"mask_plane_loss: p must be float32 \[B>=1,P>=1,mh>=1,mw>=1\], got float32 \[6, 4, 4\]"):
            ops.mask_plane_loss(p.view(6, 4, 4), target, ids, num, 5)
        with pytest.raises(RuntimeError, match=r"mask_plane_loss: target_mask must be float32 \[2,8,4,4\], got float32 \[2, 3, 4, 4\]"):
            ops.mask_plane_loss(p, target[:, :3], ids, num, 5)
        with pytest.raises(RuntimeError, match=r"mask_plane_loss: num_classes must be an int in 2 \.\. 4096, got 1"):
            ops.mask_plane_loss(p, target, ids, num, 1)
        with pytest.raises(RuntimeError, match=r"mask_plane_loss: plane slots P must be in 1 \.\. count = 8, got 9"):
            ops.mask_plane_loss(torch.zeros(2, 9, 4, 4, device=DEV), target, ids, num, 5)
        with pytest.raises(RuntimeError, match=r"mask_plane_loss_backward: counts must be int32 \[2\], got int32 \[2, 3\] as the forward returned them"):
            ops.mask_plane_loss_backward(p, target, ids, num, 5, torch.zeros(2, 3, dtype=I32, device=DEV), torch.ones(1, device=DEV))
        with pytest.raises(RuntimeError, match=r"mask_plane_loss_backward: grad_out must be float32 \[2\], got float32 \[1\]"):
            ops.mask_plane_loss_backward(p, target, ids, num, 5, torch.zeros(2, dtype=I32, device=DEV), torch.ones(1, device=DEV), True)
        assert ops.CONV_PROFILE == [], "a refused call launched something"
    finally:
        ops.CONV_PROFILE = prof


# ---------------------------------------------------------------------------------------------------------- schedule fuzzing
# The child's time limit: four times the wall time measured on the fuzzed library, rounded up to 30 s: 4.3 s for the child's 90 tests,
# start-up included, so 17 s -> 30 s.
FUZZ_TIMEOUT = 30


@pytest.mark.skipif(os.environ.get("MRCNN_SYNC_FUZZ_CHILD") == "1", reason="this IS the fuzzed child run")
def test_this_file_passes_under_schedule_fuzzing():
    """class_plane_backward_kernel hands the partial sums of waves 1 .. 3 to wave 0 through LDS, once per group of 256 channels, with a
    barrier on each side of the hand-off; the loss kernels sum through workgroup.hpp's block_sum, whose LDS row the next call reuses; the
    finishing launch ranks the slots of a class with ballots and no barrier at all. On the fuzzed build every wave sleeps a random time
    behind each barrier, and a hand-off that the barriers do not order fails its bit-for-bit comparison there."""
    assert os.path.exists(FUZZ_LIB), f"{FUZZ_LIB} is missing: run __graft_entry__.build()"
    env = dict(os.environ, MRCNN_LIB=FUZZ_LIB, MRCNN_SYNC_FUZZ_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_head_train.py", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=FUZZ_TIMEOUT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
