"""The training losses on the GPU (csrc/losses.hip) against what the reference's own five loss functions returned
(tests/golden/losses.npz): every case through ops.*, through torch.ops.maskrcnn.* and through losses.* with .backward(), under both
reductions.

Bars (losses_cases, derived there): every loss and every gradient element within 1 fp32 ulp of the fixture value + 1e-14; every loss
at least as close to the float64 reference as the reference's own float32 result plus one ulp; counts and status bit-equal; exact
zeros in the gradients wherever the fixture has them; a second call bit-identical to the first (the fixed order of the sums)."""
import numpy as np
import pytest
import torch

from losses_cases import HEAD_NAMES, RPN_NAMES, assert_losses, assert_within_one_ulp, head_case, rpn_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REDUCTIONS = ("mean", "per_image")
HEAD_GRADS = ("grad_logits", "grad_bbox", "grad_masks")


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def rpn_inputs(c):
    return dev(c["match"]), dev(c["logits"]), dev(c["pred"]), dev(c["target"])


def head_inputs(c):
    return tuple(dev(c[k]) for k in ("ids", "num_rois", "deltas", "mask", "logits", "pred_bbox", "pred_masks"))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def run_ops(c, args, forward, backward, grads):
    """Forward and backward of one family through a pair of ops, twice; the quotient sums / counts is the caller's."""
    from maskrcnn_amd import losses
    k = len(grads)
    first = forward(*args)
    again = forward(*args)
    sums, counts, status = first[:3]
    assert (sums.dtype, counts.dtype, status.dtype) == (torch.float64, torch.int32, torch.int32)
    assert tuple(sums.shape) == tuple(counts.shape) == (c["batch"], k) and tuple(status.shape) == (c["batch"],)
    assert all(same_bits(a, b) for a, b in zip(first, again)), "two forward calls differ"
    assert np.array_equal(counts.cpu().numpy(), c["counts"]) and np.array_equal(status.cpu().numpy(), c["status"])
    for r in REDUCTIONS:
        assert_losses(losses.reduce_numpy(sums.cpu().numpy(), counts.cpu().numpy(), r)[0], c, r, "ops")
        grad_out = torch.ones((k,) if r == "mean" else (c["batch"], k), dtype=torch.float32, device=DEV)
        got = backward(*args, *first[3:], counts, grad_out)
        again = backward(*args, *first[3:], counts, grad_out)
        assert all(same_bits(a, b) for a, b in zip(got, again)), "two backward calls differ"
        for name, g in zip(grads, got):
            assert g.dtype == torch.float32
            assert_within_one_ulp(g.cpu().numpy(), c[f"{name}_{r}"], f"{c['name']} {r} {name}")
            assert not torch.signbit(g[g == 0]).any(), f"{name}: a -0 where nothing contributes"


@pytest.mark.parametrize("name", RPN_NAMES)
def test_rpn_ops_equal_the_reference(name):
    from maskrcnn_amd import ops
    c = rpn_case(name)
    run_ops(c, rpn_inputs(c), ops.rpn_loss, ops.rpn_loss_backward, ("grad_logits", "grad_bbox"))


@pytest.mark.parametrize("name", RPN_NAMES)
def test_rpn_dispatcher_ops_equal_the_reference(name):
    import maskrcnn_amd  # noqa: F401
    c = rpn_case(name)
    run_ops(c, rpn_inputs(c), torch.ops.maskrcnn.rpn_loss, torch.ops.maskrcnn.rpn_loss_backward, ("grad_logits", "grad_bbox"))


@pytest.mark.parametrize("name", HEAD_NAMES)
def test_head_ops_equal_the_reference(name):
    from maskrcnn_amd import ops
    c = head_case(name)
    run_ops(c, head_inputs(c), ops.head_loss, ops.head_loss_backward, HEAD_GRADS)


@pytest.mark.parametrize("name", HEAD_NAMES)
def test_head_dispatcher_ops_equal_the_reference(name):
    import maskrcnn_amd  # noqa: F401
    c = head_case(name)
    run_ops(c, head_inputs(c), torch.ops.maskrcnn.head_loss, torch.ops.maskrcnn.head_loss_backward, HEAD_GRADS)


@pytest.mark.parametrize("name", RPN_NAMES)
def test_rpn_losses_with_backward_equal_the_reference(name):
    """Upstream gradients of 2 and 4: powers of two scale the fixture's gradients exactly, and the absolute part of the bar stays."""
    from maskrcnn_amd import losses
    c = rpn_case(name)
    match, logits, pred, target = rpn_inputs(c)
    for r in REDUCTIONS:
        logits, pred = logits.detach().requires_grad_(True), pred.detach().requires_grad_(True)
        got = losses.rpn_losses(match.to(torch.int64).unsqueeze(2), logits, pred, target, reduction=r)
        assert got.rpn_class_loss.is_cuda and tuple(got.rpn_bbox_loss.shape) == (() if r == "mean" else (c["batch"],))
        assert_losses(torch.stack(got[:2], -1).detach().cpu().numpy(), c, r, "front end")
        assert np.array_equal(got.status.cpu().numpy(), c["status"])
        (2 * got.rpn_class_loss.sum() + 4 * got.rpn_bbox_loss.sum()).backward()
        assert_within_one_ulp(logits.grad.cpu().numpy(), 2 * c["grad_logits_" + r], f"{name} {r} grad_logits x 2")
        assert_within_one_ulp(pred.grad.cpu().numpy(), 4 * c["grad_bbox_" + r], f"{name} {r} grad_bbox x 4")


@pytest.mark.parametrize("name", HEAD_NAMES)
def test_head_losses_with_backward_equal_the_reference(name):
    from maskrcnn_amd import losses
    c = head_case(name)
    ids, num_rois, deltas, mask, logits, pbox, pmask = head_inputs(c)
    for r in REDUCTIONS:
        # the reference's flat [R, C, ...] predictions under "mean", [B, count, ...] under "per_image"
        shape = (lambda t: t.reshape(-1, *t.shape[2:])) if r == "mean" else (lambda t: t)
        preds = [shape(t.detach()).clone().requires_grad_(True) for t in (logits, pbox, pmask)]
        got = losses.head_losses(ids, num_rois, deltas, mask, *preds, reduction=r)
        assert_losses(torch.stack(got[:3], -1).detach().cpu().numpy(), c, r, "front end")
        assert np.array_equal(got.status.cpu().numpy(), c["status"])
        (2 * got.class_loss.sum() + 4 * got.bbox_loss.sum() + 8 * got.mask_loss.sum()).backward()
        for p, scale, g in zip(preds, (2, 4, 8), HEAD_GRADS):
            assert tuple(p.grad.shape) == tuple(p.shape)
            assert_within_one_ulp(p.grad.cpu().numpy().reshape(c[f"{g}_{r}"].shape), scale * c[f"{g}_{r}"], f"{name} {r} {g} x {scale}")


def test_misaligned_views_keep_the_bits():
    """Predictions that start 4 bytes into their storage (the bindings realign them; the mask gradient's scalar head and tail are
    exercised by the 1x1 and C = 81 cases above)."""
    from maskrcnn_amd import ops
    c = head_case("count8_c81_28")
    args = head_inputs(c)
    want = ops.head_loss(*args)
    shifted = []
    for t in args:
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        buf[1:] = t.reshape(-1)
        shifted.append(buf[1:].view(t.shape))
    assert all(s.data_ptr() % 16 == 4 for s in shifted)
    got = ops.head_loss(*shifted)
    assert all(same_bits(a, b) for a, b in zip(want, got))
    grad_out = torch.ones(3, device=DEV)
    assert all(same_bits(a, b) for a, b in zip(ops.head_loss_backward(*args, want[1], grad_out), ops.head_loss_backward(*shifted, got[1], grad_out)))


def need_memory(gib: int):
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    if free < gib * 2 ** 30:
        pytest.skip(f"needs {gib} GB of free device memory, {free / 2 ** 30:.1f} GB are free")


def test_head_offsets_above_2_to_31():
    """1024 slots x 512 classes x 64 x 64 mask floats are 2^31 elements: the last slot's last plane, the only one that contributes
    to the box and mask losses, lies past what an int32 offset can hold. It must equal the same slot run on its own, bit for bit,
    and every other element of the 8 GB mask gradient must be zero."""
    from maskrcnn_amd import ops
    need_memory(24)
    count, classes, side = 1024, 512, 64
    assert count * classes * side * side == 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(11)
    rand = lambda *shape: torch.rand(*shape, device=DEV, generator=g)
    ids = torch.zeros(1, count, dtype=torch.int32, device=DEV)
    ids[0, -1] = classes - 1
    num_rois = torch.tensor([count], dtype=torch.int32, device=DEV)
    deltas, mask = rand(1, count, 4) * 16 - 8, (rand(1, count, side, side) < 0.5).float()
    logits, pbox = rand(1, count, classes) * 16 - 8, rand(1, count, classes, 4) * 16 - 8
    pmask = rand(1, count, classes, side, side).clamp_(1e-6, 1 - 1e-6)
    sums, counts, status = ops.head_loss(ids, num_rois, deltas, mask, logits, pbox, pmask)
    grad_out = torch.ones(1, 3, device=DEV)                                   # per image: scaled by the image's own counts
    grads = ops.head_loss_backward(ids, num_rois, deltas, mask, logits, pbox, pmask, counts, grad_out)
    last = [t[:, -1:].contiguous() for t in (ids, deltas, mask, logits, pbox, pmask)]
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    alone = ops.head_loss(last[0], one, *last[1:])
    alone_grads = ops.head_loss_backward(last[0], one, *last[1:], alone[1], grad_out)
    assert counts.tolist() == [[count, 4, side * side]] and status.tolist() == [0] and alone[1].tolist() == [[1, 4, side * side]]
    assert same_bits(sums[:, 1:], alone[0][:, 1:]) and float(sums[0, 2]) > 0
    assert same_bits(grads[1][:, -1], alone_grads[1][:, 0]) and same_bits(grads[2][:, -1], alone_grads[2][:, 0])
    plane = grads[2][0, -1, classes - 1]
    assert int(torch.count_nonzero(plane)) > side * side - 8
    assert int(torch.count_nonzero(grads[2])) == int(torch.count_nonzero(plane))
    assert int(torch.count_nonzero(grads[1])) == int(torch.count_nonzero(grads[1][0, -1, classes - 1])) == 4


def test_rpn_offsets_above_2_to_31():
    """32 images of 2^24 anchors: pred_bbox and its gradient are 2^31 floats. Only the last image has sampled anchors, the last of
    them the very last anchor; its sums and (per image) its gradients must equal the image run on its own, bit for bit, and the
    31 other images' gradients must be zero."""
    from maskrcnn_amd import ops
    need_memory(40)
    batch, a, count = 32, 1 << 24, 8
    assert batch * a * 4 == 2 ** 31 and batch * a < 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(12)
    match = torch.zeros(batch, a, dtype=torch.int32, device=DEV)
    match[-1, [0, 1023, 1024, a - 1025, a - 2, a - 1]] = 1
    match[-1, [5, a - 3]] = -1
    logits = torch.rand(batch, a, 2, device=DEV, generator=g) * 16 - 8
    pred = torch.rand(batch, a, 4, device=DEV, generator=g) * 16 - 8
    target = torch.rand(batch, count, 4, device=DEV, generator=g) * 16 - 8
    sums, counts, status, chunk_pos = ops.rpn_loss(match, logits, pred, target)
    grad_out = torch.ones(batch, 2, device=DEV)
    grad_logits, grad_bbox = ops.rpn_loss_backward(match, logits, pred, target, chunk_pos, counts, grad_out)
    alone = ops.rpn_loss(match[-1:], logits[-1:], pred[-1:], target[-1:])
    alone_grads = ops.rpn_loss_backward(match[-1:], logits[-1:], pred[-1:], target[-1:], alone[3], alone[1], grad_out[-1:])
    assert counts[-1].tolist() == [8, 24] and not counts[:-1].any() and not status.any() and not sums[:-1].any()
    assert same_bits(sums[-1:], alone[0]) and same_bits(chunk_pos[-1:], alone[3])
    assert same_bits(grad_logits[-1:], alone_grads[0]) and same_bits(grad_bbox[-1:], alone_grads[1])
    assert int(torch.count_nonzero(grad_bbox[-1, a - 1])) == 4 and int(torch.count_nonzero(grad_bbox[-1])) == 24
    assert int(torch.count_nonzero(grad_logits[-1])) == 16
    assert not grad_logits[:-1].any() and not grad_bbox[:-1].any()


class HostTraffic:
    """Counts the calls that move a device tensor to the host or wait for it."""
    NAMES = ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__", "__index__", "nonzero")

    def __init__(self, monkeypatch):
        self.calls = []
        for name in self.NAMES:
            monkeypatch.setattr(torch.Tensor, name, self.counted(name, getattr(torch.Tensor, name)))
        to = torch.Tensor.to

        def counted_to(t, *a, **k):
            out = to(t, *a, **k)
            if t.is_cuda and not out.is_cuda:
                self.calls.append("to")
            return out

        monkeypatch.setattr(torch.Tensor, "to", counted_to)
        monkeypatch.setattr(torch, "nonzero", self.counted("torch.nonzero", torch.nonzero))
        monkeypatch.setattr(torch.cuda, "synchronize", self.counted("synchronize", torch.cuda.synchronize, always=True))

    def counted(self, name, fn, always=False):
        def wrapper(*a, **k):
            if always or (a and isinstance(a[0], torch.Tensor) and a[0].is_cuda):
                self.calls.append(name)
            return fn(*a, **k)
        return wrapper


def test_targets_feed_the_losses_without_touching_the_host(monkeypatch):
    """rpn_targets and detection_targets outputs go straight into the losses and .backward(): nothing is moved to the host before
    the final comparison, which is against the numpy route on the same targets."""
    from maskrcnn_amd import losses, targets
    from targets_cases import shared_geometry
    g = shared_geometry()
    rng = np.random.default_rng(5)
    count, classes, a = 16, 9, 100
    masks = np.zeros((6, 64, 64), np.uint8)
    for i, (y1, x1, y2, x2) in enumerate(g["gt"].astype(int)):
        masks[i, y1:y2, x1:x2] = rng.random((y2 - y1, x2 - x1)) < 0.7
    anchors, rois = dev(g["boxes"]), dev(np.stack([g["boxes"], g["boxes"]]).astype(np.float32))
    gt, ids, off, keys, masks_d = dev(g["gt"]), dev(g["ids"]), dev(g["off"]), dev(g["keys"]), dev(masks)
    uniform = lambda lo, hi, *shape: dev((lo + (hi - lo) * rng.random(shape)).astype(np.float32)).requires_grad_(True)
    rpn_logits, rpn_pred = uniform(-8, 8, 2, a, 2), uniform(-8, 8, 2, a, 4)
    logits, pbox, pmask = uniform(-8, 8, 2 * count, classes), uniform(-8, 8, 2 * count, classes, 4), uniform(0.01, 0.99, 2 * count, classes, 28, 28)
    torch.cuda.synchronize()

    traffic = HostTraffic(monkeypatch)
    rpn_match, rpn_bbox = targets.rpn_targets(anchors, gt, ids, count=count, keys=keys, device=DEV, gt_off=off)
    t = targets.detection_targets(rois / 64, gt / 64, ids, masks_d, count=count, keys=keys, device=DEV, gt_off=off)   # normalised: exact
    rpn = losses.rpn_losses(rpn_match, rpn_logits, rpn_pred, rpn_bbox)
    head = losses.head_losses(t, logits, pbox, pmask)
    total = sum(rpn[:2]) + sum(head[:3])
    total.backward()
    assert traffic.calls == [], f"host traffic before the comparison: {traffic.calls}"
    monkeypatch.undo()

    torch.cuda.synchronize()
    assert int(t.num_pos.sum()) > 0 and int((rpn_match == 1).sum()) > 0 and total.dtype == torch.float32 and torch.isfinite(total)
    host = lambda v: v.detach().cpu().clone().requires_grad_(v.requires_grad)
    h_rpn_logits, h_rpn_pred, h_logits, h_pbox, h_pmask = (host(v) for v in (rpn_logits, rpn_pred, logits, pbox, pmask))
    want_rpn = losses.rpn_losses(host(rpn_match), h_rpn_logits, h_rpn_pred, host(rpn_bbox), device="cpu")
    want_head = losses.head_losses(targets.DetectionTargets(*[host(v) for v in t]), h_logits, h_pbox, h_pmask, device="cpu")
    (sum(want_rpn[:2]) + sum(want_head[:3])).backward()
    for got, want, what in zip((*rpn[:2], *head[:3]), (*want_rpn[:2], *want_head[:3]), ("rpn class", "rpn bbox", "class", "bbox", "mask")):
        assert_within_one_ulp(got.detach().cpu().numpy(), want.detach().numpy(), f"end to end {what} loss")
    assert torch.equal(rpn.status.cpu(), want_rpn.status) and torch.equal(head.status.cpu(), want_head.status)
    for got, want, what in zip((rpn_logits, rpn_pred, logits, pbox, pmask), (h_rpn_logits, h_rpn_pred, h_logits, h_pbox, h_pmask),
                               ("rpn_class_logits", "rpn_pred_bbox", "class_logits", "pred_bbox", "pred_masks")):
        assert_within_one_ulp(got.grad.cpu().numpy(), want.grad.numpy(), f"end to end gradient of {what}")
