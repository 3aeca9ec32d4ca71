"""Host tests (no GPU) of the RPN's training branch: the numpy restatements of the three kernels (maskrcnn_amd.rpn_train) against stock
torch in float64, the conditions that make the GPU tests' bit-for-bit comparisons theorems, and the device="cpu" front end against the
float64 stock graph."""
import numpy as np
import pytest
import torch

import rpn_train_cases as rc
from maskrcnn_amd import _lib, rpn_train
from maskrcnn_amd.rpn_train import TrainableRPN, compact_numpy, gather_numpy, scatter_numpy

F32, F64 = torch.float32, torch.float64
NAMES = [c.id for c in rc.CASES]
E2E = ["corners_and_empty", "overlap_and_over", "wide_k128"]


def compacted(c):
    return compact_numpy(rc.match_of(c), c.capacity)


def test_the_cases_tables_are_the_pyramids():
    assert rpn_train.anchor_firsts(rc.SIZES, rc.APL) == rc.FIRST
    for c in rc.CASES:
        for listed in c.anchors:
            assert listed == sorted(set(listed)) and all(0 <= a < rc.A for a in listed)


def test_the_header_declares_the_three_entry_points_and_the_library_exports_them():
    names = _lib.declared_symbols()
    for name in ("mrcnn_anchor_compact", "mrcnn_pyramid_patch_gather_f32", "mrcnn_pyramid_patch_scatter_f32"):
        assert name in names and hasattr(_lib.lib, name)
    assert _lib.header_abi_version() >= 33 and int(_lib.lib.mrcnn_abi_version()) == _lib.header_abi_version()
    restype, argtypes = _lib.header_prototypes()["mrcnn_pyramid_patch_scatter_f32"]
    assert len(argtypes) == 12


def test_the_bindings_are_reached_through_ops_without_a_schema():
    from maskrcnn_amd import ops
    for name in ("anchor_compact", "pyramid_patch_gather", "pyramid_patch_scatter"):
        assert callable(getattr(ops, name)) and name not in ops.__all__ and not hasattr(torch.ops.maskrcnn, name)


@pytest.mark.parametrize("name", NAMES)
def test_compact_numpy_is_nonzero_in_order_with_capacity_and_overflow(name):
    c = rc.case(name)
    index, num, status = compacted(c)
    assert index.dtype == num.dtype == status.dtype == np.int32 and index.shape == (rc.BATCH, c.capacity)
    for b, listed in enumerate(c.anchors):
        n = min(len(listed), c.capacity)
        assert num[b] == n and status[b] == int(len(listed) > c.capacity)
        assert index[b, :n].tolist() == listed[:n] and (index[b, n:] == -1).all()
    # the k-th positive of the full row is the k-th positive of the compacted one
    m = rc.match_of(c)
    for b in range(rc.BATCH):
        kept = index[b, :num[b]]
        assert np.nonzero(m[b] == 1)[0][:int((m[b, kept] == 1).sum())].tolist() == kept[m[b, kept] == 1].tolist()


@pytest.mark.parametrize("name", NAMES)
def test_gather_numpy_is_unfold_on_the_padded_map(name):
    c = rc.case(name)
    index, num, _ = compacted(c)
    maps = rc.rounded_maps(c)
    got = gather_numpy([m.numpy() for m in maps], index, num, rc.APL)
    assert got.dtype == np.float32 and got.shape == (rc.BATCH * c.capacity, 9 * c.channels)
    want = rc.unfold_patches([m.to(F64) for m in maps], index, num)
    assert np.array_equal(got.astype(np.float64), want.numpy())
    # the empty slots and the padding taps are +0: no sign bit anywhere but where the maps have one
    raw = got.view(np.int32).reshape(rc.BATCH, c.capacity, 9 * c.channels)
    for b in range(rc.BATCH):
        assert not raw[b, num[b]:].any()


@pytest.mark.parametrize("name", NAMES)
def test_scatter_numpy_is_the_autograd_of_unfold(name):
    c = rc.case(name)
    index, num, _ = compacted(c)
    d = rc.dpatch_of(c, integer=True)
    bound = 27 * 8                       # at most 9 taps x 3 anchors a pixel land on one element, each at most 8
    assert bound < 2 ** 24               # every partial sum is an integer below 2^24: fp32 holds it, in any order
    want = rc.unfold_scatter(d, index, num, c.channels)
    got32 = scatter_numpy(d.numpy(), index, num, rc.SIZES, c.channels, rc.APL)
    got64 = scatter_numpy(d.to(F64).numpy(), index, num, rc.SIZES, c.channels, rc.APL)
    for g32, g64, w in zip(got32, got64, want):
        assert g32.dtype == np.float32 and np.array_equal(g32.astype(np.float64), w.numpy()) and np.array_equal(g64, w.numpy())
    # rounded data in float64: the order of a float64 sum of at most 27 terms moves its last bits only
    d = rc.dpatch_of(c, integer=False).to(F64)
    want = rc.unfold_scatter(d, index, num, c.channels)
    for g, w in zip(scatter_numpy(d.numpy(), index, num, rc.SIZES, c.channels, rc.APL), want):
        assert np.abs(g - w.numpy()).max() <= 27 * 2.0 ** -52 * max(1.0, float(w.abs().max()))
    needs = [True, False, True, False, False]
    some = scatter_numpy(d.numpy(), index, num, rc.SIZES, c.channels, rc.APL, needs)
    assert [g is not None for g in some] == needs


@pytest.mark.parametrize("name", NAMES)
def test_the_integer_branch_is_exact_in_fp32(name):
    """Every product and partial sum of the whole-branch case, forward and backward, stays below 2^24, so fp32 computes it exactly in
    any order, and the zero terms the dense graph adds change nothing: sparse and dense agree bit for bit."""
    c = rc.case(name)
    index, num, _ = compacted(c)
    maps, p = rc.integer_maps(c), rc.integer_params(c)
    gl, gb = rc.upstream(c)
    bound = rc.exactness_bound(c, maps, p, index, num, gl, gb)
    assert bound < 2 ** 24, bound
    for v in (*maps, *p, gl, gb):
        assert torch.equal(v, v.round())


@pytest.mark.parametrize("name", E2E)
def test_no_sampled_pre_activation_is_near_zero_in_the_rounded_case(name):
    c = rc.case(name)
    index, num, _ = compacted(c)
    maps = rc.rounded_maps(c)
    margin = rc.relu_margin(maps, rc.separated_params(c, maps, index, num), index, num)
    assert margin > 1e-3, margin


def cpu_rpn(c, p):
    return TrainableRPN.from_state_dict(rc.state_dict_of(p))


def test_from_state_dict_keeps_the_reference_names_and_layouts():
    c = rc.case("corners_and_empty")
    rpn = cpu_rpn(c, rc.rounded_params(c))
    assert (rpn.channels, rpn.anchors_per_location, rpn.hidden) == (c.channels, rc.APL, c.hidden)
    assert sorted(n for n, _ in rpn.named_parameters()) == ["conv_bbox.bias", "conv_bbox.weight", "conv_class.bias", "conv_class.weight",
                                                            "conv_shared.bias", "conv_shared.weight"]
    assert tuple(rpn.conv_shared.weight.shape) == (c.hidden, c.channels, 3, 3) and tuple(rpn.conv_bbox.weight.shape) == (12, c.hidden, 1, 1)


@pytest.mark.parametrize("name", E2E)
def test_the_cpu_front_end_agrees_with_the_float64_stock_graph(name):
    c = rc.case(name)
    maps, target = rc.rounded_maps(c), rc.target_bbox_of(c)
    p = rc.separated_params(c, maps, *compacted(c)[:2])
    want_cls, want_box, m64, p64 = rc.stock_losses(maps, p, rc.kept_match(c), target)
    rpn = cpu_rpn(c, p)
    fms = [m.clone().requires_grad_(True) for m in maps]
    out = rpn.losses(fms, rc.match_of(c), target, device="cpu")
    (out.rpn_class_loss + out.rpn_bbox_loss).backward()
    over = [int(len(listed) > c.capacity) * rpn_train.STATUS_OVERFLOW for listed in c.anchors]
    assert out.status.tolist() == over
    tol = lambda w: 1e-4 * max(1.0, float(w.abs().max()))
    assert abs(float(out.rpn_class_loss.detach()) - float(want_cls)) <= tol(want_cls)
    assert abs(float(out.rpn_bbox_loss.detach()) - float(want_box)) <= tol(want_box)
    for l, (f, m) in enumerate(zip(fms, m64)):
        assert float((f.grad.to(F64) - m.grad).abs().max()) <= tol(m.grad), f"map {l}"
    got = [rpn.conv_shared.weight, rpn.conv_shared.bias, rpn.conv_class.weight, rpn.conv_class.bias, rpn.conv_bbox.weight, rpn.conv_bbox.bias]
    for n, g, w in zip(rc.Params._fields, got, p64):
        assert float((g.grad.to(F64) - w.grad).abs().max()) <= tol(w.grad), n


def test_the_cpu_dense_pass_is_the_stock_graph_and_has_no_graph():
    c = rc.case("corners_and_empty")
    maps, p = rc.rounded_maps(c), rc.rounded_params(c)
    scores, deltas = cpu_rpn(c, p).dense(maps, device="cpu")
    logits, bbox, _ = rc.dense_graph(maps, p)
    assert scores.shape == (rc.BATCH, rc.A) and deltas.shape == (rc.BATCH, rc.A, 4) and not scores.requires_grad
    assert float((scores.to(F64) - torch.softmax(logits, 2)[..., 1]).abs().max()) <= 1e-5
    assert float((deltas.to(F64) - bbox).abs().max()) <= 1e-4 * float(bbox.abs().max())


def test_pyramid_patches_on_the_cpu_honours_needs_input_grad():
    c = rc.case("overlap_and_over")
    index, num, _ = (torch.from_numpy(v) for v in compacted(c))
    maps = rc.integer_maps(c)
    maps[0].requires_grad_(True)
    maps[2].requires_grad_(True)
    d = rc.dpatch_of(c, integer=True)
    out = rpn_train.pyramid_patches(maps, index, num, rc.APL)
    assert out.grad_fn is not None
    out.backward(d)
    want = rc.unfold_scatter(d, index.numpy(), num.numpy(), c.channels)
    assert torch.equal(maps[0].grad.to(F64), want[0]) and torch.equal(maps[2].grad.to(F64), want[2])
    assert maps[1].grad is None and maps[3].grad is None
