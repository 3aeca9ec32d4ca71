"""maskrcnn_amd/_binding.py on the host: the one argument checker and the one `out` checker (device refusal switched off, CPU
tensors), what is registered under torch.ops.maskrcnn, and that no assert stands between a caller and a kernel."""
import ast
import os

import pytest
import torch

import maskrcnn_amd  # noqa: F401  (registers the ops)
from maskrcnn_amd import _binding, ops
from maskrcnn_amd._binding import checked, checked_out

F32, I32, U8 = torch.float32, torch.int32, torch.uint8


def refused(match_got, **kw):
    """checked("the_op", "the_arg", ..., gpu=False) raises a RuntimeError that names the op, the argument and what it got."""
    with pytest.raises(RuntimeError) as e:
        checked("the_op", "the_arg", gpu=False, **kw)
    msg = str(e.value)
    assert msg.startswith("the_op: the_arg must be "), msg
    assert match_got in msg.split(", got ", 1)[1], msg
    return msg


def accepted(**kw):
    return checked("the_op", "the_arg", gpu=False, **kw)


def test_checker_dtype_set_and_bool_view():
    t = torch.zeros(3, dtype=U8)
    assert accepted(t=t, dtype=(U8, torch.bool), shape=(3,)) is t
    b = torch.zeros(3, dtype=torch.bool)
    got = accepted(t=b, dtype=(U8, torch.bool), shape=(3,), bool_as_uint8=True)
    assert got.dtype == U8 and got.data_ptr() == b.data_ptr()
    assert accepted(t=b, dtype=(U8, torch.bool), shape=(3,)).dtype == torch.bool
    msg = refused("int32 [3]", t=torch.zeros(3, dtype=I32), dtype=(U8, torch.bool), shape=(3,))
    assert "uint8 / bool [3]" in msg
    refused("bool [3]", t=b, dtype=U8, shape=(3,), bool_as_uint8=True)           # the view does not widen what is accepted


def test_checker_rank_and_dimensions():
    t = torch.zeros(2, 5, 4)
    assert accepted(t=t, dtype=F32, shape=(2, "N", 4)) is t                         # exact, free, exact
    assert accepted(t=t, dtype=F32, shape=(("B", 1), ("N", 5), 4)) is t             # minimum met, minimum met exactly
    assert accepted(t=t, dtype=F32, shape=None) is t                                # any shape
    refused("float32 [2, 5, 4]", t=t, dtype=F32, shape=(2, "N"))                    # one rank too few in the pattern
    refused("float32 [5, 4]", t=t[0], dtype=F32, shape=(2, "N", 4))                 # one rank too few in the tensor
    refused("float32 [2, 5, 4]", t=t, dtype=F32, shape=(3, "N", 4))                 # exact size off by one
    msg = refused("float32 [2, 5, 4]", t=t, dtype=F32, shape=(2, ("N", 6), 4))      # minimum missed by one
    assert "float32 [2,N>=6,4]" in msg
    assert accepted(t=torch.zeros(0, 4), dtype=F32, shape=("M", 4)).shape == (0, 4)  # a free dimension may be empty


def test_checker_optional_and_hint():
    assert accepted(t=None, dtype=F32, shape=(3,), optional=True) is None
    refused("None", t=None, dtype=F32, shape=(3,))
    msg = refused("int32 [3]", t=torch.zeros(3, dtype=I32), dtype=F32, shape=(3,), optional=True, hint=" (see the_doc)")
    assert "or None" in msg and msg.endswith(" (see the_doc)")


def test_checker_strides_and_alignment():
    base = torch.arange(24, dtype=F32).view(4, 6)
    view = base.t()                                                                  # [6, 4], strides (1, 6)
    got = accepted(t=view, dtype=F32, shape=(6, 4))
    assert got.is_contiguous() and torch.equal(got, view) and got.data_ptr() != view.data_ptr()
    assert accepted(t=view, dtype=F32, shape=(6, 4), strides="keep") is view
    msg = refused("float32 [6, 4] strides (1, 6)", t=view, dtype=F32, shape=(6, 4), strides="refuse")
    assert "contiguous" in msg
    assert accepted(t=base, dtype=F32, shape=(4, 6), strides="refuse") is base
    # alignment is repaired, not refused: an aligned tensor passes as it is, a misaligned one comes back as an aligned copy
    assert base.data_ptr() % 16 == 0 and accepted(t=base, dtype=F32, shape=(4, 6), align16=True) is base
    off = torch.zeros(25, dtype=F32)[1:].view(4, 6)
    assert off.data_ptr() % 16 == 4
    assert accepted(t=off, dtype=F32, shape=(4, 6)) is off
    fixed = accepted(t=off, dtype=F32, shape=(4, 6), align16=True)
    assert fixed is not off and fixed.data_ptr() % 16 == 0 and torch.equal(fixed, off)
    grad = torch.zeros(3, requires_grad=True)
    assert not accepted(t=grad, dtype=F32, shape=(3,)).requires_grad


def test_checker_refuses_cpu_tensors_first():
    wrong_everything = torch.zeros(2, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        checked("the_op", "the_arg", wrong_everything, I32, (7,))
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        checked_out("the_op", "out", wrong_everything, I32, (7,), torch.device("cpu"))


def test_out_checker():
    cpu, meta = torch.device("cpu"), torch.device("meta")
    want = dict(dtype=I32, shape=(2, 3), dev=cpu, gpu=False)
    good = torch.empty(2, 3, dtype=I32)
    assert checked_out("the_op", "the_out", good, **want) is good
    made = checked_out("the_op", "the_out", None, **want)
    assert made.dtype == I32 and made.shape == (2, 3) and made.device == cpu
    assert not checked_out("the_op", "the_out", None, zeros=True, **want).any()
    for bad, got in ((torch.empty(2, 3, dtype=torch.int64), "int64 [2, 3]"), (torch.empty(2, 4, dtype=I32), "int32 [2, 4]"),
                     (torch.empty(3, 2, dtype=I32).t(), "strides (1, 2)"), (torch.empty(2, 3, dtype=I32, device=meta), "on meta")):
        with pytest.raises(RuntimeError) as e:
            checked_out("the_op", "the_out", bad, **want)
        msg = str(e.value)
        assert msg.startswith("the_op: out tensor the_out must be int32 [2,3] contiguous on cpu, got ") and got in msg, msg
    view = torch.empty(3, 2, dtype=I32).t()
    assert checked_out("the_op", "the_out", view, contiguous=False, **want) is view
    longer = torch.empty(9, dtype=I32)                                               # a minimum: a longer buffer will do
    assert checked_out("the_op", "the_out", longer, I32, (("len", 6),), cpu, gpu=False) is longer
    assert checked_out("the_op", "the_out", None, I32, (("len", 6),), cpu, gpu=False).shape == (6,)
    with pytest.raises(RuntimeError, match="len>=6"):
        checked_out("the_op", "the_out", torch.empty(5, dtype=I32), I32, (("len", 6),), cpu, gpu=False)


def test_workspace_and_null_pointer():
    assert _binding._ptr(None) is None and _binding._ptr0(None) is None
    assert _binding._ptr0(torch.empty(0, 4)) is None
    t = torch.empty(1, 4)
    assert _binding._ptr0(t) == t.data_ptr() == _binding._ptr(t)
    assert torch.empty(3, 0).data_ptr() == 0                                         # null already: _ptr0 changes nothing for it
    for nbytes, want in ((0, 16), (1, 16), (16, 16), (17, 17), (4096, 4096)):
        ws = _binding.workspace(nbytes, "cpu")
        assert ws.dtype == U8 and ws.numel() == want


def test_a_pattern_entry_of_another_type_is_an_error_not_a_free_dimension():
    import numpy as np
    with pytest.raises(TypeError, match="shape pattern entry"):
        accepted(t=torch.zeros(3), dtype=F32, shape=(np.int64(4),))
    with pytest.raises(TypeError, match="shape pattern entry"):
        accepted(t=torch.zeros(3), dtype=F32, shape=(None,))


# str(torch.ops.maskrcnn.<op>.default._schema) for every op, as the commit before the binding modules were split registered them.
SCHEMAS = [
    'maskrcnn::anchor_match(Tensor anchors, Tensor gt_boxes, Tensor gt_class_ids, Tensor gt_off, float neg_iou=0.29999999999999999, float pos_iou=0.69999999999999996, float crowd_iou=0.001) -> (Tensor, Tensor, Tensor, Tensor, Tensor)',
    'maskrcnn::bbox_iou(Tensor dt, Tensor gt, Tensor? iscrowd=None, Tensor? dt_off=None, Tensor? gt_off=None, Tensor? out_off=None, int? out_len=None) -> Tensor',
    'maskrcnn::blend_instances(Tensor image, Tensor masks, Tensor colors, Tensor? boxes=None, int threshold=0) -> Tensor',
    'maskrcnn::bottleneck_forward(Tensor x, Tensor w1, Tensor s1, Tensor t1, Tensor w2, Tensor s2, Tensor t2, Tensor w3, Tensor s3, Tensor t3, Tensor? wd, Tensor? sd, Tensor? td, int stride) -> Tensor',
    'maskrcnn::conv_bn_act(Tensor x, Tensor w, Tensor? scale, Tensor? shift, int stride, int[] pad, bool relu, Tensor? residual, int res_div) -> Tensor',
    'maskrcnn::crop(Tensor image, Tensor boxes, Tensor box_index, float extrapolation_value, int crop_height, int crop_width) -> Tensor',
    'maskrcnn::crop_backward(Tensor grads, Tensor boxes, Tensor box_index, Tensor(a!) grads_image) -> ()',
    'maskrcnn::crop_forward(Tensor image, Tensor boxes, Tensor box_index, float extrapolation_value, int crop_height, int crop_width, Tensor(a!) crops) -> ()',
    'maskrcnn::detection_targets(Tensor rois, Tensor gt_boxes, Tensor gt_class_ids, Tensor gt_off, Tensor keys, int count=100, float positive_ratio=0.33000000000000002, float[] std_dev=[0.10000000000000001, 0.10000000000000001, 0.20000000000000001, 0.20000000000000001], float pos_iou=0.5, float crowd_iou=0.001) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)',
    'maskrcnn::head_loss(Tensor target_class_ids, Tensor num_rois, Tensor target_deltas, Tensor target_mask, Tensor logits, Tensor pred_bbox, Tensor pred_masks) -> (Tensor, Tensor, Tensor)',
    'maskrcnn::head_loss_backward(Tensor target_class_ids, Tensor num_rois, Tensor target_deltas, Tensor target_mask, Tensor logits, Tensor pred_bbox, Tensor pred_masks, Tensor counts, Tensor grad_out) -> (Tensor, Tensor, Tensor)',
    'maskrcnn::mask_targets(Tensor gt_masks, Tensor gt_off, Tensor rois_out, Tensor gt_index, Tensor num_pos, int[] mask_shape=28) -> Tensor',
    'maskrcnn::nms(Tensor dets, float threshold) -> Tensor',
    'maskrcnn::rle_area_bbox(Tensor num_runs, Tensor counts, Tensor heights, Tensor widths) -> (Tensor, Tensor)',
    'maskrcnn::rle_decode(Tensor num_runs, Tensor counts, int height, int width) -> Tensor',
    'maskrcnn::rle_encode(Tensor masks, int threshold=0, int? capacity=None) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)',
    'maskrcnn::rle_from_poly(Tensor xy, Tensor vert_off, Tensor heights, Tensor widths, int? capacity=None) -> (Tensor, Tensor, Tensor)',
    'maskrcnn::rle_from_string(Tensor bytes, Tensor str_off, Tensor heights, Tensor widths, int? capacity=None) -> (Tensor, Tensor, Tensor)',
    'maskrcnn::rle_iou(Tensor dt_num_runs, Tensor dt_counts, Tensor gt_num_runs, Tensor gt_counts, Tensor? iscrowd=None, Tensor? dt_off=None, Tensor? gt_off=None, Tensor? out_off=None, int? out_len=None) -> Tensor',
    'maskrcnn::rle_merge(Tensor num_runs, Tensor counts, Tensor group_off, bool intersect=False, int? capacity=None) -> (Tensor, Tensor)',
    'maskrcnn::rle_to_string(Tensor num_runs, Tensor counts, int? total_bytes=None) -> (Tensor, Tensor)',
    'maskrcnn::rpn_deltas(Tensor anchors, Tensor gt_boxes, Tensor gt_off, Tensor match, Tensor iou_argmax, int count, float[] std_dev) -> (Tensor, Tensor)',
    'maskrcnn::rpn_loss(Tensor match, Tensor logits, Tensor pred_bbox, Tensor target_bbox) -> (Tensor, Tensor, Tensor, Tensor)',
    'maskrcnn::rpn_loss_backward(Tensor match, Tensor logits, Tensor pred_bbox, Tensor target_bbox, Tensor chunk_pos, Tensor counts, Tensor grad_out) -> (Tensor, Tensor)',
    'maskrcnn::sample_by_key(Tensor match, Tensor keys, int count) -> Tensor',
]
PUBLIC = ['HeadSums', 'MaskrcnnHipError', 'anchor_match', 'bbox_iou', 'blend_instances', 'bottleneck_forward', 'bottleneck_fused',
          'bottleneck_fused_supported', 'bottleneck_native', 'bottleneck_plan', 'coco_match', 'conv3x3_winograd_heads', 'conv_bn_act',
          'conv_bn_act_f16mfma', 'crop', 'deconv2x2', 'detection_decode', 'detection_select', 'detection_targets', 'head_loss',
          'head_loss_backward', 'mask_targets', 'maxpool', 'nchw_to_nhwc', 'nhwc_to_nchw', 'nms_batched', 'nms_general', 'proposal_decode',
          'proposal_select', 'rle_area_bbox', 'rle_decode', 'rle_encode', 'rle_from_poly', 'rle_from_string', 'rle_iou', 'rle_merge',
          'rle_to_string', 'roi_align_pyramid', 'rpn_deltas', 'rpn_loss', 'rpn_loss_backward', 'rpn_scores_deltas',
          'same_pad', 'sample_by_key', 'split_f16', 'topk_desc']


def test_registered_schemas_and_public_names_are_the_parents():
    registered = sorted(str(s) for s in torch._C._jit_get_all_schemas() if s.name.startswith("maskrcnn::"))
    assert registered == SCHEMAS
    for schema in SCHEMAS:
        name = schema[len("maskrcnn::"):schema.index("(")]
        assert str(getattr(torch.ops.maskrcnn, name).default._schema) == schema
    assert set(ops.__all__) == set(PUBLIC) and len(ops.__all__) == len(PUBLIC)
    for name in PUBLIC + ["RLE_BAD_BYTE", "RLE_LONG_TOKEN", "RLE_OPEN_TOKEN", "RLE_BAD_SIZE", "RLE_BAD_OFFSETS", "RLE_EMPTY_RUN",
                          "RLE_PIXEL_SUM", "POLY_MAX_DIM", "POLY_MAX_PART_POINTS", "poly_host_bounds", "rle_string_tokens", "rle_table",
                          "CONV_PROFILE", "BOTTLENECK_OP_FUSED", "NMS_MAX_BOXES", "nms_plan", "NmsPlan", "crop_plan", "CropPlan",
                          "resize_route", "paste_store_width"]:
        assert hasattr(ops, name), name


def test_every_op_refuses_cpu_tensors_by_default():
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        torch.ops.maskrcnn.sample_by_key(torch.zeros(1, 8, dtype=I32), torch.zeros(1, 8, dtype=I32), 4)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        ops.sample_by_key(torch.zeros(1, 8, dtype=I32), torch.zeros(1, 8, dtype=I32), 4)


def test_launches_of_every_module_book_into_the_list_assigned_on_ops(monkeypatch):
    """_launch lives in _binding.py and serves three modules; the list it appends to is the one assigned as ops.CONV_PROFILE."""
    assert _binding._profile_home is ops
    calls = []
    monkeypatch.setattr(ops, "CONV_PROFILE", None)
    _binding._launch(lambda *a: calls.append(a) or 0, (1, 2), lambda: pytest.fail("book() runs only while profiling"))
    assert calls == [(1, 2)]

    class Event:                                   # stands in for torch.cuda.Event: the host has no stream to record on
        def __init__(self, enable_timing):
            self.recorded_after = None

        def record(self):
            self.recorded_after = len(calls)
    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(ops, "CONV_PROFILE", [])       # as bench.py and the tests switch it on: assigned on ops
    _binding._launch(lambda *a: calls.append(a) or 0, (3,), lambda: (7.0, (1, 2, 3), 11, "tag"))
    (e0, e1, *booked), = ops.CONV_PROFILE
    assert calls == [(1, 2), (3,)] and (e0.recorded_after, e1.recorded_after) == (1, 2) and booked == [7.0, (1, 2, 3), 11, "tag"]
    with pytest.raises(ops.MaskrcnnHipError):          # a failing entry point raises and books nothing
        _binding._launch(lambda: 1, (), lambda: pytest.fail("book() after a failed launch"))
    assert len(ops.CONV_PROFILE) == 1


def test_no_assert_between_a_caller_and_a_kernel():
    here = os.path.dirname(os.path.abspath(_binding.__file__))
    for name in ("ops.py", "ops_coco.py", "ops_train.py", "_binding.py"):
        with open(os.path.join(here, name)) as f:
            tree = ast.parse(f.read())
        found = [node.lineno for node in ast.walk(tree) if isinstance(node, ast.Assert)]
        assert not found, f"{name}: assert at lines {found} vanishes under python -O; raise RuntimeError instead"
