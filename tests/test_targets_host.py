"""RPN training targets without a GPU: the numpy route of maskrcnn_amd.targets equals every array the reference's
data.rpn_samples produced (tests/golden/targets.npz, made by tests/golden/make_golden_targets.py) exactly; the header, the
library's exports, the build flags and the argument validation of csrc/targets.hip; anchors.pyramid_anchors' float64 form."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from targets_cases import case, cases, images, pyramid_config, shared_geometry, usable

ENTRY_POINTS = ("mrcnn_anchor_match", "mrcnn_sample_by_key", "mrcnn_rpn_deltas", "mrcnn_anchor_match_workspace_bytes",
                "mrcnn_sample_by_key_workspace_bytes", "mrcnn_rpn_deltas_workspace_bytes")


def test_fixture_covers_the_cases_and_records_its_numpy():
    z = load_golden("targets")
    assert int(str(z["numpy_version"]).split(".")[0]) >= 2          # the deltas follow NumPy >= 2 scalar promotion
    names = {c["name"] for c in cases()}
    for want in ("pyr64_b3", "pyr128_b3", "pyr64_b3_count8", "pyr128_b3_count8_equal_keys", "pyr128_b3_count8_mod4_keys", "thresholds",
                 "ties", "pyr128_outside_duplicates", "pyr64_crowd", "pyr64_all_crowd", "hand20", "rows1024", "full_b2"):
        assert want in names, want
    assert case("pyr64_b3")["anchors"].shape == (1008, 4) and case("pyr128_b3")["anchors"].shape == (4092, 4)
    assert case("full_b2")["anchors"].shape == (261888, 4) and case("full_b2")["batch"] == 2 and case("full_b2")["count"] == 128
    assert all(c["anchors"].dtype == np.float64 for c in cases())
    assert np.diff(case("rows1024")["off"]).max() == 1024
    assert sorted(np.diff(case("pyr64_b3")["off"]).tolist()) == [1, 3, 6]
    # the thresholds: anchor 0 is neutral at IoU 30/100, positive at 70/100 and at 1
    t = case("thresholds")
    assert t["match_u"][:, 0].tolist() == [0, 1, 1]
    assert t["iou_max"][:, 0].tolist() == [np.float32(0.3), np.float32(0.7), 1.0]
    # ties: the first duplicate row, the first of two symmetric anchors, anchor 0 for a box outside every anchor
    t = case("ties")
    assert t["argmax"][0].tolist()[:2] == [0, 0] and t["gt_argmax"].tolist()[:3] == [0, 0, 0]
    assert case("pyr128_outside_duplicates")["gt_argmax"][0] == 0
    assert case("pyr64_all_crowd")["status"].tolist() == [1, 0, 0]
    assert np.isneginf(case("hand20")["bbox_all"]).sum() == 3         # the zero-height box: dh; the zero-area box: dh and dw
    c8 = case("pyr64_b3_count8")
    assert (c8["match_u"] == 1).sum(1).max() > 4 >= (c8["match"] == 1).sum(1).max()
    h = case("hand20")
    assert np.array_equal(h["match"], h["match_u"])                   # fewer negatives than wanted: nothing is reset


def test_numpy_route_equals_every_array_of_the_fixture():
    from maskrcnn_amd import targets
    for c in cases():
        a, n = c["anchors"], c["anchors"].shape[0]
        first = 0
        for i, (boxes, ids) in enumerate(images(c)):
            s, e = c["off"][i], c["off"][i + 1]
            match, arg, iou, gt_arg, status = targets.match_numpy(a, boxes, ids)
            assert status == c["status"][i], c["name"]
            assert np.array_equal(match, c["match_u"][i]), c["name"]
            assert np.array_equal(gt_arg, c["gt_argmax"][s:e]), c["name"]
            if c["sparse"]:
                sel = c["u_idx"][(c["u_idx"] >= i * n) & (c["u_idx"] < (i + 1) * n)] - i * n
                where = (c["u_idx"] >= i * n) & (c["u_idx"] < (i + 1) * n)
                assert np.array_equal(arg[sel], c["u_argmax"][where]) and np.array_equal(iou[sel], c["u_iou"][where]), c["name"]
            else:
                assert np.array_equal(arg, c["argmax"][i]) and iou.dtype == np.float32 and np.array_equal(iou, c["iou_max"][i]), c["name"]
            npos = int(c["npos_all"][i])
            if status == 0:
                every, k = targets.deltas_numpy(a, boxes, match, arg, max(npos, 1))
                assert k == npos and np.array_equal(every[:npos], c["bbox_all"][first:first + npos]), c["name"]   # -inf included
            first += npos
            sampled = targets.sample_numpy(match, c["keys"][i], c["count"])
            assert np.array_equal(sampled, c["match"][i]), c["name"]
            if status == 0:
                bbox, _ = targets.deltas_numpy(a, boxes, sampled, arg, c["count"])
                assert bbox.dtype == np.float32 and np.array_equal(bbox, c["bbox"][i]), c["name"]
        if usable(c):
            for packed in (False, True):
                if packed:
                    m, b = targets.rpn_targets(a, c["boxes"], c["ids"], c["count"], keys=c["keys"], device="cpu", gt_off=c["off"])
                else:
                    bs, cs = zip(*images(c))
                    m, b = targets.rpn_targets(torch.from_numpy(a.copy()), list(bs), [torch.from_numpy(v.copy()) for v in cs], c["count"],
                                               keys=torch.from_numpy(c["keys"].copy()), device="cpu")
                assert m.dtype == torch.int32 and tuple(m.shape) == (c["batch"], n, 1) and b.dtype == torch.float32
                assert np.array_equal(m.numpy()[..., 0], c["match"]) and np.array_equal(b.numpy(), c["bbox"]), c["name"]


def test_both_matchers_agree_on_one_geometry():
    """match_numpy and roi_match_numpy restate one rule: on the same boxes the RoIs that reach pos_iou are the anchors whose
    iou_max does, matched to the same row. (test_gpu_targets.py asserts the same of the two kernels on this input.)"""
    from maskrcnn_amd import targets
    g = shared_geometry()
    assert np.array_equal(g["boxes"].astype(np.float32).astype(np.float64), g["boxes"])
    positives = []
    for i, (s, e) in enumerate(zip(g["off"][:-1], g["off"][1:])):
        boxes, ids = g["gt"][s:e], g["ids"][s:e]
        _, arg, iou, _, status = targets.match_numpy(g["boxes"], boxes, ids)
        cls, gt_index, roi_iou, roi_status = targets.roi_match_numpy(g["boxes"].astype(np.float32), boxes, ids, pos_iou=0.7)
        want = np.where((arg >= 0) & (iou >= np.float32(0.7)))[0]
        idx, p, q = targets.roi_sample_numpy(cls, g["keys"][i], 100, 1.0)
        assert status == roi_status == 0 and q == 0 and (idx[p:] == -1).all()
        assert sorted(idx[:p].tolist()) == want.tolist() and np.array_equal(gt_index[idx[:p]], arg[idx[:p]])
        assert np.array_equal(roi_iou.view(np.int32), iou.view(np.int32)) and np.array_equal(gt_index, arg)
        assert iou[0] == 0 and cls[0] == 1                                    # box 0 touches no row
        positives.append(len(want))
    assert positives[0] >= 1 and positives[1] >= 1
    # image 0: the rows themselves — the crowd and the id-0 row are never matched, the duplicate loses to row 0
    arg = targets.match_numpy(g["boxes"], g["gt"][:5], g["ids"][:5])[1]
    assert arg[1] == 0 and arg[5] == 0 and arg[4] == 3 and not np.isin(arg, [1, 2, 4]).any()
    ov = targets._overlaps(g["boxes"][7:8].astype(np.float32), g["gt"][[0, 3]])
    assert ov[0, 0] == ov[0, 1] == np.float32(0.2) and arg[7] == 0            # an exact tie between two rows: the first wins


def test_front_end_refuses_bad_ground_truth_on_the_host():
    from maskrcnn_amd import targets
    c = case("pyr64_all_crowd")
    bs, cs = zip(*images(c))
    with pytest.raises(ValueError, match="image 0 has no usable ground truth"):
        targets.rpn_targets(c["anchors"], list(bs), list(cs), device="cpu")
    with pytest.raises(ValueError, match="image 1 has no usable ground truth"):
        targets.rpn_targets(c["anchors"], [bs[1], np.zeros((0, 4), np.float32)], [cs[1], np.zeros(0, np.int32)], device="cpu")
    good_b, good_c = bs[2], cs[2]
    for bad in ([[5, 5, 4, 9]], [[5, 9, 8, 5]], [[0, 0, np.nan, 4]], [[0, 0, np.inf, 4]]):
        with pytest.raises(ValueError, match="image 1: boxes must be finite"):
            targets.rpn_targets(c["anchors"], [good_b, np.array(bad, np.float32)], [good_c, np.array([1], np.int32)], device="cpu")
    with pytest.raises(ValueError, match="at most 1024"):
        targets.rpn_targets(c["anchors"], [np.tile(good_b, (1025, 1))], [np.ones(1025, np.int32)], device="cpu")
    for bad in (np.array([[0, 0, 0, 5.0]]), np.array([[0, 0, np.nan, 5.0]]), np.zeros((0, 4))):
        with pytest.raises(ValueError, match="anchors"):
            targets.rpn_targets(bad, [good_b], [good_c], device="cpu")
    with pytest.raises(ValueError, match="count"):
        targets.rpn_targets(c["anchors"], [good_b], [good_c], count=0, device="cpu")
    with pytest.raises(ValueError, match="gt_off"):
        targets.rpn_targets(c["anchors"], c["boxes"], c["ids"], device="cpu", gt_off=np.array([0, 9], np.int32))


def test_default_keys_follow_the_generator_on_the_host_route():
    from maskrcnn_amd import targets
    c = case("pyr64_b3_count8")
    bs, cs = zip(*images(c))
    run = lambda seed: targets.rpn_targets(c["anchors"], list(bs), list(cs), 8, device="cpu", generator=torch.Generator().manual_seed(seed))
    (m1, b1), (m2, b2), (m3, _) = run(5), run(5), run(6)
    assert torch.equal(m1, m2) and torch.equal(b1, b2) and not torch.equal(m1, m3)
    assert ((m1 == 1).sum(1) <= 4).all() and ((m1 != 0).sum(1) == 8).all()
    assert (((m1[..., 0] == 1) <= torch.from_numpy(c["match_u"] == 1)) & ((m1[..., 0] == -1) <= torch.from_numpy(c["match_u"] == -1))).all()


def test_host_route_never_touches_the_library(monkeypatch):
    from maskrcnn_amd import ops, targets
    for name in ("anchor_match", "sample_by_key", "rpn_deltas"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("the host route called into the library"))
    c = case("hand20")
    bs, cs = zip(*images(c))
    targets.rpn_targets(c["anchors"], list(bs), list(cs), keys=c["keys"], device="cpu")


def test_header_declares_and_library_exports_the_entry_points():
    from maskrcnn_amd import _lib
    protos = _lib.header_prototypes()
    i32, f32, vp, sz, dbl = ctypes.c_int32, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double
    for name in ENTRY_POINTS:
        assert name in _lib.declared_symbols() and hasattr(_lib.lib, name), name
    assert protos["mrcnn_anchor_match"] == (ctypes.c_int, [vp, i32, vp, vp, vp, i32, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp, sz, vp])
    assert protos["mrcnn_sample_by_key"] == (ctypes.c_int, [vp, vp, i32, i32, i32, vp, vp, sz, vp])
    assert protos["mrcnn_rpn_deltas"] == (ctypes.c_int, [vp, i32, vp, vp, i32, i32, vp, vp, i32, ctypes.POINTER(dbl), vp, vp, vp, sz, vp])
    assert protos["mrcnn_anchor_match_workspace_bytes"] == (sz, [i32]) and protos["mrcnn_sample_by_key_workspace_bytes"] == (sz, [i32])
    assert protos["mrcnn_rpn_deltas_workspace_bytes"] == (sz, [i32, i32])
    for name in ENTRY_POINTS:
        fn = getattr(_lib.lib, name)
        assert (fn.restype, list(fn.argtypes)) == protos[name], name
    assert _lib.lib.mrcnn_abi_version() == _lib.header_abi_version() >= 24


def test_source_is_built_without_fma_contraction_or_fast_math():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mrcnn_build", f"{ROOT}/maskrcnn_amd/build.py")
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    for src in ("targets.hip", "detection_targets.hip"):       # both include the shared matching rule (csrc/target_match.hpp)
        assert "-ffp-contract=off" in build.SOURCES[src], src
        flags = build.COMMON + build.SOURCES[src]
        assert "-fno-fast-math" in flags, src
        # nothing that lets the compiler approximate the IoU's division
        assert not [f for f in flags if re.search(r"fast-math|unsafe-math|reciprocal|approx|no-hip-fp32-correctly-rounded|finite-math", f)
                    and f != "-fno-fast-math"], src
        assert '#include "target_match.hpp"' in open(f"{ROOT}/maskrcnn_amd/csrc/{src}").read(), src
    assert "built with FP contraction off" in open(f"{ROOT}/maskrcnn_amd/csrc/target_match.hpp").read()


def test_entry_points_refuse_the_limits_before_touching_a_pointer():
    """Argument validation runs before any HIP call (no GPU needed; the dummy pointers are never read)."""
    from maskrcnn_amd import _lib
    lib = _lib.lib
    p = ctypes.c_void_p(4096)
    std = (ctypes.c_double * 4)(0.1, 0.1, 0.2, 0.2)
    err = lambda: lib.mrcnn_last_error().decode()

    def match(a=1008, m=6, b=1, ws=1 << 20):
        return lib.mrcnn_anchor_match(p, a, p, p, p, m, b, 0.3, 0.7, 0.001, p, p, p, p, p, p, ws, None)

    def sample(a=1008, b=1, count=128, ws=1 << 30):
        return lib.mrcnn_sample_by_key(p, p, b, a, count, p, p, ws, None)

    def deltas(a=1008, m=6, b=1, count=128, ws=1 << 20):
        return lib.mrcnn_rpn_deltas(p, a, p, p, m, b, p, p, count, std, p, p, p, ws, None)

    for call in (match, sample, deltas):
        for kw, text in ((dict(a=0), "num_anchors=0"), (dict(a=(1 << 24) + 1), "num_anchors"), (dict(b=0), "batch=0"),
                         (dict(b=65536), "batch=65536"), (dict(a=1 << 24, b=128), "too large")):
            assert call(**kw) == -1 and text in err(), (call.__name__, kw, err())
    for call in (match, deltas):
        assert call(m=1025) == -1 and "at most 1024 rows per image" in err()
        assert call(m=2049, b=2) == -1 and "at most 1024 rows per image" in err()
        assert call(m=-1) == -1 and "num_rows" in err()
    for call in (sample, deltas):
        assert call(count=0) == -1 and "count=0" in err()
        assert call(count=-5) == -1 and "count=-5" in err()
    assert match(ws=8 * 6 - 1) == -1 and "workspace" in err()
    assert sample(ws=64) == -1 and "workspace" in err()
    assert deltas(ws=3) == -1 and "workspace" in err()
    assert lib.mrcnn_anchor_match(None, 1008, p, p, p, 6, 1, 0.3, 0.7, 0.001, p, p, p, p, p, p, 1 << 20, None) == -1 and "null" in err()
    assert lib.mrcnn_anchor_match_workspace_bytes(6) >= 48 and lib.mrcnn_anchor_match_workspace_bytes(0) == 0
    assert lib.mrcnn_sample_by_key_workspace_bytes(2) == 2 * lib.mrcnn_sample_by_key_workspace_bytes(1) > 0
    assert lib.mrcnn_rpn_deltas_workspace_bytes(3, 261888) >= 3 * 4 * ((261888 + 4095) // 4096)


def test_public_interface_and_cpu_refusal():
    from maskrcnn_amd import ops, targets
    for name in ("anchor_match", "sample_by_key", "rpn_deltas"):
        assert name in ops.__all__ and hasattr(torch.ops.maskrcnn, name), name
    a = torch.zeros(4, 4, dtype=torch.float64)
    boxes, ids, off = torch.zeros(1, 4), torch.ones(1, dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32)
    match, keys = torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32)
    for call in (lambda: ops.anchor_match(a, boxes, ids, off), lambda: ops.sample_by_key(match, keys, 8),
                 lambda: ops.rpn_deltas(a, boxes, off, match, match, 8), lambda: torch.ops.maskrcnn.anchor_match(a, boxes, ids, off),
                 lambda: torch.ops.maskrcnn.sample_by_key(match, keys, 8),
                 lambda: torch.ops.maskrcnn.rpn_deltas(a, boxes, off, match, match, 8, [0.1, 0.1, 0.2, 0.2])):
        with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
            call()
    assert targets.MAX_ROWS_PER_IMAGE == 1024 and "rpn_targets" in targets.__all__


def test_pyramid_anchors_default_is_unchanged_and_float64_narrows_to_it():
    from maskrcnn_amd import anchors
    from maskrcnn_amd.config import InferenceConfig
    cfg = InferenceConfig()
    a32, a64 = anchors.pyramid_anchors(cfg), anchors.pyramid_anchors(cfg, dtype=torch.float64)
    # the rule of the module's docstring, written out again: corners in float64, then narrowed
    parts = [anchors.level_anchors(cfg.rpn_anchor_scales[i], cfg.rpn_anchor_ratios, cfg.backbone_shapes[i], cfg.backbone_strides[i],
                                   cfg.rpn_anchor_stride) for i in range(5)]
    want = torch.from_numpy(np.concatenate(parts, axis=0))
    assert a32.dtype == torch.float32 and tuple(a32.shape) == (261888, 4) and torch.equal(a32, want.float())
    assert a64.dtype == torch.float64 and torch.equal(a64, want) and torch.equal(a64.float(), a32)
    assert torch.equal(anchors.pyramid_anchors(cfg, dtype=torch.float32), a32)
    for name in ("pyr64", "pyr128"):       # the reference's create_pyramid_anchors, from the fixture
        got = anchors.pyramid_anchors(pyramid_config(name), dtype=torch.float64).numpy()
        assert np.array_equal(got, load_golden("targets")["anchors_" + name]), name
    with pytest.raises(ValueError):
        anchors.pyramid_anchors(cfg, dtype=torch.float16)
