"""GPU tests (-m gpu) of predict() at its largest batch, pipeline.max_batch_per_launch.

max_batch_per_launch promises that up to that batch no layer's kernel choice depends on the batch and no launch is refused, which
is what makes image i of a batch equal image i alone, bit for bit. The other tests hold it far from the limit (batch 1 against 8 or
2). Here each case runs the step at the limit itself, where the largest tensor lies in the top part of the 32-bit offset range:

  routing        the sequence of (kernel, N, K) of every conv launch (ops.CONV_PROFILE) at the largest batch equals the one of a
                 single image (repeated once per sub-batch when predict() splits the batch);
  bit identity   images 0, b // 2 and b - 1 run alone equal their slices of the batch (torch.equal): the pyramid, RPN scores
                 and dets, RoIs and counts and the logits where return_intermediates is allowed; detections and masks always;
  non-degenerate some image has a detection;
  at the limit   the tensor that bounds the batch is within 10 % of its byte limit, and one more image would pass it.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_BUFFER_BYTES = 0xFFFFFFF0   # csrc/conv_common.hpp (the fp32 kernels' limit)
F16_LIMIT = 1 << 31             # the fp16 family's tensors stay below this (csrc/conv_f16p.hip)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import maskrcnn_amd  # noqa: F401
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _free_between_cases():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _state_dict(arch, seed):
    """The full-size tests' synthetic weights, with the class / bbox layers scaled so that detections exist."""
    from maskrcnn_amd import modules
    sd = modules.synthetic_state_dict(arch, seed=0, bn_seed=1)
    g = torch.Generator().manual_seed(seed)
    sd["classifier.linear_class.weight"] = torch.randn(81, 1024, generator=g) * 0.05
    sd["classifier.linear_class.bias"] = torch.randn(81, generator=g) * 0.5
    sd["classifier.linear_bbox.weight"] = torch.randn(324, 1024, generator=g) * 0.02
    sd["rpn.conv_bbox.bias"] = torch.randn(12, generator=g) * 0.3
    return sd


def _calibrated_net(sd, cfg, image, window, dev, **kw):
    """Random weights saturate the RPN's scores and blow its deltas up: rescale the head layers (weights only) on one image
    until both are sane (as tests/test_gpu_fullsize.py does), so that the batch's RPN scores are distinct and proposals vary."""
    from maskrcnn_amd.pipeline import MaskRCNNInference
    for _ in range(4):
        net = MaskRCNNInference(sd, cfg, dev, **kw)
        _, mid = net.predict(image, window, return_intermediates=True)
        sc = mid["rpn_scores"].double().clamp(1e-7, 1 - 1e-7)
        sat, dstd = torch.log(sc / (1 - sc)).std().item(), mid["rpn_deltas"].std().item()
        done = True
        for key, cur, target, limit in (("rpn.conv_class.weight", sat, 1.0, 2.0), ("rpn.conv_bbox.weight", dstd, 0.5, 1.0)):
            if cur > limit:
                sd[key] = sd[key] * (target / cur)
                done = False
        if done:
            return net
        del net, mid
    return MaskRCNNInference(sd, cfg, dev, **kw)


def _images(cfg, b, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (b, cfg.image_height, cfg.image_width, 3), generator=g).float() - torch.tensor(cfg.mean_pixel)
    return x.permute(0, 3, 1, 2).contiguous().to(dev)


def _routing(net, images, windows):
    from maskrcnn_amd import ops
    ops.CONV_PROFILE = []
    try:
        net.predict(images, windows)
        torch.cuda.synchronize()
        prof = ops.CONV_PROFILE
    finally:
        ops.CONV_PROFILE = None
    return [(r[5] if len(r) > 5 else "direct", r[3][1], r[3][2]) for r in prof]


def _check_detections(det1, det, i, what):
    for f in ("class_ids", "scores", "boxes", "counts", "masks"):
        assert torch.equal(getattr(det1, f)[0], getattr(det, f)[i]), f"{what}: image {i}: {f} differs from the image alone"


def _check_at_max_batch(net, cfg, dev, b, intermediates, seed, what):
    images = _images(cfg, b, seed, dev)
    windows = torch.tensor([[0., 0., float(cfg.image_height), float(cfg.image_width)]] * b, device=dev)
    # routing: one image against the largest batch (split batches repeat the one-image sequence once per sub-batch)
    one = _routing(net, images[:1], windows[:1])
    parts = -(-b // net.max_batch)
    seq = _routing(net, images, windows)
    assert seq == one * parts, (what, [(k, a, c) for k, (a, c) in enumerate(zip(one * parts, seq)) if a != c][:5],
                                len(one) * parts, len(seq))
    # bit identity with images run alone
    if intermediates:
        det, mid = net.predict(images, windows, return_intermediates=True)
    else:
        det, mid = net.predict(images, windows), None
    torch.cuda.synchronize()
    assert int(det.counts.max()) > 0, f"{what}: no detections at all"
    p = None if mid is None else mid["rois"].size(1)
    for i in sorted({0, b // 2, b - 1}):
        if mid is None:
            det1 = net.predict(images[i:i + 1], windows[i:i + 1])
        else:
            det1, mid1 = net.predict(images[i:i + 1], windows[i:i + 1], return_intermediates=True)
            for lvl, (a, c) in enumerate(zip(mid1["feature_maps"], mid["feature_maps"])):
                assert torch.equal(a[0], c[i]), f"{what}: image {i}: P{lvl + 2} differs from the image alone"
            for k in ("rpn_scores", "rpn_dets", "rois", "roi_counts"):
                assert torch.equal(mid1[k][0], mid[k][i]), f"{what}: image {i}: {k} differs from the image alone"
            assert torch.equal(mid1["logits"], mid["logits"][i * p:(i + 1) * p]), f"{what}: image {i}: logits differ"
            del mid1
        torch.cuda.synchronize()
        _check_detections(det1, det, i, what)
        del det1
    return det, mid


def test_predict_at_max_batch_f32_r50_1024(dev):
    """configs[2] (R50-FPN, 1024^2, 1000 proposals) at its largest batch, 31 images: the RPN's shared activation on P2 would be
    4.16 GB (0.97 of MAX_BUFFER_BYTES; the fused heads kernel never writes it) and P2 itself is 2.08 GB (0.97 of 2^31)."""
    from maskrcnn_amd.config import InferenceConfig
    from maskrcnn_amd.pipeline import max_batch_per_launch
    cfg = InferenceConfig(image_height=1024, image_width=1024, backbone="resnet50", pre_nms_limit=1000, proposal_count=1000,
                          detection_max_instances=50)
    b = max_batch_per_launch(cfg)
    assert b == 31
    shared = lambda n: 4 * n * (1024 // 4) * (1024 // 4) * 512
    assert 0.9 * MAX_BUFFER_BYTES < shared(b) <= MAX_BUFFER_BYTES < shared(b + 1)
    w1 = torch.tensor([[0., 0., 1024., 1024.]], device=dev)
    net = _calibrated_net(_state_dict("resnet50", 5), cfg, _images(cfg, 1, 99, dev), w1, dev)
    assert net.max_batch == b
    det, mid = _check_at_max_batch(net, cfg, dev, b, True, 31, "f32 R50 1024^2")
    p2 = mid["feature_maps"][0]
    assert p2.dtype == torch.float32 and 0.95 * F16_LIMIT < p2.numel() * 4 < F16_LIMIT


def test_predict_at_max_batch_f16_r101_832x1344_one_pass(dev):
    """configs[4]'s geometry (R101-FPN, 832 x 1344) in the "f16" mode, one pass (concurrent_sub_batches=1) at net.max_batch: the
    pipelined fp16 kernel counts the RPN's P2 shared activation at 4 bytes per element (4 * 15 * 208 * 336 * 512 = 0.99998 of
    2^31) though its heads form never writes it. Past 15 images P2's RPN left conv_f16_pipelined_heads for the tile kernel and a
    separate head conv, which sum the heads in another grouping: the RPN scores of image i then differ from image i alone."""
    from maskrcnn_amd.config import InferenceConfig
    h, w = 832, 1344
    cfg = InferenceConfig(image_height=h, image_width=w, backbone="resnet101", pre_nms_limit=1000, proposal_count=1000)
    w1 = torch.tensor([[0., 0., float(h), float(w)]], device=dev)
    net = _calibrated_net(_state_dict("resnet101", 7), cfg, _images(cfg, 1, 98, dev), w1, dev, precision="f16",
                          concurrent_sub_batches=1)
    b = net.max_batch
    _check_at_max_batch(net, cfg, dev, b, True, 15, "f16 R101 832x1344")
    shared = lambda n: 4 * n * (h // 4) * (w // 4) * 512
    assert b == 15 and 0.9 * F16_LIMIT < shared(b) < F16_LIMIT <= shared(b + 1)


@pytest.mark.parametrize("hw,b", [((1024, 1024), 31), ((832, 1344), 30)], ids=["1024x1024", "832x1344"])
def test_predict_f16_default_constructor_at_the_fp32_bound(dev, hw, b):
    """The "f16" mode through the public path (default constructor: two concurrent sub-batches for even batches) at the largest
    batch the fp32 bound allows: predict() splits it into sub-batches of at most net.max_batch (15) images, each of which keeps
    the one-image routing, and every image equals itself alone. (31 images at 1024^2 used to run as one pass: 31 is odd.)"""
    from maskrcnn_amd.config import InferenceConfig
    from maskrcnn_amd.pipeline import max_batch_per_launch
    h, w = hw
    cfg = InferenceConfig(image_height=h, image_width=w)
    assert max_batch_per_launch(cfg) == b
    w1 = torch.tensor([[0., 0., float(h), float(w)]], device=dev)
    net = _calibrated_net(_state_dict(cfg.backbone, 9), cfg, _images(cfg, 1, 97, dev), w1, dev, precision="f16")
    assert net.max_batch == 15 and net.sub_batches == 2
    _check_at_max_batch(net, cfg, dev, b, False, b, f"f16 default {h}x{w}")
