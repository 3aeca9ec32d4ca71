"""GPU parity (-m gpu) of the COCO RLE encoder (csrc/rle.hip): every comparison is exact (integer / byte work). References:
the golden vectors made with the reference's own codec (tests/golden/rle.npz) and a numpy restatement of rleEncode /
rleToString / rleArea / rleToBbox below (the same statement equalled the compiled codec on every golden case:
test_restatement_equals_the_golden_vectors)."""
import json

import numpy as np
import pytest
import torch

from test_rle_host import golden_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ops():
    from maskrcnn_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------ numpy restatement
def np_string(cnts) -> bytes:
    out = bytearray()
    cnts = [int(c) for c in cnts]
    for i, x in enumerate(cnts):
        if i > 2:
            x -= cnts[i - 2]
        more = True
        while more:
            c = x & 31
            x >>= 5
            more = (x != -1) if (c & 16) else (x != 0)
            if more:
                c |= 32
            out.append(c + 48)
    return bytes(out)


def np_rle(mask: np.ndarray):
    """(counts, string, area, bbox [x, y, w, h]) of a boolean [h, w] mask."""
    h, w = mask.shape
    v = np.ascontiguousarray(mask.T).reshape(-1)                    # column-major: j = x*h + y
    change = np.empty(v.size, bool)
    change[0] = v[0]                                                # v(-1) = 0
    np.not_equal(v[1:], v[:-1], out=change[1:])
    pos = np.flatnonzero(change)
    cnts = np.diff(np.concatenate([[0], pos, [h * w]])).astype(np.int64)
    area = int(cnts[1::2].sum())
    if area:
        cols, rows = np.flatnonzero(mask.any(0)), np.flatnonzero(mask.any(1))
        bbox = [int(cols[0]), int(rows[0]), int(cols[-1] - cols[0] + 1), int(rows[-1] - rows[0] + 1)]
    else:
        bbox = [0, 0, 0, 0]
    return cnts, np_string(cnts), area, bbox


def test_restatement_equals_the_golden_vectors():
    for c in golden_cases():
        cnts, s, area, bbox = np_rle(c["mask"])
        assert np.array_equal(cnts, c["counts"]) and s == c["string"] and area == c["area"] and bbox == c["bbox"], c["name"]


def check(enc, i, want, name=""):
    """Row i of an encode (the six tensors) against (counts, string, area, bbox)."""
    num_runs, counts, strings, string_bytes, areas, bboxes = enc
    cnts, s, area, bbox = want
    k = int(num_runs[i])
    assert k == len(cnts), (name, k, len(cnts))
    assert np.array_equal(counts[i, :k].cpu().numpy().view(np.uint32), np.asarray(cnts, dtype=np.uint32)), name
    nb = int(string_bytes[i])
    assert nb == len(s) and strings[i, :nb].cpu().numpy().tobytes() == s, name
    assert int(areas[i]) == area and bboxes[i].tolist() == list(bbox), (name, int(areas[i]), bboxes[i].tolist(), area, bbox)


# ------------------------------------------------------------------------------------------------ the C ABI, directly
class Abi:
    """mrcnn_rle_encode_u8 called through ctypes on buffers the test owns: every output sits between two guard bands and is
    pre-filled with a sentinel, so both 'not written' and 'nothing written outside' can be seen."""
    GUARD = 256

    def __init__(self, n, capacity):
        self.n, self.capacity = n, capacity
        g = self.GUARD
        new = lambda nbytes: torch.full((g + nbytes + g,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.raw = dict(num_runs=new(4 * n), counts=new(4 * n * capacity), strings=new(6 * n * capacity),
                        string_bytes=new(4 * n), areas=new(4 * n), bboxes=new(16 * n))

    def body(self, key):
        return self.raw[key][self.GUARD:-self.GUARD]

    def ptr(self, key):
        return self.body(key).data_ptr()

    def call(self, masks, threshold, h=None, w=None, row_stride=None, null=(), n=None, capacity=None):
        from maskrcnn_amd._lib import lib
        n = self.n if n is None else n
        h = masks.size(1) if h is None else h
        w = masks.size(2) if w is None else w
        nbytes = int(lib.mrcnn_rle_workspace_bytes(n, min(h, 16384), min(w, 16384)))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
        p = {k: (None if k in null else self.ptr(k)) for k in self.raw}
        rc = lib.mrcnn_rle_encode_u8(None if "masks" in null else masks.data_ptr(), masks.stride(0),
                                     masks.stride(1) if row_stride is None else row_stride, n, h, w, threshold,
                                     self.capacity if capacity is None else capacity, p["num_runs"], p["counts"], p["strings"],
                                     p["string_bytes"], p["areas"], p["bboxes"], None if "workspace" in null else ws.data_ptr(),
                                     nbytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    def guards_intact(self):
        g = self.GUARD
        return all(bool((t[:g] == SENTINEL).all()) and bool((t[-g:] == SENTINEL).all()) for t in self.raw.values())

    def untouched(self, keys=None):
        return all(bool((self.raw[k] == SENTINEL).all()) for k in (keys or self.raw))

    def tensors(self):
        n, c = self.n, self.capacity
        i32 = lambda k, *shape: self.body(k).view(torch.int32).view(*shape)
        return (i32("num_runs", n), i32("counts", n, c), self.body("strings").view(n, 6 * c), i32("string_bytes", n),
                i32("areas", n), i32("bboxes", n, 4))


def cropped_view(masks: np.ndarray, top=3, left=5, extra=(4, 7), on=1):
    """The masks [n,h,w] as a view into a larger, noise-filled uint8 tensor: odd origin, row stride > w, image stride > h*w."""
    n, h, w = masks.shape
    rng = np.random.default_rng(h * 131 + w)
    big = rng.integers(0, 256, (n, h + top + extra[0], w + left + extra[1]), dtype=np.uint8)
    big[:, top:top + h, left:left + w] = masks.astype(np.uint8) * on
    return torch.from_numpy(big).to(DEV)[:, top:top + h, left:left + w]


# ------------------------------------------------------------------------------------------------ 1 golden cases
def test_golden_through_ops(ops):
    for c in golden_cases():
        m = torch.from_numpy(c["mask"]).to(DEV)
        want = (c["counts"], c["string"], c["area"], c["bbox"])
        capacity = max(len(c["counts"]), 1)
        check(ops.rle_encode(m[None], capacity=capacity), 0, want, c["name"])                    # bool [1,h,w], exact fit
        check(ops.rle_encode(m.to(torch.uint8) * 255, capacity=capacity + 3), 0, want, c["name"])  # uint8 0/255 [h,w]
        if len(c["counts"]) <= ops.rle_default_capacity(*c["mask"].shape):
            check(ops.rle_encode(m), 0, want, c["name"])


def test_golden_through_the_c_abi_with_cropped_views():
    for c in golden_cases():
        want = (c["counts"], c["string"], c["area"], c["bbox"])
        view = cropped_view(c["mask"][None], on=200)                 # on pixels are 200, off pixels 0, noise all around
        abi2 = Abi(1, len(c["counts"]) + 2)
        assert abi2.call(view, 100) == 0, c["name"]
        check(abi2.tensors(), 0, want, c["name"])
        assert abi2.guards_intact(), c["name"]
        # counts only / strings only / neither
        for null in (("strings",), ("counts",), ("counts", "strings")):
            a = Abi(1, len(c["counts"]) + 2)
            assert a.call(view, 0, null=null) == 0, (c["name"], null)
            assert a.untouched(null) and a.guards_intact(), (c["name"], null)
            num_runs, counts, strings, string_bytes, areas, bboxes = a.tensors()
            assert int(num_runs[0]) == len(c["counts"]) and int(areas[0]) == c["area"] and bboxes[0].tolist() == c["bbox"]
            assert int(string_bytes[0]) == len(c["string"])
            if "counts" not in null:
                assert np.array_equal(counts[0, :len(c["counts"])].cpu().numpy().view(np.uint32), c["counts"])
            if "strings" not in null:
                assert strings[0, :len(c["string"])].cpu().numpy().tobytes() == c["string"]


def test_golden_through_the_dispatcher(ops):
    for c in golden_cases():
        m = torch.from_numpy(c["mask"]).to(DEV)
        enc = torch.ops.maskrcnn.rle_encode(m[None], 0, max(len(c["counts"]), 1))
        assert len(enc) == 6 and enc[1].dtype == torch.int32 and enc[2].dtype == torch.uint8
        check(enc, 0, (c["counts"], c["string"], c["area"], c["bbox"]), c["name"])


# ------------------------------------------------------------------------------------------------ 2 restatement
def test_random_shapes_and_batches_vs_restatement(ops):
    rng = np.random.default_rng(7)
    shapes = [(37, 53), (1, 1), (2, 3), (64, 64), (100, 31), (31, 100), (257, 129), (40, 1), (1, 40), (513, 66), (90, 2049)]
    shapes += [tuple(int(v) for v in rng.integers(1, 70, 2)) for _ in range(20)]
    shapes += [(5, 1024), (5, 1025)]      # one segment of rows: 1024 and 1025 cells, a cell a thread of the scan and one more
    for h, w in shapes:
        n = int(rng.integers(1, 6))
        masks = rng.random((n, h, w)) < rng.choice([0.03, 0.3, 0.5, 0.9])
        enc = ops.rle_encode(torch.from_numpy(masks).to(DEV), capacity=h * w + 1)
        for i in range(n):
            check(enc, i, np_rle(masks[i]), (h, w, i))
        enc = ops.rle_encode(cropped_view(masks), capacity=h * w + 1)           # strided view through the binding
        for i in range(n):
            check(enc, i, np_rle(masks[i]), (h, w, i, "view"))


def test_empty_batch(ops):
    enc = ops.rle_encode(torch.zeros(0, 37, 53, dtype=torch.uint8, device=DEV))
    assert [tuple(t.shape) for t in enc] == [(0,), (0, 1024), (0, 6 * 1024), (0,), (0,), (0, 4)]
    abi = Abi(1, 4)
    assert abi.call(torch.zeros(1, 8, 8, dtype=torch.uint8, device=DEV), 0, n=0) == 0 and abi.untouched()


def test_grey_levels_at_threshold_127(ops):
    rng = np.random.default_rng(8)
    for h, w in ((37, 53), (120, 200), (64, 3)):
        grey = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
        grey[0, :5, :2] = [[127, 128], [128, 127], [0, 255], [126, 129], [127, 127]][:5] if w >= 2 else 0
        enc = ops.rle_encode(torch.from_numpy(grey).to(DEV), threshold=127, capacity=h * w + 1)
        for i in range(3):
            check(enc, i, np_rle(grey[i] > 127), (h, w, i))
        enc = ops.rle_encode(torch.from_numpy(grey).to(DEV), threshold=254, capacity=h * w + 1)
        check(enc, 1, np_rle(grey[1] > 254), (h, w, "254"))


def test_batches_mixing_empty_full_and_checkerboard(ops):
    h, w = 48, 52
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(9)
    kinds = [np.zeros((h, w), bool), np.ones((h, w), bool), (yy + xx) % 2 == 0, (yy + xx) % 2 == 1, rng.random((h, w)) < 0.5,
             np.zeros((h, w), bool), np.ones((h, w), bool)]
    masks = np.stack([kinds[i] for i in rng.permutation(len(kinds))] + kinds)
    enc = ops.rle_encode(torch.from_numpy(masks).to(DEV), capacity=h * w + 1)
    for i in range(len(masks)):
        check(enc, i, np_rle(masks[i]), i)


# ------------------------------------------------------------------------------------------------ 3 full size
def pasted_masks(ops, n=50, height=1200, width=1920, seed=3):
    """n masks as detect() makes them: seeded 28 x 28 sigmoid masks pasted by ops.paste_masks at seeded boxes."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, 28), torch.linspace(-1, 1, 28), indexing="ij")
    blobs = []
    for _ in range(n):
        a, b, c = (torch.rand(3, generator=g) * 0.8 + 0.3).tolist()
        field = 1.0 - (xx / a) ** 2 - (yy / b) ** 2 + c * 0.3 * torch.sin(5 * xx) * torch.cos(4 * yy)
        blobs.append(torch.sigmoid(4 * field + 0.5 * torch.randn(28, 28, generator=g)))
    m28 = torch.stack(blobs)[:, :, :, None].contiguous()                      # [n,28,28,1]
    y1 = torch.rand(n, generator=g) * (height - 80)
    x1 = torch.rand(n, generator=g) * (width - 80)
    y2 = torch.minimum(y1 + 40 + torch.rand(n, generator=g) * 700, torch.tensor(float(height)))
    x2 = torch.minimum(x1 + 40 + torch.rand(n, generator=g) * 900, torch.tensor(float(width)))
    boxes = torch.stack([y1, x1, y2, x2], 1)
    return ops.paste_masks(m28.to(DEV), torch.zeros(n, dtype=torch.int64, device=DEV), boxes.to(DEV), height, width,
                           channels_last=True)


def test_full_size_pasted_masks_twice_the_same_bits(ops):
    masks = pasted_masks(ops)
    assert masks.dtype == torch.bool and tuple(masks.shape) == (50, 1200, 1920)
    host = masks.cpu().numpy()
    assert int(host.any((1, 2)).sum()) >= 45                                  # real masks, not empty canvases
    first = ops.rle_encode(masks)
    assert int(first[0].max()) <= first[1].size(1)                            # they fit the default capacity
    for i in range(50):
        check(first, i, np_rle(host[i]), i)
    second = ops.rle_encode(masks)
    for a, b, i in zip(first, second, range(6)):
        if i in (1, 2):                                                       # counts / strings: the written part
            lens = first[0] if i == 1 else first[3]
            live = torch.arange(a.size(1), device=DEV)[None, :] < lens[:, None]
            assert torch.equal(a[live], b[live])
        else:
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 4 at the limit
def test_largest_mask(ops):
    side = 16384
    m = torch.zeros(1, side, side, dtype=torch.uint8, device=DEV)
    enc = ops.rle_encode(m)
    assert int(enc[0][0]) == 1 and int(enc[1][0, 0]) == side * side == 1 << 28
    assert enc[2][0, :int(enc[3][0])].cpu().numpy().tobytes() == np_string([1 << 28]) and int(enc[3][0]) == 6
    assert int(enc[4][0]) == 0 and enc[5][0].tolist() == [0, 0, 0, 0]
    rects = [(0, 0, 1, 1), (5, 7, 9000, 12000), (16000, 16001, 16384, 16384), (10000, 13000, 16384, 13003), (0, 16383, 3, 16384)]
    host = np.zeros((side, side), bool)
    for y1, x1, y2, x2 in rects:
        m[0, y1:y2, x1:x2] = 1
        host[y1:y2, x1:x2] = True
    enc = ops.rle_encode(m)
    check(enc, 0, np_rle(host), "rects")
    assert max(int(v) for v in np_rle(host)[0]) > 1 << 25                     # six-character groups are in the string
    m.fill_(1)
    enc = ops.rle_encode(m, capacity=2)
    check(enc, 0, ([0, 1 << 28], np_string([0, 1 << 28]), 1 << 28, [0, 0, side, side]), "full")


# ------------------------------------------------------------------------------------------------ 5 overflow
def test_overflow_leaves_the_row_alone():
    h = w = 64
    yy, xx = np.mgrid[0:h, 0:w]
    rect = np.zeros((h, w), bool)
    rect[10:30, 20:50] = True
    ell = ((yy - 30) / 20.0) ** 2 + ((xx - 33) / 15.0) ** 2 <= 1
    # 4 097 runs: the mask that changes at EVERY pixel of the column-major order and starts on (a leading 0 count). On 64 rows
    # that is every other row; the (y + x) checkerboard proper joins runs across the column boundaries and has 4 033.
    every = (xx * h + yy) % 2 == 0
    checker = (yy + xx) % 2 == 1
    masks = np.stack([rect, ell, every, np.zeros((h, w), bool), checker, rect.T.copy()])
    fit, over = (0, 1, 3, 5), (2, 4)
    assert len(np_rle(every)[0]) == 4097 and len(np_rle(checker)[0]) == 4033
    assert all(len(np_rle(masks[i])[0]) <= 100 for i in fit)
    abi = Abi(6, 100)
    assert abi.call(cropped_view(masks), 0) == 0
    enc = abi.tensors()
    for i in fit:
        check(enc, i, np_rle(masks[i]), i)
    assert int(enc[0][2]) == 4097 and int(enc[0][4]) == 4033
    for i in over:
        assert int(enc[3][i]) == 0
        assert int(enc[4][i]) == h * w // 2 == np_rle(masks[i])[2] and enc[5][i].tolist() == np_rle(masks[i])[3]
        assert bool((enc[1][i].view(torch.uint8) == SENTINEL).all()) and bool((enc[2][i] == SENTINEL).all())
    assert enc[5][2].tolist() == [0, 0, 64, 63] and enc[5][4].tolist() == [0, 0, 64, 64]
    assert abi.guards_intact()
    # ... and the rows of the masks that fit are written up to their length only
    for i in fit:
        k, nb = int(enc[0][i]), int(enc[3][i])
        assert bool((enc[1][i, k:].view(torch.uint8) == SENTINEL).all()) and bool((enc[2][i, nb:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 6 refusals
def test_refusals_leave_the_outputs_untouched(ops):
    from maskrcnn_amd._lib import MaskrcnnHipError, lib
    m = torch.ones(2, 16, 20, dtype=torch.uint8, device=DEV)
    wide = torch.ones(1, 1, 16385, dtype=torch.uint8, device=DEV)
    tall = torch.ones(1, 16385, 1, dtype=torch.uint8, device=DEV)
    for what, kw, src in (("threshold 255", dict(threshold=255), m), ("threshold -1", dict(threshold=-1), m),
                          ("capacity 0", dict(threshold=0, capacity=0), m), ("width 16385", dict(threshold=0), wide),
                          ("height 16385", dict(threshold=0), tall), ("row stride", dict(threshold=0, row_stride=19), m),
                          ("n", dict(threshold=0, n=65536), m),
                          *[(f"null {k}", dict(threshold=0, null=(k,)), m)
                            for k in ("masks", "num_runs", "string_bytes", "areas", "bboxes", "workspace")]):
        abi = Abi(2, 8)
        rc = abi.call(src, **kw)
        assert rc != 0 and lib.mrcnn_last_error().decode().startswith("rle_encode"), what
        assert abi.untouched(), what
    with pytest.raises(MaskrcnnHipError):
        ops.rle_encode(m, threshold=255)
    with pytest.raises(MaskrcnnHipError):
        ops.rle_encode(m, capacity=0)
    with pytest.raises(MaskrcnnHipError):
        ops.rle_encode(wide)
    with pytest.raises(RuntimeError):
        ops.rle_encode(m.permute(0, 2, 1))                                    # last stride != 1
    with pytest.raises(RuntimeError):
        ops.rle_encode(m.float())


# ------------------------------------------------------------------------------------------------ 7 detect
def small_net():
    from maskrcnn_amd import modules
    from maskrcnn_amd.config import InferenceConfig
    from maskrcnn_amd.pipeline import MaskRCNNInference
    cfg = InferenceConfig(image_height=256, image_width=256, image_min_dim=200, image_max_dim=256, backbone="resnet50",
                          pre_nms_limit=300, proposal_count=100, detection_max_instances=10)
    sd = modules.synthetic_state_dict("resnet50", seed=0, bn_seed=1)
    g = torch.Generator().manual_seed(5)
    sd["classifier.linear_class.weight"] = torch.randn(81, 1024, generator=g) * 0.05
    sd["classifier.linear_class.bias"] = torch.randn(81, generator=g) * 0.5
    return MaskRCNNInference(sd, cfg, DEV)


def compare_detect(net, images, min_total=1):
    from maskrcnn_amd import image as imagelib
    dense = net.detect(images)
    rle = net.detect(images, mask_format="rle")
    assert len(dense) == len(rle) == len(images)
    total = 0
    for i, (d, r) in enumerate(zip(dense, rle)):
        if d[0] is None:
            assert r == (None, None, None, None), i
            continue
        for a, b in zip(d[:3], r[:3]):
            assert a.dtype == b.dtype and torch.equal(a, b), i
        masks, enc = d[3], r[3]
        assert isinstance(enc, imagelib.RleMasks) and len(enc) == masks.size(0) and enc.size == tuple(masks.shape[1:])
        want = masks if masks.dtype == torch.bool else masks > 127
        assert (masks.dtype == torch.bool) == (tuple(masks.shape[1:]) == (256, 256)), i     # bool exactly at scale == 1
        coco = enc.to_coco()
        assert len(coco) == len(enc)
        for j, obj in enumerate(coco):
            assert obj["size"] == list(masks.shape[1:]) and isinstance(obj["counts"], bytes)
            assert np.array_equal(imagelib.rle_decode(obj), want[j].cpu().numpy()), (i, j)
        assert torch.equal(enc.areas.cpu().long(), want.flatten(1).sum(1).cpu()), i
        total += len(enc)
    print(f"detect: {total} detections over {len(images)} images")
    assert total >= min_total
    return rle


def test_detect_rle_same_size_and_mixed_batches(ops, monkeypatch):
    net = small_net()
    rng = np.random.default_rng(19)
    same = [rng.integers(0, 256, (300, 480, 3), dtype=np.uint8) for _ in range(3)]
    compare_detect(net, same)
    shapes = ((300, 480, 3), (256, 256, 3), (300, 480, 3), (120, 160, 3), (256, 256, 3), (400, 300, 3))
    mixed = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    first = compare_detect(net, mixed)
    # 256 x 256 images run at scale == 1 (bool masks, threshold 0), the others are resized (grey levels, threshold 127)
    kinds = [r[3].size == (256, 256) for r in first if r[0] is not None]
    print(f"images with detections: {kinds.count(True)} at scale == 1, {kinds.count(False)} resized")
    # the second encode: a default capacity nothing fits into
    calls = []
    real = ops.rle_encode
    monkeypatch.setattr(ops, "rle_default_capacity", lambda h, w: 2)
    monkeypatch.setattr(ops, "rle_encode", lambda *a, **k: (calls.append(k.get("capacity")), real(*a, **k))[1])
    again = compare_detect(net, mixed)
    assert any(c is not None for c in calls) and any(c is None for c in calls)       # overflowed groups were encoded twice
    for a, b in zip(first, again):
        if a[0] is not None:
            assert a[3].to_coco() == b[3].to_coco()
    with pytest.raises(ValueError):
        net.detect(mixed[:1], mask_format="polygon")
    # images with nothing detected keep today's result (no score reaches a confidence of 2)
    monkeypatch.setattr(net.cfg, "detection_min_confidence", 2.0)
    assert net.detect(mixed[:2]) == [(None, None, None, None)] * 2
    assert net.detect(mixed[:2], mask_format="rle") == [(None, None, None, None)] * 2


# ------------------------------------------------------------------------------------------------ 8 the CLI
def test_predict_cli_coco_json(tmp_path, capsys):
    import importlib.util
    import os
    from maskrcnn_amd import image as imagelib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("predict_cli", os.path.join(root, "predict.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    jpg = os.path.join(root, "tests", "golden", "car58a54312d.jpg")
    out, js = str(tmp_path / "det.npz"), str(tmp_path / "det.json")
    res = cli.main(["--random-weights", "--backbone", "resnet50", "--save", out, "--coco-json", js, jpg])
    printed = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    with open(js) as fh:
        records = json.load(fh)
    z = np.load(out)
    n = z["class_ids"].shape[0]
    print(f"predict.py --coco-json: {n} detections")
    assert len(records) == len(res) == n and (len(printed) == n if n else printed == ["no instances"])
    for i, rec in enumerate(records):
        assert set(rec) == {"image_id", "category_id", "bbox", "score", "segmentation"}
        assert rec["image_id"] == "car58a54312d" and rec["category_id"] == int(z["class_ids"][i])
        y1, x1, y2, x2 = z["boxes"][i].tolist()
        assert rec["bbox"] == [round(x1, 1), round(y1, 1), round(x2 - x1, 1), round(y2 - y1, 1)]
        assert rec["score"] == float(z["scores"][i])
        seg = rec["segmentation"]
        assert seg["size"] == [1200, 1920] and isinstance(seg["counts"], str)
        dense = z["masks"][i] if z["masks"].dtype == np.bool_ else z["masks"][i] > 127
        assert np.array_equal(imagelib.rle_decode(seg), dense), i
