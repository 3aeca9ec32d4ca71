"""GPU parity (-m gpu) of the training ground truth made on the device: ops.rle_resample (csrc/gt_masks.hip) and
ground_truth.load_batch. Every comparison is exact (byte / integer work; boxes bit for bit).

(a) load_batch on the device against tests/golden/ground_truth.npz (the reference's own CocoMaskRCNNDataset.load, encode_image,
    encode_masks, encode_boxes), and through targets.rpn_targets / targets.detection_targets against the device="cpu" route.
(b) ops.rle_resample against the composition of ops that are bit-exact with Pillow already: ops.rle_decode -> torch.flip ->
    ops.resize_bilinear_u8 -> paste into zeros. Shapes: the smallest that can still go wrong (rows_for).
(c) the bad-argument messages.
(d) this file once more, in a child pytest, on the schedule-fuzz library."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ_LIB = os.path.join(ROOT, "maskrcnn_amd", "csrc", "build", "variants", "sync_fuzz", "libmaskrcnn_hip.so")
POISON = 0xEE
UNUSABLE, BAD_SIZE, BAD_PLACEMENT, SHRINK_LIMIT = 1, 2, 4, 8


@pytest.fixture(scope="module")
def ops():
    from maskrcnn_amd import ops as o
    return o


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


def encode(mask: np.ndarray) -> np.ndarray:
    """Column-major run lengths of a dense mask, off run first (rleEncode)."""
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)
    change = np.nonzero(flat[1:] != flat[:-1])[0] + 1
    runs = np.diff(np.concatenate([[0], change, [flat.size]]))
    return (np.concatenate([[0], runs]) if flat[0] else runs).astype(np.uint32)


class Row:
    def __init__(self, h, w, new_h, new_w, top, left, flip, runs, num_runs=None):
        self.h, self.w, self.geom, self.runs = h, w, (new_h, new_w, top, left, int(flip)), np.asarray(runs, np.uint32)
        self.num_runs = self.runs.size if num_runs is None else num_runs


def table(rows, capacity=None):
    capacity = capacity or max(1, max(r.runs.size for r in rows))
    counts = np.zeros((len(rows), capacity), np.uint32)
    for k, r in enumerate(rows):
        m = min(r.runs.size, capacity)
        counts[k, :m] = r.runs[:m]
    return (dev([r.num_runs for r in rows], np.int32), dev(counts.view(np.int32)), dev([r.h for r in rows], np.int32),
            dev([r.w for r in rows], np.int32), dev([r.geom for r in rows], np.int32).reshape(len(rows), 5))


def composed(ops, rows, num_runs, counts, H, W):
    """What the parent commit offers for this job: per row rle_decode, flip, resize_bilinear_u8, a pad copy."""
    out = torch.zeros(len(rows), H, W, dtype=torch.uint8, device=DEV)
    for k, r in enumerate(rows):
        new_h, new_w, top, left, flip = r.geom
        m = ops.rle_decode(num_runs[k:k + 1], counts[k:k + 1], r.h, r.w)
        if flip:
            m = torch.flip(m, dims=[2])
        if (new_h, new_w) != (r.h, r.w):
            m = ops.resize_bilinear_u8(m[0].contiguous(), new_h, new_w)[None]      # 2-d: a [1,h,w<=4] tensor would read as [h,w,c]
        out[k, top:top + new_h, left:left + new_w] = m[0]
    return out


def rows_for(H):
    """The rows of one call on an H x H canvas. Resize factors 16/5, 64/47, 64/100 and 64/257 on the 64 canvas, the same sources
    at 130/47, 130/100 and 130/257 on the 130 one (both canvases cross tile borders of any tile up to 64); identity on one axis
    only and on both; 1-pixel sources; odd and even top / left; every shape flipped and not."""
    rng = np.random.default_rng(1234 + H)
    shapes = [(1, 1, 1, 1), (1, 1, 5, 9), (1, 7, 1, 22), (7, 1, 22, 1), (1, 7, 4, 7), (7, 1, 7, 3), (5, 3, 16, 10),
              (5, 3, 5, 10), (5, 3, 16, 3)]
    if H == 64:
        shapes += [(33, 47, 45, 64), (100, 70, 64, 45), (257, 129, 64, 32), (33, 47, 33, 47), (33, 47, 33, 64), (33, 47, 45, 47)]
    else:
        shapes += [(33, 47, 91, 130), (100, 70, 130, 91), (257, 129, 130, 65), (100, 70, 100, 70), (100, 70, 130, 70), (100, 70, 100, 91),
                   (257, 129, 129, 129)]
    rows = []
    for i, (h, w, nh, nw) in enumerate(shapes):
        for flip in (0, 1):
            top = (H - nh) // 2 if i % 3 else min(H - nh, 2 * i + 1)           # centred (odd and even pads), or an odd offset
            left = (H - nw) // 2 if i % 3 else min(H - nw, 2 * i + 3)
            mask = rng.random((h, w)) < (0.5 if i % 2 else 0.15)               # half on: a run per pixel or so
            mask[0, 0] = mask[-1, -1] = True                                    # touches the corners
            rows.append(Row(h, w, nh, nw, top, left, flip, encode(mask)))
    h, w = 33, 47
    rows.append(Row(h, w, 45, 64, 3, 0, 1, [h * w]))                            # all off
    rows.append(Row(h, w, 45, 64, 3, 0, 0, [0, h * w]))                         # all on
    rows.append(Row(h, w, 45, 64, 0, 0, 0, [5, 7, 9], num_runs=-1))             # refused upstream
    rows.append(Row(h, w, 45, 64, 0, 0, 1, encode(rng.random((h, w)) < 0.5), num_runs=1 << 20))    # over its capacity
    rows.append(Row(h, w, 45, 64, 1, 0, 1, [2 * h + 5, 7 * h + 3, 4 * h - 1, 11 * h + 2, h * w - (24 * h + 9)]))   # runs that cross columns
    rows.append(Row(h, w, 45, 64, 1, 0, 0, [h, 3, h * w]))                      # runs past h*w are clipped
    rows.append(Row(h, w, 45, 64, 1, 0, 0, [h, 3]))                             # pixels the runs do not reach are 0
    return rows


@pytest.fixture(scope="module", params=[64, 130])
def call(request, ops):
    """One rle_resample call per canvas into a poisoned `out`, with the composition it is compared with, shared by the tests."""
    H = request.param
    rows = rows_for(H)
    num_runs, counts, hs, ws, geom = table(rows)
    out = torch.full((len(rows), H, H), POISON, dtype=torch.uint8, device=DEV)
    masks, status = ops.rle_resample(num_runs, counts, hs, ws, geom, H, H, out=out)
    assert masks is out
    return rows, (num_runs, counts, hs, ws, geom), H, masks.cpu().numpy(), status.cpu().numpy(), composed(ops, rows, num_runs, counts, H, H).cpu().numpy()


def test_resample_equals_decode_flip_resize_paste(call):
    rows, _, H, got, status, want = call
    refused = np.array([not 0 <= r.num_runs <= 1 << 19 for r in rows])
    assert status.tolist() == np.where(refused, UNUSABLE, 0).tolist()
    assert not got[refused].any()
    assert want[~refused].any(axis=(1, 2)).sum() >= len(rows) - 5          # the comparison is not of zeros with zeros
    for k, r in enumerate(rows):
        assert np.array_equal(got[k], want[k]), (k, r.h, r.w, r.geom, np.argwhere(got[k] != want[k])[:5].tolist())
    assert set(np.unique(got).tolist()) <= {0, 1}


def test_resample_twice_gives_the_same_bytes_and_allocates_its_own_output(call, ops):
    rows, args, H, got, status, _ = call
    masks, st = ops.rle_resample(*args, H, H)
    assert masks.shape == (len(rows), H, H) and masks.dtype == torch.uint8 and masks.is_contiguous()
    assert np.array_equal(masks.cpu().numpy(), got) and np.array_equal(st.cpu().numpy(), status)


def test_resample_into_a_view_with_odd_strides_writes_its_extent_only(call, ops):
    rows, args, H, got, _, _ = call
    n, rs = len(rows), H + 5
    ims = (H + 3) * rs + 1
    buf = torch.full((3 + n * ims + 64,), POISON, dtype=torch.uint8, device=DEV)
    view = buf.as_strided((n, H, H), (ims, rs, 1), 3)
    masks, _ = ops.rle_resample(*args, H, H, out=view)
    assert masks is view and np.array_equal(view.cpu().numpy(), got)
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside.as_strided((n, H, H), (ims, rs, 1), 3)[:] = True
    assert bool((buf[~inside] == POISON).all())


def test_each_refusal_has_its_bit_a_zero_mask_and_intact_neighbours(ops):
    H, W = 40, 72                                                               # not square, not a multiple of the tile
    good = lambda s: Row(20, 30, 27, 40, 5, 7, s & 1, encode(np.random.default_rng(s).random((20, 30)) < 0.4))
    on = [0, 600]
    rows = [good(1), Row(20, 30, 27, 40, 5, 7, 0, on, num_runs=-1), good(2), Row(20, 30, 27, 40, 5, 7, 0, on, num_runs=3),
            Row(0, 30, 27, 40, 5, 7, 0, on), Row(20, 16385, 27, 40, 5, 7, 0, on), Row(20, 30, 0, 40, 5, 7, 0, on),
            Row(20, 30, 27, 16385, 5, 7, 0, on), good(3), Row(20, 30, 27, 40, 14, 7, 0, on), Row(20, 30, 27, 40, 5, 33, 0, on),
            Row(20, 30, 27, 40, -1, 7, 0, on), Row(20, 30, 27, 40, 5, -1, 0, on), good(4), Row(20, 30, 1, 40, 5, 7, 0, on),
            Row(20, 30, 27, 1, 5, 7, 0, on), Row(16, 32, 1, 2, 5, 7, 0, [0, 512]), Row(17, 32, 1, 2, 5, 7, 0, [0, 544]), good(5)]
    want_status = [0, UNUSABLE, 0, UNUSABLE, BAD_SIZE, BAD_SIZE, BAD_SIZE, BAD_SIZE | BAD_PLACEMENT, 0, BAD_PLACEMENT,
                   BAD_PLACEMENT, BAD_PLACEMENT, BAD_PLACEMENT, 0, SHRINK_LIMIT, SHRINK_LIMIT, 0, SHRINK_LIMIT, 0]
    num_runs, counts, hs, ws, geom = table(rows, capacity=2)                    # row 3: more runs than the capacity
    full = table(rows)
    out = torch.full((len(rows), H, W), POISON, dtype=torch.uint8, device=DEV)
    masks, status = ops.rle_resample(full[0], full[1], hs, ws, geom, H, W, out=out)
    got = masks.cpu().numpy()
    assert status.cpu().numpy().tolist() == [0 if k == 3 else s for k, s in enumerate(want_status)]
    ok = [k for k, s in enumerate(want_status) if s == 0 or k == 3]
    want = composed(ops, [rows[k] for k in ok], full[0][ok], full[1][ok], H, W).cpu().numpy()
    for j, k in enumerate(ok):
        assert np.array_equal(got[k], want[j]), k
    assert all(not got[k].any() for k, s in enumerate(want_status) if s and k != 3)
    # with a capacity of 2 every random row is over its capacity as well: all but the [0, area] rows are refused
    masks2, status2 = ops.rle_resample(num_runs, counts, hs, ws, geom, H, W)
    st2 = status2.cpu().numpy()
    assert st2[[0, 2, 8, 13, 18]].tolist() == [UNUSABLE] * 5 and st2[3] == UNUSABLE and st2[16] == 0
    assert np.array_equal(masks2[16].cpu().numpy(), got[16]) and not masks2[[0, 2, 3]].any()


def test_no_rows_launch_nothing(ops):
    e = lambda *s: torch.empty(*s, dtype=torch.int32, device=DEV)
    masks, status = ops.rle_resample(e(0), e(0, 4), e(0), e(0), e(0, 5), 64, 48)
    assert masks.shape == (0, 64, 48) and masks.dtype == torch.uint8 and status.shape == (0,) and status.dtype == torch.int32


def test_bad_arguments_are_refused_before_any_launch(ops):
    rows = rows_for(64)[:3]
    num_runs, counts, hs, ws, geom = table(rows)
    n = len(rows)

    def message(*args, **kw):
        with pytest.raises(RuntimeError) as e:
            ops.rle_resample(*args, **kw)
        return str(e.value)

    assert message(num_runs, counts, hs.float(), ws, geom, 64, 64) == f"rle_resample: heights must be int32 [{n}], got float32 [{n}]"
    assert message(num_runs, counts, hs, ws[:2], geom, 64, 64) == f"rle_resample: widths must be int32 [{n}], got int32 [2]"
    assert message(num_runs, counts, hs, ws, geom[:, :4], 64, 64) == f"rle_resample: geom must be int32 [{n},5], got int32 [{n}, 4]"
    assert message(num_runs.long(), counts, hs, ws, geom, 64, 64) == f"rle_resample: num_runs must be int32 [N], got int64 [{n}]"
    assert message(num_runs, counts[:2], hs, ws, geom, 64, 64).startswith(f"rle_resample: counts must be int32 [{n},capacity>=1], got int32 [2, ")
    assert message(num_runs, counts, hs, ws, geom, 0, 64) == "rle_resample: out_h, out_w must be in [1, 16384], got 0, 64"
    assert message(num_runs, counts, hs, ws, geom, 64, 16385) == "rle_resample: out_h, out_w must be in [1, 16384], got 64, 16385"
    bad = torch.empty(n, 64, 64, dtype=torch.int8, device=DEV)
    assert message(num_runs, counts, hs, ws, geom, 64, 64, out=bad).startswith(
        f"rle_resample: out tensor out must be uint8 [{n},64,64] on cuda:0, got int8 [{n}, 64, 64]")
    wide = torch.empty(n, 64, 128, dtype=torch.uint8, device=DEV)[:, :, ::2]
    assert message(num_runs, counts, hs, ws, geom, 64, 64, out=wide) == \
        "rle_resample: out tensor out must have unit last stride, got strides (8192, 128, 2)"
    assert "Not compiled with CPU support" in message(num_runs.cpu(), counts.cpu(), hs.cpu(), ws.cpu(), geom.cpu(), 64, 64)


# --------------------------------------------------------------------------------------------------------- (a) load_batch
@pytest.fixture(scope="module")
def fixture_cases():
    from test_ground_truth_host import fixture_cases as cases
    return cases()


def test_load_batch_on_the_device_equals_the_reference(fixture_cases):
    from maskrcnn_amd import ground_truth
    from test_ground_truth_host import same_as_fixture
    for case in fixture_cases:
        got = ground_truth.load_batch(case.gt, case.image_ids, case.min_dim, case.max_dim, hflip=case.flips, crowds="reference",
                                      labels=case.labels, device=DEV)
        assert all(t.device == DEV for t in got[:5])
        same_as_fixture(got, case)


def test_targets_take_the_device_ground_truth_and_agree_with_the_host_route(fixture_cases):
    """The GroundTruth goes into targets.rpn_targets / targets.detection_targets as it is; the outputs equal those of the
    device="cpu" ground truth (numpy and Pillow), moved to the device and run through the same functions with the same keys."""
    from maskrcnn_amd import ground_truth, targets
    for case in (fixture_cases[0], fixture_cases[3]):
        args = (case.gt, case.image_ids, case.min_dim, case.max_dim)
        on_dev = ground_truth.load_batch(*args, hflip=case.flips, labels=case.labels, device=DEV)
        on_cpu = ground_truth.load_batch(*args, hflip=case.flips, labels=case.labels, device="cpu")
        for a, b in zip(on_dev[:5], on_cpu[:5]):
            assert a.dtype == b.dtype and a.device == DEV and torch.equal(a.cpu(), b)
        assert on_dev.scales == on_cpu.scales and on_dev.flips == on_cpu.flips and bool((on_dev.gt_class_ids < 0).any())
        B, D, A, N = len(case.image_ids), case.max_dim, 96, 40
        g = torch.Generator().manual_seed(7)
        anchors = torch.rand(A, 4, generator=g, dtype=torch.float64) * (D / 2)
        anchors[:, 2:] += anchors[:, :2] + 2
        rois = torch.rand(B, N, 4, generator=g) * (D / 2)
        rois[..., 2:] += rois[..., :2] + 3
        off = on_cpu.gt_off.tolist()
        for i in range(B):                                       # some RoIs are ground-truth boxes: there are positives
            k = min(off[i + 1] - off[i], 4)
            rois[i, :k] = on_cpu.gt_boxes[off[i]:off[i] + k]
        keys_a = torch.randint(0, 2 ** 31 - 1, (B, A), generator=g, dtype=torch.int32)
        keys_r = torch.randint(0, 2 ** 31 - 1, (B, N), generator=g, dtype=torch.int32)
        outs = []
        for gt in (on_dev, ground_truth.GroundTruth(*[t.to(DEV) for t in on_cpu[:5]], on_cpu.scales, on_cpu.flips)):
            r = targets.rpn_targets(anchors.to(DEV), gt.gt_boxes, gt.gt_class_ids, count=32, keys=keys_a.to(DEV), gt_off=gt.gt_off)
            d = targets.detection_targets(rois.to(DEV), gt.gt_boxes, gt.gt_class_ids, gt.gt_masks, count=24, keys=keys_r.to(DEV),
                                          gt_off=gt.gt_off)
            outs.append([*r, *d])
        assert len(outs[0]) == 11 and outs[0][0].shape == (B, A, 1) and outs[0][5].shape == (B, 24, 28, 28)
        assert bool((outs[0][0] == 1).any()) and bool((outs[0][8] > 0).any())        # positives on both sides: not all padding
        for a, b in zip(*outs):
            assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------- (d) schedule fuzzing
# The child's time limit: four times the wall time measured on the fuzzed library, rounded up to 30 s: 4.1 s (11 tests; 2.9 s of
# it inside pytest, the rest start-up), so 16.4 s -> 30 s.
FUZZ_TIMEOUT = 30


@pytest.mark.skipif(os.environ.get("MRCNN_SYNC_FUZZ_CHILD") == "1", reason="this IS the fuzzed child run")
def test_this_file_passes_under_schedule_fuzzing():
    """Every barrier of rle_resample_tile_kernel — between the coefficients and their readers, the fill and the horizontal pass,
    the two passes, the last sub-tile and the store — is followed by a random sleep per wave on that build; a hand-off a barrier
    does not order fails its comparison there."""
    assert os.path.exists(FUZZ_LIB), f"{FUZZ_LIB} is missing: run __graft_entry__.build()"
    env = dict(os.environ, MRCNN_LIB=FUZZ_LIB, MRCNN_SYNC_FUZZ_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_ground_truth.py", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=FUZZ_TIMEOUT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
